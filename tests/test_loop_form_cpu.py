"""CPU: ``pipeline._choose_form`` -- the one place that decides which launch sequence a FusedRenderAndCompare runs --
against tests/loop_form_twin.py, the restatement of the predicates the constructor used to hold, over the whole grid of
options; and the decisions the GPU tests state outright.  No GPU, no library load."""
import itertools

import pytest

import loop_form_twin as twin
from sdfest_amd import _lib
from sdfest_amd.pipeline import FORMS, _choose_form

SMALL, DET = _lib.ABI["SDFR_BWD_SMALL_TILES"], _lib.ABI["SDFR_SDF_GRAD_DETERMINISTIC"]
TRI = (None, False, True)
# (world, rank, a process group): without a group; a group of one; the first and the last rank of 2 and of 3 -- the
# first rank's shard has a view whenever the split leaves one, the last one's is the first to be empty
RANKS = ((1, 0, False), (1, 0, True), (2, 0, True), (2, 1, True), (3, 0, True), (3, 2, True))
GRID = dict(V_all=(1, 4, 7, 8, 9, 32, 64, 65), ranks=RANKS, latent=(8, 248, 249), R=(64, 128, 129),
            narrow=(False, True), shape_opt=(False, True), sdf_grad_mode=(0, 1, SMALL, DET | SMALL, DET),
            form=("auto", "tail", "records"), fuse_depth_loss=(True, False), merge_launches=(True, False),
            fused_render=TRI, fc_in_tail=TRI, defer_loss=TRI, exchange=("sdf", "latent"))
FACTS = ("records_form", "defer_pose", "defer_loss", "fused_render", "fc_in_tail", "big_exchange", "det")


def both(V_all, ranks, latent, R, narrow, shape_opt, sdf_grad_mode, form, fuse_depth_loss, merge_launches,
         fused_render, fc_in_tail, defer_loss, exchange):
    """(what the twin says, what _choose_form says): each a tuple of the form's name, FACTS and how often the decoder
    was asked for its Linear stack -- or the text of the ValueError"""
    world, rank, grouped = ranks
    try:
        t = twin.decide(V_all, rank, world, grouped, latent, R, narrow, shape_opt, sdf_grad_mode, form,
                        fuse_depth_loss, merge_launches, fused_render, fc_in_tail, defer_loss, exchange)
        want = (t["form"],) + tuple(t[k] for k in FACTS) + (t["asked"],)
    except ValueError as e:
        want = str(e)
    b, e = twin.shard(V_all, rank, world)
    asked = []

    def narrow_linear_stack():
        asked.append(1)
        return narrow
    try:
        f = _choose_form(V_all, e - b, world, grouped, latent, R, shape_opt, sdf_grad_mode, form, fuse_depth_loss,
                         merge_launches, fused_render, fc_in_tail, defer_loss, exchange, narrow_linear_stack)
        got = (f.name,) + tuple(getattr(f, k) for k in FACTS) + (len(asked),)
    except ValueError as e:
        got = str(e)
    return want, got


def test_the_twin_reads_the_header_s_flags():
    assert (twin.BWD_SMALL_TILES, twin.SDF_GRAD_DETERMINISTIC) == (SMALL, DET)


def test_choose_form_is_the_constructor_s_predicates_on_the_whole_grid():
    """every point of GRID: the same ValueError text, or the same form, the same seven facts and the same number of
    questions to the decoder.  Not thinned: nine points in ten raise, and every point that raises is to be kept (about
    20 s of plain arithmetic)."""
    n = raised = 0
    seen = set()
    for point in itertools.product(*GRID.values()):
        want, got = both(*point)
        assert want == got, (dict(zip(GRID, point)), want, got)
        n += 1
        if isinstance(want, str):
            raised += 1
        else:
            assert want[0] in FORMS and type(want[1]) is bool
            seen.add(want[0])
    assert n == 5598720 and raised > 0 and seen == set(FORMS), (n, raised, seen)


def choose(V_all=2, V=None, world=1, grouped=False, latent=8, R=64, shape_opt=True, sdf_grad_mode=0, form="auto",
           fuse_depth_loss=True, merge_launches=True, fused_render=None, fc_in_tail=None, defer_loss=None,
           exchange="sdf", narrow=True):
    return _choose_form(V_all, V_all if V is None else V, world, grouped, latent, R, shape_opt, sdf_grad_mode, form,
                        fuse_depth_loss, merge_launches, fused_render, fc_in_tail, defer_loss, exchange, lambda: narrow)


def test_the_decisions_the_gpu_tests_state():
    for V in (1, 4):        # tests/test_loop_decoders_gpu.py, tests/test_fused_render_gpu.py
        assert choose(V).name == "fc_in_tail" and choose(V, narrow=False).name == "one_launch"
    assert choose(7).name == "tail"                                   # shape optimisation: fused only up to 4 views
    assert choose(7, shape_opt=False).name == "one_launch"
    assert choose(8).name == "records" and choose(8, form="tail").name == "tail"
    assert choose(8, form="tail", fused_render=True).fused_render     # SDFR_FUSED_MAX_VIEWS
    assert choose(2, grouped=True).name == "records" and choose(4, V=2, world=2, grouped=True).name == "records"
    assert choose(2, merge_launches=False).name == "separate" and choose(2, fuse_depth_loss=False).name == "separate"
    with pytest.raises(ValueError, match="parameter vectors of up to 256 entries, this decoder's latent makes 257"):
        choose(2, latent=249, form="records")
    for kw in ({}, dict(form="tail"), dict(merge_launches=False)):    # latent 249 otherwise: the separate launches
        assert choose(2, latent=249, **kw).name == "separate"
    assert choose(8, latent=249).name == "separate"
    big = choose(2, form="records", sdf_grad_mode=DET | SMALL)
    assert big.big_exchange and big.det and not choose(2, form="records", exchange="latent").big_exchange
