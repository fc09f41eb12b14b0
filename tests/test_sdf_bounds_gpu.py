"""GPU: sdfr_sdf_bounds (csrc/boxes.hip) through sdfest_amd.sdf_bounds -- the bounds of a grid's iso-surface are bitwise
the minimum and maximum of the vertices marching cubes emits for it (one statement of the arithmetic,
csrc/mesh_grid.hpp), for a grid alone or in a batch, whatever the outputs held; and SDFPipeline.bounding_boxes against
generate_meshes + Mesh.oriented_box."""
import numpy as np
import pytest
import torch

import _loop_scenes as S

pytestmark = pytest.mark.gpu


def sphere(R, radius, centre=(0.0, 0.0, 0.0)):
    a = np.linspace(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(a, a, a, indexing="ij")
    return (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius).astype(np.float32)


def grids(R, level):
    """name -> (R,R,R) float32: a sphere inside, one that leaves the volume (crossings on the last edges when the
    volume is padded), one with a corner value exactly at the level, one the level does not cross"""
    leaving = sphere(R, 0.9, (0.45, -0.3, 0.2))
    corner = sphere(R, 0.55, (0.1, 0.05, -0.1))
    corner[R // 2, R // 2, 1] = level
    corner[R // 3, R // 2, R // 2] = level          # one inside the ball too
    return {"sphere": sphere(R, 0.6), "leaving": leaving, "corner": corner,
            "positive": np.full((R, R, R), 0.5, np.float32) + level}


def mesh_bounds(grid, level, complete):
    """(lo, hi, V) from the emitted vertices; (+inf, -inf, 0) where marching cubes has nothing to emit"""
    from sdfest_amd import extract_mesh
    try:
        v = extract_mesh(grid, level, complete=complete).vertices
    except ValueError:          # the level outside the grid's range
        v = grid.new_zeros((0, 3))
    if v.shape[0] == 0:
        inf = torch.full((3,), float("inf"), device=grid.device)
        return inf, -inf, 0
    return v.amin(0), v.amax(0), int(v.shape[0])


@pytest.mark.parametrize("level", [0.0, 0.07])
@pytest.mark.parametrize("complete", [False, True])
@pytest.mark.parametrize("R", [8, 9])
def test_bounds_are_bitwise_the_mesh_vertices_minimum_and_maximum(R, complete, level):
    from sdfest_amd import sdf_bounds
    named = grids(R, level)
    dev = torch.device("cuda")
    alone = {}
    for name, g in named.items():
        t = torch.tensor(g, device=dev)
        lo, hi, crossed = sdf_bounds(t, level, complete=complete)                     # N = 1
        assert lo.shape == hi.shape == (1, 3) and crossed.shape == (1,) and crossed.dtype == torch.int32
        mlo, mhi, V = mesh_bounds(t, level, complete)
        assert int(crossed[0]) == V, name
        assert torch.equal(lo[0].view(torch.int32), mlo.view(torch.int32)), (name, lo, mlo)
        assert torch.equal(hi[0].view(torch.int32), mhi.view(torch.int32)), (name, hi, mhi)
        if name == "positive":
            assert V == 0 and bool(torch.isinf(lo).all()) and bool((lo > 0).all()) and bool((hi < 0).all())
        else:
            assert V > 0
        alone[name] = (lo[0], hi[0], int(crossed[0]))
    # the padded volume closes the sphere that leaves the grid: its bounds reach the border layer
    if complete:
        assert float(alone["leaving"][1][0]) > 1.0
    # N = 3 different grids: grid k in the batch is bitwise grid k alone
    names = ["leaving", "positive", "corner"]
    batch = torch.tensor(np.stack([named[n] for n in names]), device=dev)
    lo, hi, crossed = sdf_bounds(batch, level, complete=complete)
    for k, n in enumerate(names):
        assert torch.equal(lo[k].view(torch.int32), alone[n][0].view(torch.int32))
        assert torch.equal(hi[k].view(torch.int32), alone[n][1].view(torch.int32))
        assert int(crossed[k]) == alone[n][2]


def test_outputs_may_hold_anything_and_calls_repeat():
    """the C ABI on outputs pre-filled with 0xFF bytes, twice"""
    from sdfest_amd import _lib, sdf_bounds
    dev = torch.device("cuda")
    named = grids(9, 0.0)
    batch = torch.tensor(np.stack([named["sphere"], named["positive"], named["leaving"]]), device=dev)
    lo, hi, crossed = sdf_bounds(batch, 0.0, complete=True)
    for _ in range(2):
        bounds = torch.full((3, 6), -1, dtype=torch.int32, device=dev)      # 0xFF bytes
        count = torch.full((3,), -1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().sdfr_sdf_bounds(batch.data_ptr(), 3, 9, 1, 0.0, bounds.data_ptr(), count.data_ptr(), 0,
                                              torch.cuda.current_stream().cuda_stream), "sdfr_sdf_bounds")
        assert torch.equal(bounds[:, :3], lo.view(torch.int32)) and torch.equal(bounds[:, 3:], hi.view(torch.int32))
        assert torch.equal(count, crossed)
    # N = 0: nothing happens
    empty = sdf_bounds(batch[:0], 0.0)
    assert empty[0].shape == (0, 3) and empty[2].shape == (0,)


@pytest.fixture(scope="module")
def pipeline():
    from sdfest_amd import SDFPipeline
    from test_sdfpipeline_gpu import make_config, mug_weights, plausible_init_state
    cfg = make_config(160, 120, 150.0, 150.0, 80.0, 60.0, 0.005, 2)
    return SDFPipeline(cfg, vae_state_dict=mug_weights(), init_state_dict=plausible_init_state())


def test_a_decoded_mug_at_64(pipeline):
    from sdfest_amd import sdf_bounds
    _, d = S.mug_decoder()
    level = pipeline.config["iso_threshold"]
    with torch.no_grad():
        sdf = pipeline.vae.decode(torch.tensor(d["z"][9:10] * 0.5, dtype=torch.float32, device="cuda"))[0, 0]
    assert sdf.shape == (64, 64, 64)
    for complete in (False, True):
        lo, hi, crossed = sdf_bounds(sdf, level, complete=complete)
        mlo, mhi, V = mesh_bounds(sdf, level, complete)
        assert V > 1000 and int(crossed[0]) == V
        assert torch.equal(lo[0].view(torch.int32), mlo.view(torch.int32))
        assert torch.equal(hi[0].view(torch.int32), mhi.view(torch.int32))


def test_pipeline_bounding_boxes_against_the_meshes(pipeline):
    _, d = S.mug_decoder()
    dev = torch.device("cuda")
    latent = torch.tensor(np.stack([d["z"][9] * 0.5, d["z"][3] * 0.7]), dtype=torch.float32, device=dev)
    scale = torch.tensor([0.055, 0.12], device=dev)
    position = torch.tensor([[0.02, -0.01, -0.5], [-0.3, 0.1, -0.9]], device=dev)
    orientation = torch.nn.functional.normalize(torch.tensor([[0.2, 0.6, -0.15, 0.75], [-0.3, 0.5, 0.6, 0.4]], device=dev))
    center, box_orientation, extents = pipeline.bounding_boxes(position, orientation, scale, latent)
    assert center.shape == (2, 3) and box_orientation.shape == (2, 4) and extents.shape == (2, 3)
    assert center.dtype == extents.dtype == torch.float64 and torch.equal(box_orientation, orientation.double())
    from sdfest_amd.pipeline import quaternion_apply, quaternion_invert
    meshes = pipeline.generate_meshes(latent, scale, complete_mesh=True)
    for k, mesh in enumerate(meshes):
        c, q, e = mesh.oriented_box(position[k], orientation[k])
        slack = 1e-6 * float(scale[k])
        assert float((center[k] - c).abs().max()) <= slack and float((extents[k] - e).abs().max()) <= slack
        # every posed vertex lies in the box (the pose applied in float64, as the box's is)
        v = mesh.scaled_vertices().double()
        turn = orientation[k].double().reshape(1, 4).expand(v.shape[0], 4)
        local = quaternion_apply(quaternion_invert(turn), quaternion_apply(turn, v) + position[k].double() - center[k])
        assert bool((local.abs() <= extents[k] / 2 + slack).all())
    # K = 1 (the 4-tuple of __call__) is row 0 (a decode of one latent may round otherwise than a batched one: 1e-4 of
    # the scale), and the open mesh's box too
    one = pipeline.bounding_boxes(position[:1], orientation[:1], scale[:1], latent[:1])
    assert all(o.shape == b[:1].shape and float((o[0] - b[0]).abs().max()) <= 1e-4 * float(scale[0])
               for o, b in zip(one, (center, box_orientation, extents)))
    assert pipeline.bounding_boxes(position, orientation, scale, latent, complete_mesh=False)[2].shape == (2, 3)
    # no iso_threshold: None, as generate_mesh; a level no grid edge crosses: ValueError naming the row
    config = pipeline.config
    try:
        pipeline.config = {k: v for k, v in config.items() if k != "iso_threshold"}
        assert pipeline.bounding_boxes(position, orientation, scale, latent) is None
        pipeline.config = dict(config, iso_threshold=50.0)
        with pytest.raises(ValueError, match="row 0"):
            pipeline.bounding_boxes(position, orientation, scale, latent)
    finally:
        pipeline.config = config
