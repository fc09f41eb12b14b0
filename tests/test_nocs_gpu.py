"""GPU: the NOCS annotation kernels (sdfest_amd/csrc/nocs.hip) and their host functions (sdfest_amd/nocs_utils.py).

The fit is compared with the reference's recorded runs (tests/golden/nocs_ransac.npz: the reference's own draws are
fed to the kernel).  Choices -- status, winner, iterations run, inlier set, inlier ratio -- equal exactly; position,
rotation, scale and transform to ATOL = 1e-10 absolute, the bound of the reference's own test_nocs_utils.py, which
the conditioning asserted by tools/make_nocs_goldens.py makes legitimate for another fp64 implementation.  The
correspondences are compared bit for bit with tests/nocs_twin.py."""
import os

import numpy as np
import pytest
import torch

import nocs_twin as tw
from helpers import GOLDEN
from test_nocs_cpu import CASES

pytestmark = pytest.mark.gpu

ATOL = 1e-10
G = [f"g{i}" for i in range(5)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def frame():
    f = np.load(os.path.join(GOLDEN, "nocs_frame.npz"))
    return {k: f[k] for k in f.files}


def run_batch(names, dev, dtype=None):
    """one call over the named golden cases (all of one dtype); host copies of every result"""
    from sdfest_amd import nocs_utils as nu
    src = np.concatenate([CASES[n]["source"] for n in names])
    tgt = np.concatenate([CASES[n]["target"] for n in names])
    assert src.dtype == tgt.dtype and all(CASES[n]["source"].dtype == src.dtype for n in names)
    offsets = np.concatenate([[0], np.cumsum([len(CASES[n]["source"]) for n in names])]).tolist()
    draws = torch.tensor(np.stack([CASES[n]["draws"] for n in names]), dtype=torch.int32, device=dev)
    r = nu.estimate_similarity_transforms(torch.tensor(src, device=dev), torch.tensor(tgt, device=dev), offsets,
                                          sample_indices=draws, with_inlier_mask=True)
    torch.cuda.synchronize()
    host = {k: getattr(r, k).cpu().numpy() for k in r._fields}
    host["offsets"] = offsets
    return host


def check_against_golden(name, h, k):
    c = CASES[name]
    a, b = h["offsets"][k], h["offsets"][k + 1]
    assert h["status"][k] == int(c["status"]), name
    assert h["iterations_run"][k] == int(c["iterations_run"]), name
    if int(c["status"]) == tw.POSE_ERROR:
        return
    assert h["best_iteration"][k] == int(c["best_iteration"]), name
    assert np.array_equal(np.nonzero(h["inlier_mask"][a:b])[0], c["inlier_idx"]), name
    assert h["inlier_ratio"][k] == float(c["inlier_ratio"]), name
    if int(c["status"]) == tw.OK:
        for ours, key in (("position", "position"), ("rotation_matrix", "rotation"), ("scale", "scale"),
                          ("transform", "transform")):
            err = np.max(np.abs(h[ours][k] - c[key]))
            print(f"{name} {key}: max abs error {err:.3e}")
            assert err <= ATOL, (name, key, err)
    else:
        assert np.all(np.isnan(h["position"][k])) and np.all(np.isnan(h["transform"][k]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_equals_the_reference_on_its_own_draws(name, dev):
    check_against_golden(name, run_batch([name], dev), 0)


@pytest.fixture(scope="module")
def singles(dev):
    return {n: run_batch([n], dev) for n in G}


RESULTS = ("position", "rotation_matrix", "scale", "transform", "inlier_ratio", "status", "best_iteration",
           "iterations_run")


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4], [3, 0, 4, 2, 1]])
def test_a_batch_equals_its_single_calls_bit_for_bit(order, dev, singles):
    names = [G[i] for i in order]
    h = run_batch(names, dev)
    for k, n in enumerate(names):
        check_against_golden(n, h, k)
        for key in RESULTS:
            assert h[key][k].tobytes() == singles[n][key][0].tobytes(), (n, key)
        a, b = h["offsets"][k], h["offsets"][k + 1]
        assert np.array_equal(h["inlier_mask"][a:b], singles[n]["inlier_mask"])


def test_mixed_small_cases_in_one_batch(dev):
    """sets of 5, 4, 10, 40 and 20 points side by side: every status of the fp64 cases in one call"""
    names = ["b5", "b4", "a", "d", "f"]
    h = run_batch(names, dev)
    for k, n in enumerate(names):
        check_against_golden(n, h, k)


def test_correspondences_equal_the_twin_bit_for_bit(dev, frame):
    from sdfest_amd import Camera
    from sdfest_amd import nocs_utils as nu
    depth = frame["depth_mm"].astype(np.float32) * np.float32(0.001)
    cam = Camera(**tw.REAL_CAMERA)
    ids = [int(i) for i in frame["meta_mask_id"]] + [77]        # 77: no such object
    for coord in (frame["coord"], np.concatenate([frame["coord"][..., :3], np.full_like(frame["coord"][..., :1], 255)], -1)):
        c = nu.nocs_correspondences(torch.tensor(depth, device=dev), torch.tensor(frame["mask"], device=dev),
                                    torch.tensor(np.ascontiguousarray(coord), device=dev), ids, cam)
        src, tgt, off = c.source.cpu().numpy(), c.target.cpu().numpy(), c.offsets.cpu().numpy()
        assert c.counts[-1] == 0 and c.max_depth[-1] == 0.0
        for k, mid in enumerate(ids[:-1]):
            s, t, zmax = tw.correspondences(depth, frame["mask"], coord, mid)
            assert c.counts[k] == len(s) and off[k + 1] - off[k] == len(s)
            assert src[off[k]:off[k + 1]].tobytes() == s.tobytes()
            assert tgt[off[k]:off[k + 1]].tobytes() == t.tobytes()
            assert c.max_depth[k] == np.float32(zmax)


def test_correspondences_of_an_odd_image(dev):
    """33 x 37 pixels (no multiple of the 1024-pixel block; two blocks), zero depths inside the mask"""
    from sdfest_amd import Camera
    from sdfest_amd import nocs_utils as nu
    rng = np.random.default_rng(3)
    H, W = 37, 33
    depth = rng.uniform(0.5, 2.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.2] = 0
    mask = rng.integers(0, 3, (H, W)).astype(np.uint8)
    coord = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    cam = dict(width=W, height=H, fx=40.3, fy=41.7, cx=16.2, cy=18.9, pixel_center=0.0)
    c = nu.nocs_correspondences(torch.tensor(depth, device=dev), torch.tensor(mask, device=dev),
                                torch.tensor(coord, device=dev), [2, 0, 1], Camera(**cam))
    off = c.offsets.cpu().numpy()
    for k, mid in enumerate([2, 0, 1]):
        s, t, zmax = tw.correspondences(depth, mask, coord, mid, cam)
        assert len(s) > 100 and c.counts[k] == len(s)
        assert c.source[off[k]:off[k + 1]].cpu().numpy().tobytes() == s.tobytes()
        assert c.target[off[k]:off[k + 1]].cpu().numpy().tobytes() == t.tobytes()
        assert c.max_depth[k] == np.float32(zmax)


def test_sample_indices(dev):
    from sdfest_amd import nocs_utils as nu
    sizes = [5, 257, 4, 3362, 257, 6]
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    a = nu.draw_sample_indices(off, seed=11).cpu().numpy()
    assert a.shape == (6, 100, 5)
    for k, n in enumerate(sizes):
        if n < 5:
            assert not a[k].any()
            continue
        assert a[k].min() >= 0 and a[k].max() < n
        assert all(len(set(row)) == 5 for row in a[k].tolist())
    assert sorted(a[0, 0].tolist()) == [0, 1, 2, 3, 4]                 # N = 5 terminates with a permutation
    assert np.array_equal(a[1], a[4])                                  # the batch position is not part of the stream
    assert len(np.unique(a[3])) > 400                                  # (and the indices spread over the set)
    assert np.array_equal(a, nu.draw_sample_indices(off, seed=11).cpu().numpy())      # reproducible
    b = nu.draw_sample_indices(off, seed=12).cpu().numpy()
    assert not np.array_equal(a[3], b[3])
    # per-object seeds: an object's rows depend on its own seed and size only
    seeds = torch.tensor([12, 11, 0, 12, 12, 11], dtype=torch.int64, device=dev)
    s = nu.draw_sample_indices(off, object_seeds=seeds).cpu().numpy()
    assert np.array_equal(s[0], b[0]) and np.array_equal(s[1], a[1]) and np.array_equal(s[3], b[3])
    assert np.array_equal(s[4], b[4]) and np.array_equal(s[5], a[5])


def test_reference_signature(dev):
    from sdfest_amd import nocs_utils as nu
    c = CASES["c"]
    # (c): other draws than the golden's, the same inliers up to points at the threshold.  Both fits are least squares
    # over ~180 points with 2e-4 noise per coordinate: they agree to well below 5 sigma = 1e-3
    pos, rot, scale, T = nu.estimate_similarity_transform(c["source"], c["target"], seed=5)
    assert pos.dtype == rot.dtype == T.dtype == np.float64 and isinstance(scale, float)
    assert pos.shape == (3,) and rot.shape == (3, 3) and T.shape == (4, 4)
    for ours, key in ((pos, "position"), (rot, "rotation"), (scale, "scale"), (T, "transform")):
        assert np.max(np.abs(ours - c[key])) < 1e-3, key
    np.testing.assert_allclose(T[:3, :3], scale * rot, atol=1e-15)
    # with the reference's draws: the reference's numbers
    got = nu.estimate_similarity_transform(c["source"], c["target"], sample_indices=c["draws"])
    assert np.max(np.abs(got[3] - c["transform"])) <= ATOL
    e = CASES["e"]
    assert nu.estimate_similarity_transform(e["source"], e["target"]) == (None, None, None, None)
    b4 = CASES["b4"]
    assert nu.estimate_similarity_transform(b4["source"], b4["target"]) == (None, None, None, None)
    f = CASES["f"]
    with pytest.raises(nu.PoseEstimationError):
        nu.estimate_similarity_transform(f["source"], f["target"], sample_indices=f["draws"])


def test_c_abi_clamps_offsets_and_rejects_bad_arguments(dev):
    """offsets outside [0, total] and sample indices outside the set are clamped: nothing is read out of bounds (the
    points sit at the very end of an allocation's used part, guard values behind the outputs stay)"""
    from sdfest_amd import _lib
    L = _lib.lib()
    c = CASES["c"]
    n = len(c["source"])
    src, tgt = torch.tensor(c["source"], device=dev), torch.tensor(c["target"], device=dev)
    K = 3
    off = torch.tensor([-50, n, n + 1000, 5], dtype=torch.int64, device=dev)       # [0, n), [n, n), [n, n) after clamping
    draws = torch.tensor(np.stack([c["draws"], c["draws"] + 10 ** 6, -c["draws"]]), dtype=torch.int32, device=dev)
    out = {k: torch.full((K + 1, m), 7.0, dtype=torch.float64, device=dev) for k, m in
           (("position", 3), ("rotation", 9), ("scale", 1), ("transform", 16), ("ratio", 1))}
    ints = {k: torch.full((K + 1,), 7, dtype=torch.int32, device=dev) for k in ("best", "ran", "status")}
    mask = torch.full((n + 64,), 7, dtype=torch.uint8, device=dev)
    need = L.sdfr_similarity_ransac_workspace_bytes(K, n, n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda **kw: L.sdfr_similarity_ransac(
        kw.get("src", src.data_ptr()), tgt.data_ptr(), kw.get("dtype", 0), off.data_ptr(), kw.get("total", n),
        kw.get("max_n", n), kw.get("K", K), draws.data_ptr(), out["position"].data_ptr(), out["rotation"].data_ptr(),
        out["scale"].data_ptr(), out["transform"].data_ptr(), out["ratio"].data_ptr(), ints["best"].data_ptr(),
        ints["ran"].data_ptr(), kw.get("status", ints["status"].data_ptr()), mask.data_ptr(), ws.data_ptr(),
        kw.get("wsn", need), 0, st)
    assert call(K=0) == -1 and call(total=-1) == -1 and call(max_n=-3) == -1 and call(max_n=n + 1) == -1
    assert call(dtype=5) == -1 and call(src=None) == -2 and call(status=None) == -2
    assert call(wsn=need - 1) == -3 and b"workspace" in L.sdfr_last_error()
    torch.cuda.synchronize()
    assert all(torch.all(t == 7) for t in list(out.values()) + list(ints.values()) + [mask])   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in {**out, **ints}.items()}
    assert h["status"].tolist() == [tw.OK, tw.NONE, tw.NONE, 7] and h["ran"].tolist() == [100, 0, 0, 7]
    assert h["best"][0] == int(c["best_iteration"])
    assert np.max(np.abs(h["transform"][0].reshape(4, 4) - c["transform"])) <= ATOL
    assert np.all(h["position"][3] == 7) and np.all(h["transform"][3] == 7)
    m = mask.cpu().numpy()
    assert np.array_equal(np.nonzero(m[:n])[0], c["inlier_idx"]) and np.all(m[n:] == 7)
    # sample indices beyond the set and below zero are clamped into it: five times the same point, no variance
    draws.copy_(torch.roll(draws, 1, 0))          # object 0 now has -draws (-> point 0), the others have no points
    assert call() == 0
    torch.cuda.synchronize()
    assert ints["status"].tolist() == [tw.POSE_ERROR, tw.NONE, tw.NONE, 7] and ints["ran"].tolist() == [1, 0, 0, 7]
    draws.copy_(torch.roll(draws, 1, 0))          # ... and draws + 10^6 (-> the last point)
    assert call() == 0
    torch.cuda.synchronize()
    assert ints["status"].tolist() == [tw.POSE_ERROR, tw.NONE, tw.NONE, 7]
    assert torch.all(mask[n:] == 7) and torch.all(out["transform"][3] == 7)


def test_an_object_larger_than_max_points_is_reported_not_truncated(dev):
    """device offsets with a max_points that is too small for one object: that object answers STATUS_TRUNCATED with NaN
    results, the others are the bits of their single calls"""
    from sdfest_amd import nocs_utils as nu
    names = ["g0", "c", "g2"]
    sizes = [len(CASES[n]["source"]) for n in names]
    assert sizes[1] == 257 and sizes[0] < sizes[2]
    src = torch.tensor(np.concatenate([CASES[n]["source"] for n in names]), device=dev)
    tgt = torch.tensor(np.concatenate([CASES[n]["target"] for n in names]), device=dev)
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    draws = torch.tensor(np.stack([CASES[n]["draws"] for n in names]), dtype=torch.int32, device=dev)
    r = nu.estimate_similarity_transforms(src, tgt, off, max_points=sizes[0], sample_indices=draws)
    assert r.status.tolist() == [nu.STATUS_OK, nu.STATUS_OK, nu.STATUS_TRUNCATED]
    assert r.iterations_run.tolist() == [100, 100, 0] and r.best_iteration[2] == -1 and r.inlier_ratio[2] == 0
    assert torch.isnan(r.transform[2]).all() and torch.isnan(r.position[2]).all() and torch.isnan(r.scale[2])
    assert torch.isnan(r.rotation_matrix[2]).all()
    for k in (0, 1):
        single = run_batch([names[k]], dev)
        for key in RESULTS:
            assert getattr(r, key)[k].cpu().numpy().tobytes() == single[key][0].tobytes(), (names[k], key)
    with pytest.raises(ValueError, match="max_points"):
        nu.result_from_status(nu.STATUS_TRUNCATED, None, None, None, None)
    # one point more is enough for the second object, not for the third
    r = nu.estimate_similarity_transforms(src, tgt, off, max_points=sizes[2] - 1, sample_indices=draws)
    assert r.status.tolist() == [nu.STATUS_OK, nu.STATUS_OK, nu.STATUS_TRUNCATED]
    r = nu.estimate_similarity_transforms(src, tgt, off, max_points=sizes[2], sample_indices=draws)
    assert r.status.tolist() == [nu.STATUS_OK] * 3


def test_correspondences_never_write_outside_capacity_or_their_own_rows(dev, frame):
    """sdfr_nocs_correspondences with a capacity below the total, with offsets that leave an object fewer rows than
    it has pixels, and with offsets below zero: the rows inside are the twin's, guard values behind `capacity` and in
    the rows no object owns stay"""
    from sdfest_amd import _lib
    L = _lib.lib()
    depth = frame["depth_mm"].astype(np.float32) * np.float32(0.001)
    H, W = depth.shape
    ids = [int(i) for i in frame["meta_mask_id"]][:3]
    twin = [tw.correspondences(depth, frame["mask"], frame["coord"], i) for i in ids]
    n = [len(s) for s, _, _ in twin]
    d_depth, d_mask = torch.tensor(depth, device=dev), torch.tensor(frame["mask"], device=dev)
    d_coord = torch.tensor(np.ascontiguousarray(frame["coord"]), device=dev)
    d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
    ws = torch.empty(L.sdfr_nocs_workspace_bytes(W, H, 3), dtype=torch.uint8, device=dev)
    stats = torch.empty((2, 3), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert L.sdfr_nocs_count(d_depth.data_ptr(), d_mask.data_ptr(), W, H, d_ids.data_ptr(), 3, stats[0].data_ptr(),
                             stats[1].data_ptr(), ws.data_ptr(), ws.numel(), 0, st) == 0
    assert stats[0].tolist() == n
    rows = sum(n) + 64
    cam = tw.REAL_CAMERA

    def compact(offsets, capacity):
        source = torch.full((rows, 3), 7.0, dtype=torch.float32, device=dev)
        target = torch.full((rows, 3), 7.0, dtype=torch.float32, device=dev)
        off = torch.tensor(offsets, dtype=torch.int64, device=dev)
        assert L.sdfr_nocs_correspondences(d_depth.data_ptr(), d_mask.data_ptr(), d_coord.data_ptr(),
                                           frame["coord"].shape[2], W, H, 1.0 / cam["fx"], 1.0 / cam["fy"],
                                           cam["cx"], cam["cy"], d_ids.data_ptr(), 3, off.data_ptr(), capacity,
                                           ws.data_ptr(), source.data_ptr(), target.data_ptr(), 0, st) == 0
        torch.cuda.synchronize()
        return source.cpu().numpy(), target.cpu().numpy()

    def check(got, expected):
        """expected: {first row: twin rows}; every other row keeps the guard value"""
        want = np.full((rows, 3), 7.0, np.float32)
        for at, block in expected.items():
            want[at:at + len(block)] = block
        assert got.tobytes() == want.tobytes()

    # capacity in the middle of object 1: object 0 whole, object 1 up to capacity, object 2 not at all
    cap = n[0] + n[1] // 2
    src, tgt = compact([0, n[0], n[0] + n[1], sum(n)], cap)
    check(src, {0: twin[0][0], n[0]: twin[1][0][:n[1] // 2]})
    check(tgt, {0: twin[0][1], n[0]: twin[1][1][:n[1] // 2]})
    # object 0 is given 10 rows fewer than it has; objects 1 and 2 end before they begin: no rows
    src, tgt = compact([0, n[0] - 10, 0, 0], rows)
    check(src, {0: twin[0][0][:n[0] - 10]})
    check(tgt, {0: twin[0][1][:n[0] - 10]})
    # object 0 starts 5 rows below zero (its first 5 pixels are dropped), object 1 owns 8 rows, object 2 all but 7
    src, tgt = compact([-5, n[0] - 5, n[0] + 3, n[0] + 3 + n[2] - 7], rows)
    check(src, {0: twin[0][0][5:], n[0] - 5: twin[1][0][:8], n[0] + 3: twin[2][0][:n[2] - 7]})
    check(tgt, {0: twin[0][1][5:], n[0] - 5: twin[1][1][:8], n[0] + 3: twin[2][1][:n[2] - 7]})
    src, tgt = compact([0, n[0], n[0] + n[1], sum(n)], 0)   # no capacity: nothing at all
    check(src, {})
    check(tgt, {})


# ---- the dataset -------------------------------------------------------------------------------------------------------
def write_root(root, frame):
    """a NOCS root directory with the fixture frame as real_train/scene_1/0000 (PNG files written with PIL, a one-colour
    colour image, an eight-vertex box OBJ per object with the recorded vertex minima and maxima)"""
    from PIL import Image
    scene = os.path.join(root, "real_train", "scene_1")
    models = os.path.join(root, "obj_models", "real_train")
    os.makedirs(scene)
    os.makedirs(models)
    Image.fromarray(frame["depth_mm"]).save(os.path.join(scene, "0000_depth.png"))
    Image.fromarray(frame["mask"]).save(os.path.join(scene, "0000_mask.png"))
    Image.fromarray(frame["coord"]).save(os.path.join(scene, "0000_coord.png"))
    Image.fromarray(np.full(frame["coord"].shape[:2] + (3,), (10, 200, 90), np.uint8)).save(
        os.path.join(scene, "0000_color.png"))
    with open(os.path.join(scene, "0000_meta.txt"), "w") as f:
        for mid, cat, name in zip(frame["meta_mask_id"], frame["meta_category_id"], frame["meta_name"]):
            f.write(f"{mid} {cat} {name}\n")
    quads = [(1, 2, 4, 3), (5, 7, 8, 6), (1, 5, 6, 2), (3, 4, 8, 7), (1, 3, 7, 5), (2, 6, 8, 4)]
    for name, lo, hi in zip(frame["meta_name"], frame["vertex_min"], frame["vertex_max"]):
        with open(os.path.join(models, f"{name}.obj"), "w") as f:
            for x in (lo[0], hi[0]):
                for y in (lo[1], hi[1]):
                    for z in (lo[2], hi[2]):
                        f.write(f"v {float(x)!r} {float(y)!r} {float(z)!r}\n")
            for a, b, c, d in quads:
                f.write(f"f {a} {b} {c}\nf {a} {c} {d}\n")
    return root


@pytest.fixture(scope="module")
def nocs_root(tmp_path_factory, frame):
    """the root directory, preprocessed once by the first construction"""
    from sdfest_amd import NOCSDataset
    root = write_root(str(tmp_path_factory.mktemp("nocs")), frame)
    ds = NOCSDataset({"root_dir": root, "split": "real_train"})
    return root, ds


def stored(path):
    import pickle
    with open(path, "rb") as f:
        return pickle.load(f)


def test_dataset_preprocesses_the_frame(nocs_root, frame):
    import json
    root, ds = nocs_root
    pre = os.path.join(root, "sdfest_pre", "real_train")
    assert len(ds) == 5 and ds.preprocess_stats["objects"] == 5 and ds.preprocess_stats["skipped"] == 0
    files = sorted(f for f in os.listdir(pre) if f.endswith(".pkl"))
    assert files == [f"00000000_{i}.pkl" for i in range(5)]
    cats = json.load(open(os.path.join(pre, "categories.json")))
    assert sorted(cats) == sorted(ds.category_id_to_str.values())
    assert cats["mug"] == ["00000000_0.pkl"] and cats["bowl"] == ["00000000_1.pkl", "00000000_2.pkl"]
    assert cats["bottle"] == ["00000000_3.pkl"] and cats["can"] == ["00000000_4.pkl"] and cats["laptop"] == []
    depth = frame["depth_mm"].astype(np.float32) * np.float32(0.001)
    for g, name in enumerate(files):
        s = stored(os.path.join(pre, name))
        assert sorted(s) == sorted(["color_path", "depth_path", "mask_path", "mask_id", "category_id", "obj_path",
                                    "nocs_transform", "position", "orientation_q", "extents", "nocs_scale", "max_extent"])
        mid = int(frame["meta_mask_id"][g])
        assert s["mask_id"] == mid and s["category_id"] == int(frame["meta_category_id"][g])
        assert s["color_path"].endswith("0000_color.png") and s["depth_path"].endswith("0000_depth.png")
        assert s["obj_path"] == os.path.join(root, "obj_models", "real_train", f"{frame['meta_name'][g]}.obj")
        for key, shape in (("position", (3,)), ("orientation_q", (4,)), ("extents", (3,)), ("nocs_transform", (4, 4)),
                           ("nocs_scale", ()), ("max_extent", ())):
            assert isinstance(s[key], torch.Tensor) and s[key].dtype == torch.float32 and tuple(s[key].shape) == shape
            assert s[key].device.type == "cpu"
        # the whole annotation again in numpy: the twin's correspondences, the twin's statement of the sample stream,
        # the twin's RANSAC; fp64 results that agree to 1e-10 are stored as fp32: one fp32 ulp of values up to 2
        src, tgt, _ = tw.correspondences(depth, frame["mask"], frame["coord"], mid)
        o = tw.ransac(src, tgt, tw.sample_indices(len(src), tw.object_seed(0, 0, mid)))
        assert o["status"] == tw.OK
        ulp = 2.4e-7
        assert np.max(np.abs(s["position"].numpy() - o["position"])) <= ulp
        assert np.max(np.abs(s["nocs_transform"].numpy() - o["transform"])) <= ulp
        q = tw.matrix_to_quat(o["rotation"])
        assert np.max(np.abs(s["orientation_q"].numpy() - q)) <= ulp
        extents = (frame["vertex_max"][g].astype(np.float32) - frame["vertex_min"][g].astype(np.float32))
        assert np.max(np.abs(s["extents"].numpy() - extents)) <= ulp
        assert s["nocs_scale"] == torch.linalg.norm(s["extents"]) and s["max_extent"] == s["extents"].max()
        # (and the estimate is the reference's own up to the difference between two inlier fits of the same object)
        c = CASES[f"g{g}"]
        assert np.max(np.abs(o["position"] - c["position"])) < 5e-3 and abs(o["scale"] / c["scale"] - 1) < 2e-2


OPTIONS = [dict(), dict(camera_convention="opencv"), dict(mask_pointcloud=True),
           dict(mask_pointcloud=True, camera_convention="opencv"), dict(normalize_pointcloud=True, mask_pointcloud=True),
           dict(normalize_pointcloud=True), dict(scale_convention="diagonal"), dict(scale_convention="max"),
           dict(scale_convention="half_max"), dict(scale_convention="full"),
           dict(remap_y_axis="y", remap_x_axis="-z", scale_convention="full"), dict(category_str="mug"),
           dict(orientation_repr="discretized", orientation_grid_resolution=1)]


def recover_centroid(raw, normalised):
    """the fp32 vector c with raw - c == normalised for EVERY point (fp32 subtraction, bit for bit), looked for among
    the fp32 neighbours of raw - normalised at the point closest to c (where the subtraction was exact or nearly so);
    None if there is none"""
    c = np.zeros(3, np.float32)
    for axis in range(3):
        i = int(np.argmin(np.abs(normalised[:, axis])))
        guess = np.float32(np.float64(raw[i, axis]) - np.float64(normalised[i, axis]))
        lo = hi = guess
        candidates = [guess]
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            candidates += [lo, hi]
        hits = [v for v in candidates if (raw[:, axis] - v).tobytes() == normalised[:, axis].tobytes()]
        if not hits:
            return None
        c[axis] = hits[0]
    return c


@pytest.mark.parametrize("options", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_samples_equal_the_twin(options, nocs_root, frame):
    """a second construction reads what the first one wrote; every sample equals the twin's"""
    from sdfest_amd import NOCSDataset, SO3Grid
    root, first = nocs_root
    pre = os.path.join(root, "sdfest_pre", "real_train")
    before = {f: os.stat(os.path.join(pre, f)).st_mtime_ns for f in os.listdir(pre)}
    ds = NOCSDataset({"root_dir": root, "split": "real_train", **options})
    assert ds.preprocess_stats is None
    assert before == {f: os.stat(os.path.join(pre, f)).st_mtime_ns for f in os.listdir(pre)}
    assert len(ds) == (1 if options.get("category_str") else 5)
    depth = frame["depth_mm"].astype(np.float32) * np.float32(0.001)
    grid = SO3Grid(1) if options.get("orientation_repr") == "discretized" else None
    kw = {k: v for k, v in options.items() if k not in ("category_str", "orientation_repr", "orientation_grid_resolution")}
    for i in ([0] if options.get("category_str") else [0, 3]):      # the mug and the bottle
        s = ds[i]
        data = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in stored(ds._sample_files[i]).items()}
        t = tw.sample(data, depth, frame["mask"], grid=grid, **kw)
        assert s["category_str"] == ds.category_id_to_str[data["category_id"]] and s["obj_path"] == data["obj_path"]
        assert s["pointset"].is_cuda and s["depth"].is_cuda and s["color"].shape == (480, 640, 3)
        assert np.array_equal(s["depth"].cpu().numpy(), depth) and np.array_equal(s["mask"].cpu().numpy(), t["mask"])
        assert np.array_equal(s["color"][0, 0].cpu().numpy(), np.float32([10, 200, 90]) / 255)
        pts = s["pointset"].cpu().numpy()
        assert pts.shape == t["pointset"].shape and pts.dtype == np.float32
        if options.get("normalize_pointcloud"):
            # Only the centroid may differ from the twin's, which is the fp64 mean (an fp32 twin would sum in another
            # order than the device and differ from it by BOTH sums' errors, so it could pin no more).  Everything
            # else is exact: there is ONE fp32 vector c with points == raw - c for every point and position ==
            # stored position - c, in fp32 arithmetic.  c is an fp32 sum over up to 3e5 terms and a division: with at
            # most 32 roundings between a term and the result (per-lane partial sums, a tree of depth <= 19, the
            # division), each 2^-24 relative to a partial sum of |x|, it is within 32 * 2^-24 * mean|x| of the mean
            plain = tw.sample(data, depth, frame["mask"], grid=grid, **{**kw, "normalize_pointcloud": False})
            c = recover_centroid(plain["pointset"], pts)
            assert c is not None
            assert s["position"].cpu().numpy().tobytes() == (plain["position"] - c).tobytes()
            raw = plain["pointset"].astype(np.float64)
            err, tol = np.abs(c - raw.mean(0)), 32 * 2.0 ** -24 * np.abs(raw).mean(0)
            print(f"centroid error {err}, bound {tol}")
            assert np.all(err <= tol)
        else:
            assert pts.tobytes() == t["pointset"].tobytes()
            assert np.array_equal(s["position"].cpu().numpy(), t["position"])
        q = s["quaternion"].cpu().numpy()
        assert q.dtype == t["quaternion"].dtype and np.array_equal(q, t["quaternion"])
        assert np.array_equal(s["scale"].cpu().numpy(), t["scale"])
        if grid is None:
            assert np.array_equal(s["orientation"].cpu().numpy(), t["quaternion"])
        else:
            assert s["orientation"].dtype == torch.long and int(s["orientation"]) == int(t["orientation"])


def test_validation_batches_run_through_the_trainer(nocs_root):
    import init_train_twin as it
    from sdfest_amd import NOCSDataset, SDFPoseNetTrainer
    from sdfest_amd.init_train import validation_keys
    root, _ = nocs_root
    ds = NOCSDataset({"root_dir": root, "split": "real_train", "mask_pointcloud": True, "normalize_pointcloud": True})
    batches = ds.validation_batches(2, max_points=500, seed=3)
    assert [b[0].shape[0] for b in batches] == [2, 2, 1]
    for points, targets in batches:
        assert points.is_cuda and points.shape[1:] == (500, 3) and sorted(targets) == ["orientation", "position",
                                                                                          "quaternion", "scale"]
    again = ds.validation_batches(2, max_points=500, seed=3)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(batches, again))
    trainer = SDFPoseNetTrainer(it.train_config(it.Q16), seed=4)
    got = trainer.validate(batches, "real")
    assert list(got) == validation_keys("real", False)
    assert all(np.isfinite(v) for v in got.values())
