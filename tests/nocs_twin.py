"""numpy twin of the NOCS annotation: the similarity RANSAC of the reference's ``nocs_utils`` and the front half of
``NOCSDataset._estimate_object``, restated from their behaviour for use where the reference cannot be imported (its
package pulls in open3d and yoco) and on machines that do not have it.

The RANSAC half is pinned to the reference itself by tests/golden/nocs_ransac.npz (tools/make_nocs_goldens.py records
the reference's draws and results; tests/test_nocs_cpu.py replays them through this file).  The correspondence half is
pinned by nothing but this file: it is the statement the GPU kernel is compared with.
"""
import numpy as np

N_ITER = 100
OK, NONE, POSE_ERROR, NAN_INPUT = 0, 1, 2, 3


class PoseEstimationError(Exception):
    pass


def thresholds(source, target):
    """(pass_t, stop_t): numpy's own dtype rules apply -- an fp32 input's norms and their mean are fp32."""
    tn = np.mean(np.linalg.norm(target, axis=1))
    sn = np.mean(np.linalg.norm(source, axis=1))
    pass_t = max(sn / tn, tn / sn) * 0.01
    return pass_t, pass_t / 100


def umeyama(src, tgt):
    """(scale, rotation (3,3), translation (3,), transform (4,4)) of the least-squares similarity src -> tgt; src, tgt
    (M,3) float64.  NaN in the covariance: RuntimeError; zero source variance: PoseEstimationError."""
    cs, ct = src.mean(axis=0), tgt.mean(axis=0)
    cov = (tgt - ct).T @ (src - cs) / len(src)
    if np.isnan(cov).any():
        raise RuntimeError("There are NANs in the input.")
    u, d, vh = np.linalg.svd(cov)
    s = np.eye(3)
    if np.linalg.det(cov) < 0.0:
        s[2, 2] = -1
    rot = u @ s @ vh
    var = np.var(src, axis=0).sum()
    if var == 0:
        raise PoseEstimationError()
    scale = 1 / var * np.trace(s @ np.diag(d))
    sr = np.diag([scale] * 3) @ rot
    t = ct - sr @ cs
    T = np.identity(4)
    T[:3, :3] = sr
    T[:3, 3] = t
    return scale, rot, t, T


def point_residuals(T, src, tgt):
    return np.linalg.norm(tgt.T - (T[:3, :3] @ src.T + T[:3, 3:4]), axis=0)


def ransac(source, target, draws):
    """The whole estimate with the draws given, (100, 5) ints.  Returns a dict: status, position, rotation, scale,
    transform (None unless status is OK), best_iteration (-1 without a winner), iterations_run, inlier_idx,
    inlier_ratio, residuals (of the iterations that ran), pass_t, stop_t."""
    out = dict(status=NONE, position=None, rotation=None, scale=None, transform=None, best_iteration=-1,
               iterations_run=0, inlier_idx=np.arange(len(source)), inlier_ratio=0.0, residuals=[], pass_t=None,
               stop_t=None)
    n = len(source)
    if n < 5 or len(target) < 5:
        return out
    src, tgt = np.asarray(source, np.float64), np.asarray(target, np.float64)
    pass_t, stop_t = thresholds(source, target)
    out["pass_t"], out["stop_t"] = float(pass_t), float(stop_t)
    best = 1e10
    for i in range(N_ITER):
        out["iterations_run"] = i + 1
        idx = np.asarray(draws[i])
        try:
            T = umeyama(src[idx], tgt[idx])[3]
        except PoseEstimationError:
            out["status"] = POSE_ERROR
            return out
        except RuntimeError:
            out["status"] = NAN_INPUT
            return out
        r = point_residuals(T, src, tgt)
        res = np.linalg.norm(r)
        out["residuals"].append(res)
        if res < best:
            best = res
            inl = np.nonzero(r < pass_t)[0]
            out["best_iteration"], out["inlier_idx"] = i, inl
            out["inlier_ratio"] = np.count_nonzero(inl) / n     # the reference counts non-zero INDICES
        if best < stop_t:
            break
    if out["inlier_ratio"] < 0.1:
        return out
    inl = out["inlier_idx"]
    try:
        scale, rot, t, T = umeyama(src[inl], tgt[inl])
    except PoseEstimationError:
        out["status"] = POSE_ERROR
        return out
    except RuntimeError:
        out["status"] = NAN_INPUT
        return out
    out.update(status=OK, position=t, rotation=rot, scale=scale, transform=T)
    return out


def estimate_similarity_transform(source, target, draws):
    """the reference's return convention: four results, four None, or PoseEstimationError / RuntimeError"""
    o = ransac(source, target, draws)
    if o["status"] == POSE_ERROR:
        raise PoseEstimationError()
    if o["status"] == NAN_INPUT:
        raise RuntimeError("There are NANs in the input.")
    return o["position"], o["rotation"], o["scale"], o["transform"]


# ---- the frame half --------------------------------------------------------------------------------------------------
REAL_CAMERA = dict(width=640, height=480, fx=591.0125, fy=590.16775, cx=322.525, cy=244.11084, pixel_center=0.0)
CAMERA_CAMERA = dict(width=640, height=480, fx=577.5, fy=577.5, cx=319.5, cy=239.5, pixel_center=0.0)


def correspondences(depth, mask, coord, mask_id, cam=REAL_CAMERA):
    """(source, target, max valid depth) of one object, both (N,3) float32, the valid pixels in row-major order.
    depth (H,W) float32 metres, mask (H,W) uint8, coord (H,W,3|4) uint8.  Every operation rounds to fp32 on its own;
    a division by a focal length is the product with its fp32 reciprocal (this project's depth_to_pointcloud)."""
    f32 = np.float32
    valid = (mask == mask_id).astype(f32) * depth != 0
    rows, cols = np.nonzero(valid)
    c = coord[rows, cols][:, :3].astype(f32) / f32(255)
    c[:, 2] = f32(1) - c[:, 2]
    source = c - f32(0.5)
    z = depth[rows, cols]
    rfx, rfy = f32(1.0 / cam["fx"]), f32(1.0 / cam["fy"])
    cx0, cy0 = f32(cam["cx"] - cam["pixel_center"]), f32(cam["cy"] - cam["pixel_center"])
    x = ((cols.astype(f32) - cx0) * z) * rfx
    y = ((rows.astype(f32) - cy0) * z) * rfy
    target = np.stack([x, y, z], axis=1).astype(f32)
    return source, target, (float(z.max()) if len(z) else 0.0)


# ---- the sample stream (include/sdfr.h, sdfr_nocs_sample_indices) -----------------------------------------------------
NOCS_STREAM = 0x4E4F4353


def sample_indices(n, seed):
    """(100, 5) distinct indices in [0, n): Philox counter {iteration, draw, attempt, NOCS_STREAM}, key = seed;
    index = floor(word0 * n / 2^32); a repeated index is drawn again with the next attempt"""
    from metrics_twin import philox4x32_10
    out = np.zeros((N_ITER, 5), np.int64)
    if n < 5:
        return out
    key = (np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    attempts = 64
    ctr = np.zeros((N_ITER, 5, attempts, 4), np.uint32)
    ctr[..., 0] = np.arange(N_ITER, dtype=np.uint32)[:, None, None]
    ctr[..., 1] = np.arange(5, dtype=np.uint32)[None, :, None]
    ctr[..., 2] = np.arange(attempts, dtype=np.uint32)[None, None, :]
    ctr[..., 3] = NOCS_STREAM
    idx = (philox4x32_10(ctr, key)[..., 0].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)
    for i in range(N_ITER):
        for d in range(5):
            free = [int(v) for v in idx[i, d] if int(v) not in out[i, :d]]
            out[i, d] = free[0] if free else min(set(range(5)) - set(out[i, :d].tolist()))
    return out


def object_seed(seed, image_id, mask_id):
    """NOCSDataset's key of an object's stream"""
    return ((seed * 1000003 + image_id) * 256 + mask_id) % (2 ** 63)


# ---- a sample from the stored annotation (the reference's _sample_from_sample_data) -----------------------------------
def quat_mul(a, b):
    """scalar-last Hamilton product in the operands' dtype, terms summed left to right"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def matrix_to_quat(m):
    """scalar-last, Shepperd's branches, float64"""
    m = np.asarray(m, np.float64)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    d = [m[0, 0], m[1, 1], m[2, 2], t]
    c = int(np.argmax(d))
    q = np.zeros(4)
    if c == 3:
        q[:] = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + t]
    else:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i], q[j], q[k], q[3] = 1 - t + 2 * m[i, i], m[j, i] + m[i, j], m[k, i] + m[i, k], m[k, j] - m[j, k]
    return q / np.linalg.norm(q)


def remap_matrix(remap_y, remap_x):
    axis = {"x": 0, "y": 1, "z": 2}
    r = np.zeros((3, 3))
    r[axis[remap_y[-1]], 1] = -1 if remap_y[0] == "-" else 1
    r[axis[remap_x[-1]], 0] = -1 if remap_x[0] == "-" else 1
    r[:, 2] = 1 - np.abs(r.sum(1))
    r[:, 2] *= np.linalg.det(r)
    assert np.linalg.det(r) == 1.0
    return r


def pointcloud(depth, mask, cam, convention):
    """back-projection of the pixels with depth * mask != 0 (mask None: all), row-major, fp32 step by step"""
    f32 = np.float32
    d = depth if mask is None else depth * mask.astype(f32)
    rows, cols = np.nonzero(d)
    z = d[rows, cols]
    rfx, rfy = f32(1.0 / cam["fx"]), f32(1.0 / cam["fy"])
    cx0, cy0 = f32(cam["cx"] - cam["pixel_center"]), f32(cam["cy"] - cam["pixel_center"])
    x = ((cols.astype(f32) - cx0) * z) * rfx
    y = (-(rows.astype(f32) - cy0) * z) * rfy
    p = np.stack([x, y, -z], axis=1).astype(f32)
    return p * f32([1, -1, -1]) if convention == "opencv" else p


def sample(data, depth, mask, cam=REAL_CAMERA, mask_pointcloud=False, normalize_pointcloud=False,
           camera_convention="opengl", scale_convention="half_max", remap_y_axis=None, remap_x_axis=None, grid=None):
    """data: the stored annotation as numpy float32 arrays (position, orientation_q, extents, nocs_scale, max_extent)
    and mask_id.  Returns pointset, position, quaternion, orientation, scale (float32; the centroid of a normalised
    point set is taken in float64 and rounded once)."""
    f32 = np.float32
    inst = mask == data["mask_id"]
    pts = pointcloud(depth, inst if mask_pointcloud else None, cam, camera_convention)
    flip = camera_convention != "opencv"
    position = data["position"] * f32([1, -1, -1]) if flip else data["position"]
    q, extents = data["orientation_q"], data["extents"]
    if remap_y_axis is not None:
        r = remap_matrix(remap_y_axis, remap_x_axis)
        extents = np.abs(r.astype(f32) @ extents)
        q = quat_mul(q.astype(np.float64), matrix_to_quat(r.T))      # (float32 x float64 promotes, in torch as here)
    if flip:
        q = quat_mul(np.asarray([1, 0, 0, 0], q.dtype), q)
    scale = {"diagonal": data["nocs_scale"], "max": data["max_extent"], "half_max": f32(0.5) * data["max_extent"],
             "full": extents}[scale_convention]
    if normalize_pointcloud:
        centroid = pts.astype(np.float64).mean(0)
        pts = (pts - centroid).astype(f32)
        position = (position - centroid).astype(f32)
    orientation = q if grid is None else grid.quat_to_index(q)
    return dict(pointset=pts, mask=inst, position=position, quaternion=q, orientation=orientation, scale=scale)
