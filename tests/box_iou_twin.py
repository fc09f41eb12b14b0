"""numpy float64 twin of sdfr_box_iou (csrc/boxes.hip): the intersection volume of two oriented boxes and the maximum
over turns of the second box about one of its own axes.  Written for reading, in 3-D: every face rectangle of one box
is clipped against the six half-spaces of the other, and V = (1/3) sum_f d_f area(f) with the origin at box a's centre.

A box is (centre (3,), quaternion (4,) scalar-last, full side lengths (3,))."""
import numpy as np

SNAP = 1e-12   # x L: a vertex this close to a plane is on it


def rotation(q):
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def length_scale(c1, e1, c2, e2):
    """L of the tolerances: |e_a| + |e_b| + |c_b - c_a|"""
    return np.linalg.norm(e1) + np.linalg.norm(e2) + np.linalg.norm(np.asarray(c2, float) - np.asarray(c1, float))


def planes(c, Rm, e):
    """outward normals (6,3) and offsets (6,): n.x <= d, in the order +x, -x, +y, -y, +z, -z of the box's axes"""
    N, D = [], []
    for k in range(3):
        for s in (1.0, -1.0):
            n = s * Rm[:, k]
            N.append(n)
            D.append(n @ c + e[k] / 2)
    return np.array(N), np.array(D)


def clip(poly, n, d, tol, strict):
    s = poly @ n - d
    s[np.abs(s) <= tol] = 0.0
    if strict and np.all(s == 0):
        return poly[:0]
    out = []
    m = len(poly)
    for i in range(m):
        a, b = poly[i], poly[(i + 1) % m]
        sa, sb = s[i], s[(i + 1) % m]
        if sa <= 0:
            out.append(a)
        if (sa < 0 and sb > 0) or (sa > 0 and sb < 0):
            t = sa / (sa - sb)
            out.append(a + t * (b - a))
    return np.array(out).reshape(-1, 3)


def area(poly, n):
    if len(poly) < 3:
        return 0.0
    acc = np.zeros(3)
    for i in range(1, len(poly) - 1):
        acc += np.cross(poly[i] - poly[0], poly[i + 1] - poly[0])
    return 0.5 * (acc @ n)


def face_rect(c, Rm, e, k, s):
    a, b = (k + 1) % 3, (k + 2) % 3
    ctr = c + s * Rm[:, k] * e[k] / 2
    u, v = Rm[:, a] * e[a] / 2, Rm[:, b] * e[b] / 2
    if s < 0:
        u, v = v, u
    return np.array([ctr - u - v, ctr + u - v, ctr + u + v, ctr - u + v])


def intersection_volume(c1, R1, e1, c2, R2, e2):
    """volume of the intersection of the boxes (centre, rotation matrix, side lengths)"""
    c1, c2, e1, e2 = (np.asarray(v, dtype=np.float64) for v in (c1, c2, e1, e2))
    tol = SNAP * length_scale(c1, e1, c2, e2)
    c2 = c2 - c1
    c1 = np.zeros(3)
    N1, D1 = planes(c1, R1, e1)
    N2, D2 = planes(c2, R2, e2)
    V = 0.0
    for c, Rm, e, N, D, No, Do, own in ((c1, R1, e1, N1, D1, N2, D2, 0), (c2, R2, e2, N2, D2, N1, D1, 1)):
        f = 0
        for k in range(3):
            for s in (1.0, -1.0):
                p = face_rect(c, Rm, e, k, s)
                n, d = N[f], D[f]
                f += 1
                for j in range(6):
                    # b's rectangle lying ON a plane of a with the same outward normal: a's rectangle counted it
                    p = clip(p, No[j], Do[j], tol, own == 1 and (No[j] @ n) > 0)
                    if len(p) < 3:
                        break
                V += d * area(p, n) / 3
    return min(max(V, 0.0), min(np.prod(e1), np.prod(e2)))


def box_intersection(a, b, symmetry_axis=None, symmetry_steps=1):
    """(V, IoU) of the boxes a, b = (centre, quaternion, side lengths); with `symmetry_axis` the largest over b turned
    about its own axis by 2 pi s / symmetry_steps"""
    (c1, q1, e1), (c2, q2, e2) = a, b
    R1, R2 = rotation(q1), rotation(q2)
    best = 0.0
    for s in range(symmetry_steps if symmetry_axis is not None else 1):
        Rs = R2
        if s:
            k, ang = int(symmetry_axis), 2 * np.pi * s / symmetry_steps
            i, j = (k + 1) % 3, (k + 2) % 3
            T = np.eye(3)
            T[i, i] = T[j, j] = np.cos(ang)
            T[j, i], T[i, j] = np.sin(ang), -np.sin(ang)
            Rs = R2 @ T
        best = max(best, intersection_volume(c1, R1, e1, c2, Rs, e2))
    va, vb = float(np.prod(np.asarray(e1, float))), float(np.prod(np.asarray(e2, float)))
    return best, best / (va + vb - best)


def tight_box(vertices, position, quaternion):
    """the oriented box (centre, quaternion, side lengths) of object-frame `vertices` (V,3) posed by (position,
    quaternion): what Mesh.oriented_box returns"""
    v = np.asarray(vertices, dtype=np.float64)
    lo, hi = v.min(0), v.max(0)
    return (np.asarray(position, np.float64) + rotation(quaternion) @ ((lo + hi) / 2),
            np.asarray(quaternion, np.float64), hi - lo)


# ---- closed forms: (name, box a, box b, "iou" | "volume", expected) -- the degenerate positions Qhull is no judge of
def _quat_z(degrees):
    half = np.deg2rad(degrees) / 2
    return np.array([0.0, 0.0, np.sin(half), np.cos(half)])


_I = np.array([0.0, 0.0, 0.0, 1.0])
_O = np.zeros(3)
_UNIT = np.ones(3)
GENERIC_Q = np.array([0.3, -0.5, 0.2, 0.7])
QUAT_Z90_FP32 = _quat_z(90.0).astype(np.float32).astype(np.float64)   # sin, cos of 45 degrees rounded to float32
CLOSED_FORMS = [
    ("identical at a generic pose", (np.array([0.1, 0.2, 0.3]), GENERIC_Q, np.array([0.2, 0.3, 0.4])),
     (np.array([0.1, 0.2, 0.3]), GENERIC_Q, np.array([0.2, 0.3, 0.4])), "iou", 1.0),
    ("unit cubes half a side apart", (_O, _I, _UNIT), (np.array([0.5, 0.0, 0.0]), _I, _UNIT), "iou", 1.0 / 3.0),
    ("unit cubes a whole side apart", (_O, _I, _UNIT), (np.array([1.0, 0.0, 0.0]), _I, _UNIT), "iou", 0.0),
    ("a 0.3-cube inside a unit cube", (_O, _I, _UNIT), (np.array([0.1, 0.0, 0.0]), GENERIC_Q, 0.3 * _UNIT), "volume",
     0.027),
    ("(1,2,3) against (2,1,3) turned 90 degrees, fp32 quaternion", (_O, _I, np.array([1.0, 2.0, 3.0])),
     (_O, QUAT_Z90_FP32, np.array([2.0, 1.0, 3.0])), "volume", 6.0),
    ("unit cubes turned 45 degrees", (_O, _I, _UNIT), (_O, _quat_z(45.0), _UNIT), "volume", 2.0 * (np.sqrt(2.0) - 1.0)),
    ("a 0.5-cube sharing a face plane inside a unit cube", (_O, _I, _UNIT), (np.array([0.25, 0.0, 0.0]), _I, 0.5 * _UNIT),
     "volume", 0.125),
    # parallel faces 1e-9 and 1e-8 apart, not coplanar: b's +x face that far inside a's; V = 0.5 x 0.35 x 0.5
    ("a 0.5-cube with a face 1e-9 inside a unit cube's", (_O, _I, _UNIT), (np.array([0.25 - 1e-9, 0.4, 0.0]), _I, 0.5 * _UNIT),
     "volume", 0.0875),
    ("a 0.5-cube with a face 1e-8 inside a unit cube's", (_O, _I, _UNIT), (np.array([0.25 - 1e-8, 0.4, 0.0]), _I, 0.5 * _UNIT),
     "volume", 0.0875),
]
FAR_APART = ((_O, _I, _UNIT), (np.array([3.0, 0.0, 0.0]), GENERIC_Q, _UNIT))   # exactly 0
CUBES_45 = ((_O, _I, _UNIT), (_O, _quat_z(45.0), _UNIT))


def closed_form_bound(a, b, kind, expected):
    """the yardstick 1e-12 L^3 for a volume; for an IoU that bound over the expected union (V_a + V_b) / (1 + IoU),
    times 2 (the volume is in the numerator and in the denominator)"""
    L = length_scale(a[0], a[2], b[0], b[2])
    if kind == "volume":
        return 1e-12 * L ** 3
    return 2 * 1e-12 * L ** 3 * (1.0 + expected) / (np.prod(a[2]) + np.prod(b[2]))


def rows(boxes):
    """(K,10) float64 rows of K boxes (centre, quaternion, side lengths)"""
    return np.array([np.concatenate([np.asarray(p, np.float64) for p in box]) for box in boxes])
