"""numpy twin of the pose half of the reference's ``AnnotatedRedwoodDataset.__getitem__``
(initialization/datasets/redwood_dataset.py:225-238 and :284-365), restated in float64 from reading it, for use where
the reference cannot be imported (its package pulls in open3d and yoco).

It is written independently of sdfest_amd on purpose: the remapping matrix is built the way the reference builds it
(two columns set from the names, the third from the row sums and the determinant), the quaternion of a matrix comes
from an eigenvector (not Shepperd's branches), and the camera conventions are applied as matrices.
"""
import numpy as np

AXES = ("x", "y", "z", "-x", "-y", "-z")


def quaternion_multiply(a, b):
    """Hamilton product of scalar-last quaternions: the rotation b, then a"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def quaternion_to_matrix(q):
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrix_to_quaternion(m):
    """scalar-last unit quaternion of a rotation matrix: the eigenvector of the largest eigenvalue of the symmetric
    4 x 4 matrix of Bar-Itzhack's method (the sign is arbitrary)"""
    m = np.asarray(m, dtype=np.float64)
    k = np.array([[m[0, 0] - m[1, 1] - m[2, 2], m[1, 0] + m[0, 1], m[2, 0] + m[0, 2], m[2, 1] - m[1, 2]],
                  [m[1, 0] + m[0, 1], m[1, 1] - m[0, 0] - m[2, 2], m[2, 1] + m[1, 2], m[0, 2] - m[2, 0]],
                  [m[2, 0] + m[0, 2], m[2, 1] + m[1, 2], m[2, 2] - m[0, 0] - m[1, 1], m[1, 0] - m[0, 1]],
                  [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], m[0, 0] + m[1, 1] + m[2, 2]]]) / 3.0
    values, vectors = np.linalg.eigh(k)
    return vectors[:, np.argmax(values)]


def o2n_matrix(remap_x_axis, remap_y_axis):
    """:327-365 -- the rotation from the original to the new object axes; ValueError where the reference raises"""
    m = np.zeros((3, 3))
    for name, column, key in ((remap_y_axis, 1, "remap_y_axis"), (remap_x_axis, 0, "remap_x_axis")):
        if name not in AXES:
            raise ValueError(f"Unsupported {key} {name}")
        m["xyz".index(name[-1]), column] = -1.0 if name.startswith("-") else 1.0
    m[:, 2] = 1 - np.abs(np.sum(m, 1))      # rows must sum to +-1
    m[:, 2] *= np.linalg.det(m)             # make special orthogonal
    if np.linalg.det(m) != 1.0:
        raise ValueError("Unsupported combination of remap_{y,x}_axis. det != 1")
    return m


def annotation(position, orientation_q, half_extents, scale_convention="half_max", camera_convention="opengl",
               remap_x_axis=None, remap_y_axis=None):
    """position (3,), orientation_q (4,) scalar-last and "scale" (3,) of annotations.json (an OpenCV pose and half the
    box's sides) -> {"position", "quaternion", "extents", "scale"} as the reference's sample has them, float64"""
    position = np.asarray(position, dtype=np.float64)
    q = np.asarray(orientation_q, dtype=np.float64)
    extents = 2.0 * np.asarray(half_extents, dtype=np.float64)                        # :175
    if camera_convention == "opengl":                                                  # :226-228
        position = np.diag([1.0, -1.0, -1.0]) @ position
    elif camera_convention != "opencv":
        raise ValueError(camera_convention)
    if remap_x_axis is None and remap_y_axis is None:                                  # :307-325
        pass
    elif remap_x_axis is None or remap_y_axis is None:
        raise ValueError("Either both or none of remap_{y,x}_axis have to be None.")
    else:
        o2n = o2n_matrix(remap_x_axis, remap_y_axis)
        extents = np.abs(o2n @ extents)
        q = quaternion_multiply(q, matrix_to_quaternion(o2n.T))      # new -> original -> camera
    if camera_convention == "opengl":                                                  # :234-236: a half turn about x
        q = matrix_to_quaternion(np.diag([1.0, -1.0, -1.0]) @ quaternion_to_matrix(q))
    if scale_convention == "diagonal":                                                 # :284-297
        scale = np.linalg.norm(extents)
    elif scale_convention == "max":
        scale = extents.max()
    elif scale_convention == "half_max":
        scale = 0.5 * extents.max()
    elif scale_convention == "full":
        scale = extents
    else:
        raise ValueError(f"Specified scale convention {scale_convention} not supported.")
    return {"position": position, "quaternion": q / np.linalg.norm(q), "extents": extents, "scale": scale}
