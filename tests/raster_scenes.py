"""The scenes of tests/test_mesh_depth_gpu.py (test side only): name -> mesh, camera, pose, convention, near.

Every scene was checked with the float64 twin alone (tests/raster_twin.py::bracket), before any GPU run, against the
two caps that keep the bracket from hiding a failure: at most 1 % of its pixels `mixed`, at least 5 % of its hit pixels
`flat` -- and, for the scenes whose face indices are compared, at least a third of the hit pixels with a well-defined
face.  `flat` asks for hi - lo <= 1e-4 depth over rays 1/16 pixel apart, i.e. a surface slope below 1.6e-3 f (f in
pixels): the focal lengths are long (600 at 160 x 120) so that a third of a sphere's pixels qualify."""
import numpy as np

import raster_twin as rt


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return tuple((q / np.linalg.norm(q)).astype(np.float32).astype(np.float64))


def random_quat(rng):
    return unit(rng.normal(size=4))


def make_camera(W, H, fx, fy, cx=None, cy=None):
    from sdfest_amd import Camera
    return Camera(W, H, fx, fy, W / 2 if cx is None else cx, H / 2 if cy is None else cy, pixel_center=0.5)


def scenes(mc):
    """mc(name) -> (vertices float32 (V,3), faces int32 (F,3)) of the marching-cubes mesh of "sphere" / "blobs"
    (level 0, normalised frame).  Returns a list of dictionaries: name, mesh, camera, pose = (factor, quat, position)
    in float32-representable numbers, convention, near, kind ("a" .. "f": the issue's list), faces (compare face
    indices), flat (hold the scene to the 5 % flat cap)."""
    rng = np.random.default_rng(5)
    f32 = lambda *x: tuple(float(np.float32(v)) for v in x)
    cube = rt.cube(1.0)
    out = []

    def add(name, kind, mesh, cam, factor, quat, pos, convention="opengl", near=0.0, faces=False, flat=True):
        out.append({"name": name, "kind": kind, "mesh": mesh, "camera": cam,
                    "pose": (float(np.float32(factor)), quat, f32(*pos)), "convention": convention,
                    "near": float(np.float32(near)), "faces": faces, "flat": flat})

    add("a_sphere_160", "a", mc("sphere"), make_camera(160, 120, 600.0, 600.0), 0.08, random_quat(rng),
        (0.012, -0.008, -0.5), faces=True)
    add("a_blobs_160_open3d", "a", mc("blobs"), make_camera(160, 120, 600.0, 600.0), 0.055, random_quat(rng),
        (-0.006, 0.004, 0.52), convention="open3d", faces=True)
    add("a_blobs_640", "a", mc("blobs"), make_camera(640, 480, 1500.0, 1500.0), 0.09, random_quat(rng),
        (0.01, 0.006, -0.6), faces=True)
    add("b_cube_fills_image", "b", cube, make_camera(160, 120, 300.0, 300.0), 0.3, unit([0.03, -0.04, 0.02, 1.0]),
        (0.01, -0.02, -0.62), faces=True)
    add("b_camera_inside_cube", "b", cube, make_camera(160, 120, 300.0, 300.0), 1.0, unit([0.05, 0.03, -0.02, 1.0]),
        (0.05, -0.03, 0.1), faces=True, flat=False)
    # a long thin plate, turned 40 degrees about y: one end behind the camera, both ends off the screen
    plate = (cube[0] * np.array([1.0, 0.03, 0.02], dtype=np.float32), cube[1])
    turned = unit([0.0, np.sin(np.radians(20.0)), 0.0, np.cos(np.radians(20.0))])
    add("c_partly_behind_offscreen", "c", plate, make_camera(160, 120, 600.0, 600.0), 1.0, turned,
        (0.0, 0.005, -0.5), faces=True)
    add("c_wholly_behind", "c", plate, make_camera(160, 120, 600.0, 600.0), 1.0, turned, (0.0, 0.005, 1.5),
        faces=True, flat=False)
    add("d_fine_sphere_204k", "d", rt.uv_sphere(320, 320, 1.0), make_camera(160, 120, 600.0, 600.0), 0.04,
        random_quat(rng), (0.004, 0.003, -0.5))
    add("e_ragged_offcentre", "e", rt.uv_sphere(24, 32, 1.0), make_camera(33, 25, 420.0, 360.0, 13.3, 14.6), 0.012,
        random_quat(rng), (0.002, -0.001, 0.5), convention="open3d")
    add("f_near_cuts_the_sphere", "f", mc("sphere"), make_camera(160, 120, 600.0, 600.0), 0.08, random_quat(rng),
        (0.0, 0.0, -0.5), near=0.49)
    return out
