"""Meshes of decoded SDFs: marching cubes on the GPU (``sdfr_mesh_count`` / ``sdfr_mesh_emit``, csrc/mesh.hip).

``extract_mesh`` replaces what ``SDFPipeline.generate_mesh`` does with skimage (simple_setup.py:637-660) for one grid
or a batch of them, and ``Mesh`` carries the result the way the reference's ``synthetic.Mesh`` (synthetic.py:31-120)
does with ``rel_scale=True``: an unscaled mesh in the SDF's normalised frame plus a scale and a pose.  The triangulation
is classic table marching cubes with a face-consistent case table, not skimage's Lewiner variant: the vertices lie on
the same crossed grid edges, the triangles between them may differ in ambiguous cells.
"""
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .pipeline import quaternion_apply

__all__ = ["Mesh", "extract_mesh", "sample_points", "render_mesh_depth", "draw_depth_geometry", "visible_mask"]


class Mesh:
    """A triangle mesh on the device, in the normalised unscaled frame of the SDF volume ([-1, 1] for an unpadded
    grid), with the reference's ``synthetic.Mesh`` meaning of ``scale`` / ``rel_scale`` and of the pose.

    vertices (V,3) float32, faces (F,3) int32 (the vertex indices of each triangle; (b-a) x (c-a) points out of the
    object), normals (V,3) float32 or None.  ``position`` (3,) and ``orientation`` (4,) (x, y, z, w) are settable
    attributes, as in the reference's ``Object`` (default: the identity pose)."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor] = None,
                 scale: float = 1.0, rel_scale: bool = True, position=None, orientation=None) -> None:
        self.vertices = vertices
        self.faces = faces
        self.normals = normals
        self._position, self._orientation = None, None   # the identity pose, made on first use (a batch of N
        if position is not None:                          # meshes then costs no per-mesh upload)
            self.position = position
        if orientation is not None:
            self.orientation = orientation
        self.update_scale(scale, rel_scale)

    @property
    def position(self) -> torch.Tensor:
        if self._position is None:
            self._position = torch.zeros(3, device=self.vertices.device)
        return self._position

    @position.setter
    def position(self, value) -> None:
        self._position = torch.as_tensor(value, dtype=torch.float32, device=self.vertices.device).reshape(3)

    @property
    def orientation(self) -> torch.Tensor:
        if self._orientation is None:
            self._orientation = torch.tensor([0.0, 0.0, 0.0, 1.0], device=self.vertices.device)
        return self._orientation

    @orientation.setter
    def orientation(self, value) -> None:
        self._orientation = torch.as_tensor(value, dtype=torch.float32, device=self.vertices.device).reshape(4)

    def update_scale(self, scale: float = 1.0, rel_scale: bool = False) -> None:
        """synthetic.py:90-117: relative = a factor on the original mesh; absolute = half the largest extent"""
        self.rel_scale = bool(rel_scale)
        self.scale = float(scale)
        self._factor = self.scale if self.rel_scale else self.scale / self._original_scale()

    def _original_scale(self) -> float:
        """half the largest x / y / z extent of the unscaled mesh (synthetic.py:119-127)"""
        if self.vertices.shape[0] == 0:
            return 1.0
        ext = self.vertices.amax(0) - self.vertices.amin(0)
        return float(ext.max()) / 2.0

    def scaled_vertices(self) -> torch.Tensor:
        """the vertices with the mesh's scale applied about the origin (the reference's ``_scaled_mesh``)"""
        return self.vertices * self._factor

    def transformed_vertices(self) -> torch.Tensor:
        """R(orientation) (scale v) + position: the mesh in the frame its pose refers to"""
        v = self.scaled_vertices()
        q = self.orientation.to(v).reshape(1, 4).expand(v.shape[0], 4)
        return quaternion_apply(q, v) + self.position.to(v).reshape(1, 3)

    def bounding_box(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lo (3,), hi (3,)): the axis-aligned bounds of the scaled vertices, in the mesh's own frame (before its
        pose).  ``ValueError`` for a mesh without vertices.  Plain torch: works on CPU tensors."""
        if self.vertices.shape[0] == 0:
            raise ValueError("an empty mesh has no bounding box")
        v = self.scaled_vertices()
        return v.amin(0), v.amax(0)

    def oriented_box(self, position=None, orientation=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(center (3,), orientation (4,), extents (3,)) as float64 tensors: ``bounding_box`` with the pose applied -- the
        box ``position + R(orientation) x``, x in [lo, hi], as ``boxes.box_iou`` takes it.  The pose is the mesh's own
        (float32) or the given `position` (3,) / `orientation` (4,), which keep their precision: the algebra runs in
        float64, so a float64 pose gives the box of exactly that pose.  The centre is turned by the NORMALISED quaternion,
        as ``box_iou`` normalises the one it is given."""
        lo, hi = self.bounding_box()
        lo, hi = lo.double(), hi.double()
        pose = lambda given, own: (own if given is None else torch.as_tensor(given)).detach().to(lo.device, torch.float64)
        p, q = pose(position, self.position).reshape(3), pose(orientation, self.orientation).reshape(4)
        center = p + quaternion_apply((q / q.norm()).reshape(1, 4), ((lo + hi) / 2).reshape(1, 3))[0]
        return center, q, hi - lo

    def numpy(self, transformed: bool = False):
        """(vertices (V,3) float32 -- scaled, and posed if `transformed` --, faces (F,3) int32, normals or None)"""
        v = self.transformed_vertices() if transformed else self.scaled_vertices()
        n = None
        if self.normals is not None:
            n = self.normals
            if transformed:
                q = self.orientation.to(n).reshape(1, 4).expand(n.shape[0], 4)
                n = quaternion_apply(q, n)
            n = n.cpu().numpy()
        return v.cpu().numpy(), self.faces.cpu().numpy(), n

    def write_obj(self, path: str, transformed: bool = False) -> None:
        """Wavefront OBJ (1-based indices; ``vn`` lines when the mesh has normals)"""
        v, f, n = self.numpy(transformed)
        with open(path, "w") as fh:
            fh.write(f"# {len(v)} vertices, {len(f)} faces\n")
            np.savetxt(fh, v, fmt="v %.9g %.9g %.9g")
            if n is not None:
                np.savetxt(fh, n, fmt="vn %.9g %.9g %.9g")
                np.savetxt(fh, np.repeat(f + 1, 2, axis=1), fmt="f %d//%d %d//%d %d//%d")
            else:
                np.savetxt(fh, f + 1, fmt="f %d %d %d")

    def write_ply(self, path: str, transformed: bool = False) -> None:
        """binary little-endian PLY (float vertices, optional float normals, int32 triangle lists)"""
        v, f, n = self.numpy(transformed)
        props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
        header += [f"property float {p}" for p in props]
        header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
        vert = np.ascontiguousarray(np.concatenate([v, n], 1) if n is not None else v, dtype="<f4")
        face = np.zeros(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        face["n"] = 3
        face["i"] = f
        with open(path, "wb") as fh:
            fh.write(("\n".join(header) + "\n").encode("ascii"))
            fh.write(vert.tobytes())
            fh.write(face.tobytes())

    def sample_points_uniformly(self, number_of_points: int = 100, seed: int = 0, transformed: bool = True,
                                normals: bool = False, return_triangles: bool = False):
        """``number_of_points`` points uniformly distributed over the surface (open3d's ``sample_points_uniformly``
        rule: triangle by area, then barycentrics (1 - sqrt r1, sqrt r1 (1 - r2), sqrt r1 r2)), on the GPU
        (``sdfr_sample_points``, csrc/metrics.hip).

        The mesh is scaled, and posed if `transformed` (else only scaled, as ``numpy(transformed=False)``).  The random
        stream depends on `seed` and the sample index only: the same seed gives the same samples on every call, and
        two meshes sampled with one seed use the same random numbers (as the reference samples ground truth and
        estimate).  Returns points (n,3) float32; with `normals` also (n,3) unit normals (the mesh needs vertex
        normals); with `return_triangles` also the (n,) int32 face of every point."""
        pts, nrm, tri = _sample([self], number_of_points, seed, transformed, normals)
        out = (pts[0],) + ((nrm[0],) if normals else ()) + ((tri[0],) if return_triangles else ())
        return out[0] if len(out) == 1 else out

    def render_depth(self, camera, position=None, orientation=None, convention: str = "opengl", near: float = 0.0,
                     return_triangles: bool = False, out: Optional[torch.Tensor] = None):
        """The (H,W) depth image of this mesh through `camera` at the origin (``render_mesh_depth`` for one mesh):
        at its own pose, or at `position` (3,) / `orientation` (4,) where given."""
        pos = None if position is None else torch.as_tensor(position, dtype=torch.float32).reshape(1, 3)
        ori = None if orientation is None else torch.as_tensor(orientation, dtype=torch.float32).reshape(1, 4)
        res = render_mesh_depth(self, camera, pos, ori, convention, near, return_triangles,
                                None if out is None else out.view((1,) + tuple(out.shape)))
        return (res[0][0], res[1][0]) if return_triangles else res[0]

    def to_sdf(self, cells_per_dim: int = 64, padding: int = 0, normalize: bool = True, signed: bool = True,
               return_triangles: bool = False, return_winding: bool = False, out: Optional[torch.Tensor] = None):
        """The (R,R,R) SDF volume of this mesh (``sdf_utils.mesh_to_sdf`` for one mesh): exact distances, signed by
        the generalised winding number, on the GPU."""
        from .sdf_utils import mesh_to_sdf
        return mesh_to_sdf(self, cells_per_dim, padding, normalize, signed, return_triangles, return_winding, out)

    @classmethod
    def from_file(cls, path: str, scale: float = 1, rel_scale: bool = False, center: bool = False,
                  device="cuda") -> "Mesh":
        """The reference's ``synthetic.Mesh(path=...)`` (synthetic.py:41-76) without Open3D: a Wavefront OBJ (``v``
        and ``f`` lines; corners written ``i``, ``i/j``, ``i/j/k`` or ``i//k``; negative indices count from the last
        vertex read so far; polygons become triangle fans; everything else is skipped) or a PLY as ``write_ply``
        writes it (binary little-endian or ascii; float x y z, optional nx ny nz, lists of vertex indices).  Vertex
        normals are kept where the file has one per vertex (a PLY's nx ny nz; an OBJ whose corners all read
        ``i//i``).  center: the vertex mean goes to the origin before the scale applies (Open3D's
        ``translate([0, 0, 0], relative=False)``).  `scale` / `rel_scale` as ``update_scale``.  Parsed with numpy on
        the host."""
        with open(path, "rb") as fh:
            head = fh.read(4)
        v, f, n = _read_ply(path) if head[:3] == b"ply" else _read_obj(path)
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError(f"{path}: a face refers to vertex {int(f.max() if f.max() >= len(v) else f.min())} "
                             f"of {len(v)}")
        if center and len(v):
            v = v - v.mean(axis=0)
        dev = torch.device(device)
        return cls(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)).to(dev),
                   None if n is None else torch.from_numpy(np.ascontiguousarray(n, dtype=np.float32)).to(dev),
                   scale=scale, rel_scale=rel_scale)

    def __repr__(self) -> str:
        return (f"Mesh(V={self.vertices.shape[0]}, F={self.faces.shape[0]}, scale={self.scale}, "
                f"rel_scale={self.rel_scale})")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def extract_mesh(sdf: torch.Tensor, level: float, complete: bool = False,
                 normals: bool = False) -> Union[Mesh, List[Mesh]]:
    """Marching cubes of `sdf` at `level` on the GPU.

    sdf: (R,R,R) -> one ``Mesh``; (N,R,R,R) or (N,1,R,R,R) -> a list of N (one launch sequence for all of them).
    CUDA float32, 2 <= R <= 256.  complete: treat every grid as padded by one layer of 1.0 (the reference's
    ``complete_mesh``: a closed mesh).  normals: per-vertex normals (the grid gradient at the vertex, normalised).
    Raises ``ValueError`` if `level` lies outside [min, max] of a (padded) grid, as skimage's ``marching_cubes`` does.
    One host synchronisation (the per-grid counts), as the reference's ``.cpu()``."""
    single = sdf.dim() == 3
    if sdf.dim() == 5:
        if sdf.shape[1] != 1:
            raise ValueError(f"sdf of shape {tuple(sdf.shape)}: (N,1,R,R,R) expected")
        sdf = sdf[:, 0]
    elif single:
        sdf = sdf[None]
    if sdf.dim() != 4 or not (sdf.shape[1] == sdf.shape[2] == sdf.shape[3]):
        raise ValueError(f"sdf of shape {tuple(sdf.shape)}: (R,R,R), (N,R,R,R) or (N,1,R,R,R) cubic grids expected")
    if not sdf.is_cuda or sdf.dtype != torch.float32:
        raise TypeError("sdf must be a CUDA float32 tensor (sdfest_amd has no CPU path)")
    N, R = int(sdf.shape[0]), int(sdf.shape[1])
    sdf = sdf.detach().contiguous()
    dev = sdf.device
    L = _lib.lib()
    cpl = 1 if complete else 0
    ws = _lib.workspace(L.sdfr_mesh_workspace_bytes(N, R, cpl), "sdfr_mesh_workspace_bytes", dev)
    totals = torch.empty((N, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lvl = float(np.float32(level))
    with torch.cuda.device(dev):
        _lib.check(L.sdfr_mesh_count(_ptr(sdf), N, R, cpl, lvl, _ptr(totals), _ptr(ws), ws.numel(), dev.index,
                                     stream), "sdfr_mesh_count")
        h = totals.cpu().numpy()
    lo, hi = h[:, 2].copy().view(np.float32), h[:, 3].copy().view(np.float32)
    bad = np.nonzero(~((lo <= lvl) & (lvl <= hi)))[0]
    if len(bad):
        n = int(bad[0])
        raise ValueError(f"Surface level must be within volume data range (grid {n}: level {level} outside "
                         f"[{lo[n]}, {hi[n]}])")
    nv, nf = h[:, 0].astype(np.int64), h[:, 1].astype(np.int64)
    V, F = int(nv.sum()), int(nf.sum())
    verts = torch.empty((max(V, 1), 3), dtype=torch.float32, device=dev)
    faces = torch.empty((max(F, 1), 3), dtype=torch.int32, device=dev)
    nrm = torch.empty((max(V, 1), 3), dtype=torch.float32, device=dev) if normals else None
    if V:
        with torch.cuda.device(dev):
            _lib.check(L.sdfr_mesh_emit(_ptr(sdf), N, R, cpl, lvl, _ptr(totals), _ptr(verts), _ptr(nrm), _ptr(faces),
                                        _ptr(ws), ws.numel(), dev.index, stream), "sdfr_mesh_emit")
    vo = np.concatenate([[0], np.cumsum(nv)])
    fo = np.concatenate([[0], np.cumsum(nf)])
    meshes = [Mesh(verts[vo[n]:vo[n + 1]], faces[fo[n]:fo[n + 1]],
                   nrm[vo[n]:vo[n + 1]] if nrm is not None else None) for n in range(N)]
    return meshes[0] if single else meshes


# sdfr_sample_mesh (include/sdfr.h): 72 bytes
_SAMPLE_RECORD = np.dtype({"names": ["vertices", "faces", "normals", "cdf_offset", "num_vertices", "num_faces",
                                     "factor", "quat", "position"],
                           "formats": ["<u8", "<u8", "<u8", "<i8", "<i4", "<i4", "<f4", ("<f4", 4), ("<f4", 3)],
                           "offsets": [0, 8, 16, 24, 32, 36, 40, 44, 60], "itemsize": 72})
# the float32 words of a record that hold a float field (or an array of them)
_FLOATS = {name: slice(_SAMPLE_RECORD.fields[name][1] // 4,
                       (_SAMPLE_RECORD.fields[name][1] + _SAMPLE_RECORD.fields[name][0].itemsize) // 4)
           for name in ("factor", "quat", "position")}


class _MeshTable:
    """The device table of K ``sdfr_sample_mesh`` records that ``sdfr_sample_points``, ``sdfr_mesh_depth`` and
    ``sdfr_mesh_sdf`` read (csrc/mesh_record.hpp), record k for ``meshes[k]``: the one place that writes the format.

    Every record gets the mesh's buffers, its scale (``_factor``) and the identity pose; ``factor`` (K,), ``quat`` (K,4)
    and ``position`` (K,3) are float32 views of those columns of the device table, to be rewritten in place -- from
    device tensors nothing is read back -- and ``set_poses`` fills the pose from tensors or from the meshes.  A mesh
    that occurs several times is converted once and its record written once (the repeats are one array copy).
    verb: what the caller does, for the error texts.  normals: every mesh must have vertex normals, and the records
    point to them.  empty: the rest of the error for a mesh without faces, or None: such a mesh gets a record with
    ``num_faces = 0``.

    table: the device tensor, (K, 18) float32 words of which only those columns hold floats, or None when no record
    has a face (there is nothing to launch, and nothing is uploaded); total_faces, max_faces: the sum and the largest of
    the records' face counts (record k's ``cdf_offset`` is the sum over the records before it); vertices: record k's
    float32 vertices as the kernels read them (None for an empty mesh); keep: the tensors the table points to, to be
    held until the launches that read them are on the stream."""

    def __init__(self, meshes: List[Mesh], verb: str, normals: bool = False, empty: Optional[str] = None) -> None:
        if not meshes:
            raise ValueError(f"no meshes to {verb}")
        faces = [int(m.faces.shape[0]) if m.vertices.shape[0] else 0 for m in meshes]
        if empty is not None and 0 in faces:
            raise ValueError(f"mesh {faces.index(0)} {empty}")
        dev = meshes[0].vertices.device
        if dev.type != "cuda":
            raise TypeError("meshes must live on a CUDA device (sdfest_amd has no CPU path)")
        rec = np.zeros(len(meshes), dtype=_SAMPLE_RECORD)
        first, again, starts, total = {}, [], [], 0
        self._converted = {}     # id(mesh) -> its (vertices, faces, normals) as the kernels read them
        for k, (m, F) in enumerate(zip(meshes, faces)):
            if m.vertices.device != dev:
                raise ValueError("all meshes must live on one device")
            if normals and m.normals is None:
                raise ValueError(f"mesh {k} has no vertex normals (extract_mesh(..., normals=True))")
            starts.append(total if F else 0)
            total += F
            if first.setdefault(id(m), k) != k:
                again.append(k)     # a mesh seen before: its record is copied below, nothing is converted or written
                continue
            r = rec[k]
            r["factor"], r["quat"] = m._factor, (0.0, 0.0, 0.0, 1.0)
            if F == 0:
                continue
            v = m.vertices.detach().to(torch.float32).contiguous()
            f = m.faces.detach().to(torch.int32).contiguous()
            nr = m.normals.detach().to(torch.float32).contiguous() if normals else None
            self._converted[id(m)] = (v, f, nr)
            r["vertices"], r["faces"], r["num_vertices"], r["num_faces"] = v.data_ptr(), f.data_ptr(), v.shape[0], F
            r["cdf_offset"] = starts[k]
            if normals:
                r["normals"] = nr.data_ptr()
        if again:     # 256 poses of one mesh: two array assignments, not 255 records field by field
            rec[again] = rec[[first[id(meshes[k])] for k in again]]
            rec["cdf_offset"] = starts
        self.meshes, self.device, self.total_faces, self.max_faces = meshes, dev, total, max(faces)
        self.keep = list(self._converted.values())
        self.table = None
        if total:
            words = rec.view(np.float32).reshape(len(meshes), -1)     # pointers and counts are opaque bits in here
            self.table = torch.from_numpy(words).pin_memory().to(dev, non_blocking=True)

    vertices = property(lambda self: [self._converted.get(id(m), (None,))[0] for m in self.meshes])
    factor = property(lambda self: self.table[:, _FLOATS["factor"].start])
    quat = property(lambda self: self.table[:, _FLOATS["quat"]])
    position = property(lambda self: self.table[:, _FLOATS["position"]])

    def set_poses(self, quat: Optional[torch.Tensor] = None, position: Optional[torch.Tensor] = None) -> None:
        """the records' poses from (K,4) / (K,3) tensors; None: every mesh's own orientation / position"""
        for name, given, own in (("quat", quat, "orientation"), ("position", position, "position")):
            if given is None:
                given = torch.stack([getattr(m, own).detach().to(self.device, torch.float32) for m in self.meshes])
            self.table[:, _FLOATS[name]] = given.detach().to(self.device, torch.float32)


def _sample(meshes: List[Mesh], n: int, seed: int, transformed: bool, normals: bool):
    """points (K,n,3), normals (K,n,3) or None, triangles (K,n) int32 for K meshes on one device: one launch
    sequence, no host synchronisation"""
    n = int(n)
    if n < 1:
        raise ValueError(f"number_of_points={n} must be >= 1")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed={seed} must be in [0, 2^64)")
    tab = _MeshTable(meshes, "sample", normals=normals, empty="has no faces to sample")
    if transformed:
        tab.set_poses()
    dev, K = tab.device, len(meshes)
    L = _lib.lib()
    ws = _lib.workspace(L.sdfr_sample_workspace_bytes(K, tab.total_faces, tab.max_faces),
                        "sdfr_sample_workspace_bytes", dev)
    pts = torch.empty((K, n, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((K, n, 3), dtype=torch.float32, device=dev) if normals else None
    tri = torch.empty((K, n), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(L.sdfr_sample_points(_ptr(tab.table), K, tab.total_faces, tab.max_faces, n, int(seed), _ptr(pts),
                                        _ptr(nrm), _ptr(tri), _ptr(ws), ws.numel(), dev.index, stream),
                   "sdfr_sample_points")
    del tab   # freed tensors are reused only by later work on this stream: the launches read them first
    return pts, nrm, tri


def sample_points(meshes: List[Mesh], number_of_points: int, seed: int = 0, transformed: bool = True) -> torch.Tensor:
    """``Mesh.sample_points_uniformly`` for K meshes in one launch sequence: (K, number_of_points, 3) float32.  Mesh k's
    points equal ``meshes[k].sample_points_uniformly(number_of_points, seed, transformed)`` bit for bit."""
    return _sample(list(meshes), number_of_points, seed, transformed, False)[0]


# ---- files ------------------------------------------------------------------------------------------------------------
def _read_obj(path: str):
    """(vertices (V,3) float64, faces (F,3) int64 zero-based, normals (V,3) or None) of a Wavefront OBJ"""
    verts, norms, faces, fnorm = [], [], [], []
    with open(path, "r", errors="replace") as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "vn":
                norms.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                vi, ni = [], []
                for corner in tok[1:]:
                    parts = corner.split("/")
                    i = int(parts[0])
                    vi.append(i - 1 if i > 0 else len(verts) + i)
                    k = int(parts[2]) if len(parts) > 2 and parts[2] else 0
                    ni.append(k - 1 if k > 0 else (len(norms) + k if k < 0 else -1))
                if len(vi) < 3:
                    raise ValueError(f"{path}: a face with {len(vi)} corners")
                for j in range(1, len(vi) - 1):     # a fan about the first corner
                    faces.append([vi[0], vi[j], vi[j + 1]])
                    fnorm.append([ni[0], ni[j], ni[j + 1]])
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = None
    if len(norms) == len(v) and len(f) and np.array_equal(np.asarray(fnorm, dtype=np.int64), f):
        n = np.asarray(norms, dtype=np.float64).reshape(-1, 3)
    return v, f, n


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _read_ply(path: str):
    """(vertices, faces, normals or None) of a PLY with a vertex element (scalar properties, x y z among them) followed
    by a face element whose one property is the list of vertex indices"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if end < 0:
        raise ValueError(f"{path}: no end_header")
    body = data[data.index(b"\n", end) + 1:]
    fmt, elements = None, []
    for line in data[:end].decode("ascii", errors="replace").splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property" and elements:
            elements[-1][2].append(tok[1:])
    if fmt not in ("binary_little_endian", "ascii") or [e[0] for e in elements[:2]] != ["vertex", "face"]:
        raise ValueError(f"{path}: a binary little-endian or ascii PLY with a vertex and a face element is expected")
    (_, nv, vprops), (_, nf, fprops) = elements[:2]
    if any(p[0] == "list" for p in vprops) or len(fprops) != 1 or fprops[0][0] != "list":
        raise ValueError(f"{path}: scalar vertex properties and one face index list are expected")
    names = [p[1] for p in vprops]
    ctype, itype = _PLY_TYPES[fprops[0][1]], _PLY_TYPES[fprops[0][2]]
    if fmt == "ascii":
        rows = [ln.split() for ln in body.decode("ascii").splitlines() if ln.strip()]
        vert = {nm: np.array([float(r[j]) for r in rows[:nv]]) for j, nm in enumerate(names)}
        polys = [[int(x) for x in r[1:1 + int(r[0])]] for r in rows[nv:nv + nf]]
    else:
        vdt = np.dtype([(nm, "<" + _PLY_TYPES[p[0]]) for nm, p in zip(names, vprops)])
        rec = np.frombuffer(body, dtype=vdt, count=nv)
        vert = {nm: rec[nm].astype(np.float64) for nm in names}
        rest = body[nv * vdt.itemsize:]
        tri = np.dtype([("n", "<" + ctype), ("i", "<" + itype, (3,))])
        polys = None
        if len(rest) >= nf * tri.itemsize:    # all triangles (what write_ply writes): one read
            cand = np.frombuffer(rest, dtype=tri, count=nf)
            if nf == 0 or (cand["n"] == 3).all():
                polys = cand["i"].astype(np.int64)
        if polys is None:
            polys, o = [], 0
            cs, isz = np.dtype(ctype).itemsize, np.dtype(itype).itemsize
            for _ in range(nf):
                c = int(np.frombuffer(rest, dtype="<" + ctype, count=1, offset=o)[0])
                polys.append(np.frombuffer(rest, dtype="<" + itype, count=c, offset=o + cs).astype(np.int64).tolist())
                o += cs + c * isz
    if isinstance(polys, list):
        polys = [[p[0], p[j], p[j + 1]] for p in polys for j in range(1, len(p) - 1)]
    v = np.stack([vert["x"], vert["y"], vert["z"]], 1).reshape(-1, 3)
    n = np.stack([vert["nx"], vert["ny"], vert["nz"]], 1) if all(k in vert for k in ("nx", "ny", "nz")) else None
    return v, np.asarray(polys, dtype=np.int64).reshape(-1, 3), n


# ---- depth images -----------------------------------------------------------------------------------------------------
_CONVENTIONS = {"opengl": "SDFR_MESH_DEPTH_OPENGL", "open3d": "SDFR_MESH_DEPTH_OPEN3D", "opencv": "SDFR_MESH_DEPTH_OPEN3D"}


def render_mesh_depth(meshes: Union[Mesh, List[Mesh]], camera, positions: Optional[torch.Tensor] = None,
                      orientations: Optional[torch.Tensor] = None, convention: str = "opengl", near: float = 0.0,
                      return_triangles: bool = False, out: Optional[torch.Tensor] = None):
    """Depth images of triangle meshes on the GPU (``sdfr_mesh_depth``, csrc/raster.hip): per pixel the smallest z-depth
    over the triangles its centre ray meets with depth > `near`, 0 where it meets none (the reference's ``depth != 0``
    mask convention); both faces of a triangle count, there is no far plane.

    meshes: a ``Mesh`` or a list of K.  positions (V,3) / orientations (V,4): poses that replace the meshes' own -- one
    mesh and V poses give (V,H,W), K meshes take K poses; without them every mesh is drawn at its own pose.  The mesh's
    scale (``_factor``) always applies.  The camera sits at the origin of the frame the poses refer to; convention
    "opengl" (x right, y up, looking along -z: ``render_depth_gpu``'s frame) or "open3d" / "opencv" (x right, y down,
    looking along +z: the reference's ``draw_depth_geometry``).  `camera.s` (skew) must be 0.  out: a (K,H,W) float32
    buffer to write into.  An empty mesh gives an image of zeros.  Returns the (K,H,W) depth; with `return_triangles`
    also the (K,H,W) int32 face index behind every pixel (-1: none).  One launch sequence for all images, nothing read
    back; poses given as device tensors stay on the device."""
    if convention not in _CONVENTIONS:
        raise ValueError(f"convention {convention!r}: expected one of {sorted(_CONVENTIONS)}")
    fx, fy, cx, cy, s = camera.get_pinhole_camera_parameters(0.5)
    if s != 0:
        raise ValueError(f"camera skew s={s} is not supported (only s = 0)")
    near = float(near)
    if not (0.0 <= near < float("inf")):
        raise ValueError(f"near={near} must be >= 0 and finite")
    meshes = [meshes] if isinstance(meshes, Mesh) else list(meshes)
    for name, t, w in (("positions", positions, 3), ("orientations", orientations, 4)):
        if t is not None and (t.dim() != 2 or t.shape[1] != w):
            raise ValueError(f"{name} of shape {tuple(t.shape)}: (V,{w}) expected")
    V = next((int(t.shape[0]) for t in (positions, orientations) if t is not None), None)
    if positions is not None and orientations is not None and positions.shape[0] != orientations.shape[0]:
        raise ValueError(f"{positions.shape[0]} positions for {orientations.shape[0]} orientations")
    if V is not None and len(meshes) == 1:
        meshes = meshes * V
    elif V is not None and V != len(meshes):
        raise ValueError(f"{V} poses for {len(meshes)} meshes (one pose per mesh, or one mesh)")
    tab = _MeshTable(meshes, "render")     # a mesh without faces: num_faces = 0, the kernel stores an image of zeros
    dev, K = tab.device, len(meshes)
    W, H = int(camera.width), int(camera.height)
    if out is not None:
        if tuple(out.shape) != (K, H, W) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous ({K},{H},{W}) float32 tensor on {dev}")
        depth = out
    else:
        depth = torch.empty((K, H, W), dtype=torch.float32, device=dev)
    tri = torch.empty((K, H, W), dtype=torch.int32, device=dev) if return_triangles else None
    if tab.total_faces == 0:
        depth.zero_()
        if tri is not None:
            tri.fill_(-1)
        return (depth, tri) if return_triangles else depth
    tab.set_poses(orientations, positions)
    _mesh_depth_launch(tab.table, tab.total_faces, tab.max_faces, (cx, cy, fx, fy), near,
                       _lib.ABI[_CONVENTIONS[convention]], depth, tri)
    del tab   # as in _sample: freed tensors are reused only by later work on this stream
    return (depth, tri) if return_triangles else depth


def _mesh_depth_launch(table: torch.Tensor, total_faces: int, max_faces: int, intrinsics, near: float, flags: int,
                       depth: torch.Tensor, triangles: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None) -> None:
    """``sdfr_mesh_depth`` on a device table of K 72-byte records into depth (K,H,W): kernels on the current stream
    and nothing else, so with a `workspace` made beforehand (``sdfr_mesh_depth_workspace_bytes``) the call can be
    captured into a graph and replayed after the table's poses were rewritten in place"""
    dev = depth.device
    K, H, W = (int(x) for x in depth.shape)
    cx, cy, fx, fy = intrinsics
    L = _lib.lib()
    ws = _lib.workspace(L.sdfr_mesh_depth_workspace_bytes(K, total_faces, max_faces, W, H),
                        "sdfr_mesh_depth_workspace_bytes", dev, workspace)
    with torch.cuda.device(dev):
        _lib.check(L.sdfr_mesh_depth(_ptr(table), K, total_faces, max_faces, W, H, cx, cy, fx, fy, near, flags,
                                     _ptr(depth), _ptr(triangles), _ptr(ws), ws.numel(), dev.index,
                                     torch.cuda.current_stream(dev).cuda_stream), "sdfr_mesh_depth")


def draw_depth_geometry(obj: Mesh, camera) -> torch.Tensor:
    """The reference's ``synthetic.draw_depth_geometry(obj, camera)`` (synthetic.py:142-171): the (H,W) float32 depth
    image, on the device, of `obj` at its own pose in the Open3D camera frame (the camera at the origin, x right, y
    down, looking along +z), 0 where no triangle is seen, back faces shown.  Skew (``camera.s != 0``) raises
    ``ValueError``: the rasteriser has no skew term, as ``ray_setup`` in render.hip has none."""
    return render_mesh_depth(obj, camera, convention="open3d")[0]


def visible_mask(rendered: torch.Tensor, observed: torch.Tensor, margin: float = 0.01, return_masked: bool = False,
                 return_counts: bool = False):
    """The instance mask of annotated frames on the GPU (``sdfr_visible_mask``, csrc/annotate.hip; the reference's
    ``AnnotatedRedwoodDataset._compute_mask``, redwood_dataset.py:262-275): ``(rendered != 0) & ~((observed != 0) &
    (observed < rendered - margin))`` -- the pixels the ground-truth mesh covers, minus those where the sensor saw
    something more than `margin` in front of it.

    rendered, observed: (H,W) or (B,H,W) float32 CUDA tensors of one shape; a contiguous view is read where it is, at
    whatever 4-byte offset into a larger buffer it starts (anything else is copied first).  Returns the
    ``torch.bool`` mask of that shape; with `return_masked` also ``where(mask, observed, 0)`` float32; with
    `return_counts` also (B,4) (or (4,)) int32 on the device: covered, visible, occluded, valid (visible with a depth
    reading: the points of the masked point cloud).  One launch sequence for all images, nothing read back."""
    if rendered.shape != observed.shape or rendered.dim() not in (2, 3):
        raise ValueError(f"rendered {tuple(rendered.shape)} and observed {tuple(observed.shape)}: two (H,W) or (B,H,W) "
                         "tensors of one shape expected")
    for name, t in (("rendered", rendered), ("observed", observed)):
        if not t.is_cuda or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a CUDA float32 tensor (sdfest_amd has no CPU path)")
    if rendered.device != observed.device:
        raise ValueError("rendered and observed must live on one device")
    margin = float(margin)
    if not (0.0 <= margin < float("inf")):
        raise ValueError(f"margin={margin} must be >= 0 and finite")
    single = rendered.dim() == 2
    shape = tuple(rendered.shape)
    B, H, W = (1,) + shape if single else shape
    if H < 1 or W < 1:
        raise ValueError(f"images of {H} x {W} pixels")
    dev = rendered.device
    rendered, observed = rendered.detach().contiguous(), observed.detach().contiguous()
    mask = torch.empty(shape, dtype=torch.bool, device=dev)
    masked = torch.empty(shape, dtype=torch.float32, device=dev) if return_masked else None
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev) if return_counts else None
    if B:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().sdfr_visible_mask(_ptr(rendered), _ptr(observed), B, H, W, margin, _ptr(mask),
                                                    _ptr(masked), _ptr(counts), dev.index,
                                                    torch.cuda.current_stream(dev).cuda_stream), "sdfr_visible_mask")
    out = (mask,) + ((masked,) if return_masked else ()) + (((counts[0] if single else counts),) if return_counts else ())
    return out[0] if len(out) == 1 else out
