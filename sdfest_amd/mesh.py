"""Meshes of decoded SDFs: marching cubes on the GPU (``sdfr_mesh_count`` / ``sdfr_mesh_emit``, csrc/mesh.hip).

``extract_mesh`` replaces what ``SDFPipeline.generate_mesh`` does with skimage (simple_setup.py:637-660) for one grid
or a batch of them, and ``Mesh`` carries the result the way the reference's ``synthetic.Mesh`` (synthetic.py:31-120)
does with ``rel_scale=True``: an unscaled mesh in the SDF's normalised frame plus a scale and a pose.  The triangulation
is classic table marching cubes with a face-consistent case table, not skimage's Lewiner variant: the vertices lie on
the same crossed grid edges, the triangles between them may differ in ambiguous cells.
"""
from typing import List, Optional, Union

import numpy as np
import torch

from . import _lib
from .pipeline import quaternion_apply

__all__ = ["Mesh", "extract_mesh", "sample_points"]


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

    def __repr__(self) -> str:
        return (f"Mesh(V={self.vertices.shape[0]}, F={self.faces.shape[0]}, scale={self.scale}, "
                f"rel_scale={self.rel_scale})")


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


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
    ws_bytes = L.sdfr_mesh_workspace_bytes(N, R, cpl)
    if ws_bytes == 0:
        _lib.check(_lib.ABI["SDFR_E_INVALID"], "sdfr_mesh_workspace_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    totals = torch.empty((N, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lvl = float(np.float32(level))
    with torch.cuda.device(dev):
        _lib.check(L.sdfr_mesh_count(_ptr(sdf), N, R, cpl, lvl, _ptr(totals), _ptr(ws), ws_bytes, dev.index, stream),
                   "sdfr_mesh_count")
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
            _lib.check(L.sdfr_mesh_emit(_ptr(sdf), N, R, cpl, lvl, _ptr(totals), _ptr(verts),
                                        _ptr(nrm) if nrm is not None else None, _ptr(faces), _ptr(ws), ws_bytes,
                                        dev.index, stream), "sdfr_mesh_emit")
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


def _sample(meshes: List[Mesh], n: int, seed: int, transformed: bool, normals: bool):
    """points (K,n,3), normals (K,n,3) or None, triangles (K,n) int32 for K meshes on one device: one launch
    sequence, no host synchronisation"""
    n = int(n)
    if n < 1:
        raise ValueError(f"number_of_points={n} must be >= 1")
    if not meshes:
        raise ValueError("no meshes to sample")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed={seed} must be in [0, 2^64)")
    dev = meshes[0].vertices.device
    if dev.type != "cuda":
        raise TypeError("meshes must live on a CUDA device (sdfest_amd has no CPU path)")
    K = len(meshes)
    rec = np.zeros(K, dtype=_SAMPLE_RECORD)
    keep = []
    off = 0
    for k, m in enumerate(meshes):
        if m.vertices.device != dev:
            raise ValueError("all meshes must live on one device")
        F = int(m.faces.shape[0])
        if F == 0 or m.vertices.shape[0] == 0:
            raise ValueError(f"mesh {k} has no faces to sample")
        if normals and m.normals is None:
            raise ValueError(f"mesh {k} has no vertex normals (extract_mesh(..., normals=True))")
        v = m.vertices.detach().to(torch.float32).contiguous()
        f = m.faces.detach().to(torch.int32).contiguous()
        nr = m.normals.detach().to(torch.float32).contiguous() if (normals and m.normals is not None) else None
        keep += [v, f, nr]
        rec[k]["vertices"], rec[k]["faces"] = v.data_ptr(), f.data_ptr()
        rec[k]["normals"] = nr.data_ptr() if nr is not None else 0
        rec[k]["cdf_offset"], rec[k]["num_vertices"], rec[k]["num_faces"] = off, v.shape[0], F
        rec[k]["factor"] = m._factor
        rec[k]["quat"] = (0.0, 0.0, 0.0, 1.0)
        off += F
    max_f = max(int(m.faces.shape[0]) for m in meshes)
    L = _lib.lib()
    ws_bytes = L.sdfr_sample_workspace_bytes(K, off, max_f)
    if ws_bytes == 0:
        _lib.check(_lib.ABI["SDFR_E_INVALID"], "sdfr_sample_workspace_bytes")
    table = torch.from_numpy(rec.view(np.uint8)).pin_memory().to(dev, non_blocking=True)
    if transformed:   # the poses stay on the device: floats 11..14 and 15..17 of each record
        tab = table.view(torch.float32).view(K, _SAMPLE_RECORD.itemsize // 4)
        tab[:, 11:15] = torch.stack([m.orientation.detach().to(dev, torch.float32) for m in meshes])
        tab[:, 15:18] = torch.stack([m.position.detach().to(dev, torch.float32) for m in meshes])
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pts = torch.empty((K, n, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((K, n, 3), dtype=torch.float32, device=dev) if normals else None
    tri = torch.empty((K, n), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(L.sdfr_sample_points(_ptr(table), K, off, max_f, n, int(seed), _ptr(pts),
                                        _ptr(nrm) if nrm is not None else None, _ptr(tri), _ptr(ws), ws_bytes,
                                        dev.index, stream), "sdfr_sample_points")
    del keep   # freed tensors are reused only by later work on this stream: the launches read them first
    return pts, nrm, tri


def sample_points(meshes: List[Mesh], number_of_points: int, seed: int = 0, transformed: bool = True) -> torch.Tensor:
    """``Mesh.sample_points_uniformly`` for K meshes in one launch sequence: (K, number_of_points, 3) float32.  Mesh k's
    points equal ``meshes[k].sample_points_uniformly(number_of_points, seed, transformed)`` bit for bit."""
    return _sample(list(meshes), number_of_points, seed, transformed, False)[0]
