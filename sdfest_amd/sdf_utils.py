"""Triangle mesh -> SDF volume on the GPU (``sdfr_mesh_sdf``, csrc/mesh_sdf.hip): the reference's
``vae/sdf_utils.py::mesh_to_sdf``, the step that makes every volume the VAE is trained on and encodes.

The reference delegates to the external ``mesh_to_sdf`` package (100 depth scans of the mesh, a KD-tree over the
scanned points, the sign from visibility).  Here the field is exact: the distance from every grid point to the closest
point of the closest triangle, signed by the generalised winding number.  The inverse
direction, the reference's ``mesh_from_sdf``, is ``sdfest_amd.extract_mesh``.
"""
from typing import List, Optional, Tuple, Union

import torch

from . import _lib
from .mesh import Mesh, _MeshTable, _ptr

__all__ = ["mesh_to_sdf", "normalization", "normalized_mesh"]


def _check_cells(cells_per_dim: int, padding: int) -> Tuple[int, int]:
    R, p = int(cells_per_dim), int(padding)
    if not 2 <= R <= 256:
        raise ValueError(f"cells_per_dim={cells_per_dim} must be in [2, 256]")
    if p < 0 or 2 * p >= R:
        raise ValueError(f"padding={padding} must be in [0, cells_per_dim / 2)")
    return R, p


def normalization(vertices: torch.Tensor, cells_per_dim: int = 64, padding: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's framing (``scale_to_unit_cube``, then ``(cells_per_dim - 2 padding) / cells_per_dim``) as a
    uniform scale s () and a translation t (3,) on the vertices' device, without a host read: s v + t has its
    bounding-box centre at the origin and its longest extent 2 (cells_per_dim - 2 padding) / cells_per_dim."""
    R, p = _check_cells(cells_per_dim, padding)
    v = vertices.detach().to(torch.float32)
    lo, hi = v.amin(0), v.amax(0)
    s = (2.0 / (hi - lo).amax()) * ((R - 2 * p) / R)
    return s, -s * ((lo + hi) * 0.5)


def normalized_mesh(mesh: Mesh, cells_per_dim: int = 64, padding: int = 0) -> Mesh:
    """`mesh` (its vertices as stored: scale and pose do not apply) in the frame ``mesh_to_sdf(normalize=True)`` puts it
    in, as a new ``Mesh`` at the identity pose"""
    s, t = normalization(mesh.vertices, cells_per_dim, padding)
    return Mesh(mesh.vertices.detach().to(torch.float32) * s + t, mesh.faces, mesh.normals)


def _mesh_sdf_table(meshes: List[Mesh], normalize: bool, cells_per_dim: int, padding: int):
    """(device table of K sdfr_sample_mesh records, total faces, largest face count, the tensors the table points to)"""
    tab = _MeshTable(meshes, "convert", empty="has no faces")
    if normalize:   # the framing stays on the device: nothing is read back, the vertices are not copied
        frames = [normalization(v, cells_per_dim, padding) for v in tab.vertices]
        tab.factor[:] = torch.stack([s for s, _ in frames])
        tab.position[:] = torch.stack([t for _, t in frames])
    else:
        tab.set_poses()
    return tab.table, tab.total_faces, tab.max_faces, tab.keep


def _mesh_sdf_launch(table: torch.Tensor, total_faces: int, max_faces: int, flags: int, sdf: torch.Tensor,
                     triangles: Optional[torch.Tensor] = None, winding: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None) -> None:
    """``sdfr_mesh_sdf`` on a device table of K records into sdf (K,R,R,R): kernels on the current stream and nothing
    else, so with a `workspace` made beforehand (``sdfr_mesh_sdf_workspace_bytes``) the call can be captured into a
    graph"""
    dev = sdf.device
    K, R = int(sdf.shape[0]), int(sdf.shape[1])
    L = _lib.lib()
    ws = _lib.workspace(L.sdfr_mesh_sdf_workspace_bytes(K, total_faces, max_faces, R), "sdfr_mesh_sdf_workspace_bytes",
                        dev, workspace)
    with torch.cuda.device(dev):
        _lib.check(L.sdfr_mesh_sdf(_ptr(table), K, total_faces, max_faces, R, flags, _ptr(sdf), _ptr(triangles),
                                   _ptr(winding), _ptr(ws), ws.numel(), dev.index,
                                   torch.cuda.current_stream(dev).cuda_stream), "sdfr_mesh_sdf")


def mesh_to_sdf(mesh: Union[Mesh, List[Mesh]], cells_per_dim: int = 64, padding: int = 0, normalize: bool = True,
                signed: bool = True, return_triangles: bool = False, return_winding: bool = False,
                out: Optional[torch.Tensor] = None):
    """The SDF volume of a triangle mesh on the GPU: (R,R,R) float32 for a ``Mesh``, (K,R,R,R) for a list of K (one
    launch sequence for all of them), R = `cells_per_dim`, indexed [x][y][z] with grid point i of an axis at
    (i - (R - 1) / 2) 2 / (R - 1): the layout ``extract_mesh`` and the renderer read.

    |value| is the exact Euclidean distance to the mesh (face, edge or vertex, whichever is closest); the value is
    negative where the generalised winding number exceeds 0.5 -- inside a closed mesh whose faces are oriented as
    ``Mesh`` documents.  signed=False: the unsigned distance (bitwise the absolute value of the signed one, without
    the winding work).

    normalize=True is the reference's framing: the mesh's vertices as stored (its scale and pose do not apply) with
    their bounding-box centre at the origin and their longest extent scaled to fill [-1, 1], times
    (cells_per_dim - 2 padding) / cells_per_dim; computed on the device, the vertices are not copied and nothing is
    read back.  normalize=False: the mesh at its own scale and pose, in the frame of ``extract_mesh`` and of the
    renderer (`padding` is then unused).

    return_triangles: also the (…,R,R,R) int32 index of the closest face; return_winding: also the (…,R,R,R) float32
    winding number (far from both 0 and 1 where the mesh is open or inconsistently oriented).  out: a contiguous
    float32 buffer of the result's shape to write into.  A mesh whose every face is degenerate gives a volume of NaN."""
    single = isinstance(mesh, Mesh)
    meshes = [mesh] if single else list(mesh)
    R, p = _check_cells(cells_per_dim, padding)
    if return_winding and not signed:
        raise ValueError("return_winding needs signed=True (the unsigned field does no winding work)")
    table, total, max_f, keep = _mesh_sdf_table(meshes, normalize, R, p)
    dev = table.device
    K = len(meshes)
    shape = (K, R, R, R)
    if out is not None:
        want = shape[1:] if single else shape
        if tuple(out.shape) != want or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {want} float32 tensor on {dev}")
        sdf = out.view(shape)
    else:
        sdf = torch.empty(shape, dtype=torch.float32, device=dev)
    tri = torch.empty(shape, dtype=torch.int32, device=dev) if return_triangles else None
    wind = torch.empty(shape, dtype=torch.float32, device=dev) if return_winding else None
    flags = _lib.ABI["SDFR_MESH_SDF_SIGNED" if signed else "SDFR_MESH_SDF_UNSIGNED"]
    _mesh_sdf_launch(table, total, max_f, flags, sdf, tri, wind)
    del keep   # as in mesh._sample: freed tensors are reused only by later work on this stream
    res = tuple(t[0] if single else t for t in (sdf, tri, wind) if t is not None)
    return res[0] if len(res) == 1 else res
