"""A directory of meshes -> the SDF volumes a VAE is trained on: the conversion step of the reference's
``vae/scripts/process_shapenet.py`` (its interactive mesh filtering is not part of this).

Every ``.obj`` / ``.ply`` under --inpath goes through ``Mesh.from_file`` and ``sdfest_amd.mesh_to_sdf`` (the reference's
framing: bounding-box centre to the origin, longest extent to [-1, 1] less the padding) and is written to
``outpath/00000.npy, 00001.npy, ...`` in sorted path order: float32 (R,R,R), the files ``sdf_dataset.SDFDataset`` loads.
One JSON line per mesh on stdout: its path, output file, face count and `uncertain_share`, the share of grid points
whose winding number lies within 0.25 of 0.5 -- near 0 for a closed, consistently oriented mesh, large for an open or
inconsistently oriented one, where the sign of the field means little.  It is reported, never used to skip a mesh.

    python tools/process_meshes.py --inpath DIR --outpath DIR --resolution 64 --padding 2 [--batch 8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mesh_paths(inpath):
    found = []
    for dirpath, _, files in os.walk(inpath):
        found += [os.path.join(dirpath, f) for f in files if f.lower().endswith((".obj", ".ply"))]
    return sorted(found)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--inpath", required=True)
    ap.add_argument("--outpath", required=True)
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--padding", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8, help="meshes per launch sequence")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    from sdfest_amd import Mesh, mesh_to_sdf
    paths = mesh_paths(a.inpath)
    os.makedirs(a.outpath, exist_ok=True)
    for first in range(0, len(paths), a.batch):
        chunk = paths[first:first + a.batch]
        meshes = [Mesh.from_file(p, device=a.device) for p in chunk]
        sdf, winding = mesh_to_sdf(meshes, a.resolution, a.padding, return_winding=True)
        # NaN (a mesh of degenerate faces only) counts as uncertain
        share = (~((winding - 0.5).abs() >= 0.25)).flatten(1).float().mean(1).cpu().numpy()
        volumes = sdf.cpu().numpy()
        for j, path in enumerate(chunk):
            name = f"{first + j:05d}.npy"
            np.save(os.path.join(a.outpath, name), volumes[j])
            print(json.dumps({"path": os.path.relpath(path, a.inpath), "file": name,
                              "faces": int(meshes[j].faces.shape[0]), "uncertain_share": round(float(share[j]), 6)}),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
