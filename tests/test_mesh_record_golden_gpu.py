"""GPU: ``render_mesh_depth``, ``mesh_to_sdf`` and ``sample_points`` against recorded bits (tests/golden/mesh_record.npz
of tools/make_mesh_record_goldens.py): the one test that pins what the readers and the writer of the ``sdfr_sample_mesh``
table (csrc/mesh_record.hpp, ``mesh._MeshTable``) compute to values recorded before they were gathered in one place.

The file holds its inputs -- a cube whose faces show all six index orders, a coarse sphere with five bad faces, an
empty mesh, poses, intrinsics -- and every output; the calls are the recorder's own ``compute``, replayed on the stored
inputs, and the comparison is ``torch.equal`` on the int32 views.  A change of one bit anywhere fails it: re-record only
for a change that is meant to move bits, on the commit before that change."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_mesh_record_goldens",
                                               os.path.join(ROOT, "tools", "make_mesh_record_goldens.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "mesh_record.npz")) as z:
        return ({k[3:]: z[k] for k in z.files if k.startswith("in/")},
                {k[4:]: z[k] for k in z.files if k.startswith("out/")})


def test_the_recording_is_not_trivial(golden):
    inp, want = golden
    assert len(want) == 27
    assert {tuple(np.argsort(f).tolist()) for f in inp["f1"]} == tool.ORDERS
    tool.check_not_trivial(want)


def test_outputs_equal_the_recording_bit_for_bit(golden):
    inp, want = golden
    got = tool.compute(inp)
    assert sorted(got) == sorted(want)
    differ = []
    for key, w in want.items():
        g = got[key].cpu()
        assert tuple(g.shape) == w.shape and g.element_size() == 4 == w.itemsize, key
        if not torch.equal(g.view(torch.int32), torch.from_numpy(w).view(torch.int32)):
            differ.append((key, int((g.view(torch.int32) != torch.from_numpy(w).view(torch.int32)).sum())))
    assert not differ, differ
