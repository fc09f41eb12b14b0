"""CPU: the three entry points behind ``MultiObjectRenderAndCompare(views=, track_inliers=)`` -- sdfr_volumes_replicate,
sdfr_volumes_sum_views, sdfr_inlier_ratio_objects -- are declared, exported and bound, and refuse bad arguments with the
project's codes before any HIP call (there is no GPU here)."""
import ctypes
import os
import re

import pytest

from helpers import ROOT

NEW = ("sdfr_volumes_replicate", "sdfr_volumes_sum_views", "sdfr_inlier_ratio_objects")


@pytest.fixture(scope="module")
def L():
    from sdfest_amd import _lib
    _lib.build()
    return _lib.lib()


def test_header_declares_and_library_exports(L):
    from sdfest_amd import _lib
    text = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    declared = set(re.findall(r"SDFR_API\s+[\w\s\*]+?\b(sdfr_\w+)\s*\(", text))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert _lib.ABI["SDFR_VERSION"] == 100
    # every one is named in the header's table of contents (group 3)
    contents = text[:text.index("#ifndef SDFR_H_")]
    for name in NEW:
        assert name in contents, name
    n_rep = len(_lib.SIGNATURES["sdfr_volumes_replicate"][1])
    assert n_rep == len(_lib.SIGNATURES["sdfr_volumes_sum_views"][1]) == 7
    assert len(_lib.SIGNATURES["sdfr_inlier_ratio_objects"][1]) == 17


@pytest.mark.parametrize("name", NEW[:2])
def test_volume_calls_validate_without_gpu(L, name):
    from sdfest_amd import _lib
    INVALID, NULL = _lib.ABI["SDFR_E_INVALID"], _lib.ABI["SDFR_E_NULL"]
    fn = getattr(L, name)
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    assert fn(None, None, 0, 3, 512, 0, None) == 0            # K = 0: a no-op, pointers not looked at
    assert fn(None, None, 2, 3, 0, 0, None) == 0              # empty rows
    assert fn(p, p, -1, 3, 8, 0, None) == INVALID
    assert fn(p, p, 2, 0, 8, 0, None) == INVALID              # no view
    assert fn(p, p, 2, -1, 8, 0, None) == INVALID
    assert fn(p, p, 65536, 1, 8, 0, None) == INVALID          # more rows than a launch's second dimension
    assert name.encode() in L.sdfr_last_error()
    assert fn(None, p, 2, 3, 8, 0, None) == NULL
    assert fn(p, None, 2, 3, 8, 0, None) == NULL
    assert name.encode() in L.sdfr_last_error()


def test_inlier_ratio_objects_validates_without_gpu(L):
    from sdfest_amd import _lib
    INVALID, NULL = _lib.ABI["SDFR_E_INVALID"], _lib.ABI["SDFR_E_NULL"]
    fn = L.sdfr_inlier_ratio_objects
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(din=p, est=p, stride=16, K=2, W=4, H=4, step=p, counts=p, history=p, max_history=3, state=p, params=p,
             n_params=9, best=p):
        return fn(din, est, stride, K, W, H, 0.03, step, counts, history, max_history, state, params, n_params, best, 0,
                  None)

    assert call(din=None, est=None, step=None, counts=None, state=None, params=None, best=None, history=None, K=0) == 0
    assert call(K=-1) == INVALID
    assert call(K=65536) == INVALID
    assert call(W=-1) == INVALID
    assert call(H=-4) == INVALID
    assert call(W=65536, H=65536) == INVALID       # more pixels than an int counts
    assert call(n_params=-1) == INVALID
    assert call(max_history=-1) == INVALID
    assert call(stride=15) == INVALID              # the objects' estimates would overlap
    assert b"sdfr_inlier_ratio_objects" in L.sdfr_last_error()
    for missing in ("din", "est", "step", "counts", "state"):
        assert call(**{missing: None}) == NULL, missing
    assert call(params=None) == NULL               # best_params without params to copy from
    assert b"sdfr_inlier_ratio_objects" in L.sdfr_last_error()
