"""CPU: the resident-grid entry points (include/sdfr.h) are declared, exported, bound with one more int than their
predecessors, and validate their arguments before any HIP call.  (GPU behaviour: tests/test_grid_resident_gpu.py.)"""
import ctypes


def test_entry_points_are_declared_exported_and_bound():
    from sdfest_amd import _lib
    L = _lib.lib()
    for new, old in (("sdfr_render_forward_grid_resident", "sdfr_render_forward_resident"),
                     ("sdfr_render_step_forward_grid_resident", "sdfr_render_step_forward_resident")):
        assert hasattr(L, new) and hasattr(L, old)
        (res_new, args_new), (res_old, args_old) = _lib.SIGNATURES[new], _lib.SIGNATURES[old]
        assert res_new == res_old == ctypes.c_int
        # the predecessor's arguments with `grid_resident` between depth_resident and device
        assert args_new == args_old[:-2] + [ctypes.c_int] + args_old[-2:]
    assert (_lib.ABI["SDFR_GRID_RESIDENT"], _lib.ABI["SDFR_GRID_RESIDENT_VERIFY"]) == (1, 2)
    assert 8 < _lib.ABI["SDFR_SYNC_GRID_MISMATCH_WORD"] < 32        # a free word of the 32-word sync header


def test_argument_errors_without_gpu():
    from sdfest_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q0 = ctypes.cast(buf, ctypes.c_void_p)   # a non-NULL pointer that is never dereferenced
    for flag in (0, 1, 2):
        rc = L.sdfr_render_forward_grid_resident(None, 1, 0, None, None, None, 17, 8, 8, 4.0, 4.0, 4.0, 4.0, 0.01, None,
                                                 None, 0, None, 0, 0, flag, 0, None)
        assert rc == _lib.ABI["SDFR_E_INVALID"] and b"R=1" in L.sdfr_last_error()
        rc = L.sdfr_render_forward_grid_resident(None, 16, 0, None, None, None, 17, 8, 8, 4.0, 4.0, 4.0, 4.0, 0.01, None,
                                                 None, 0, None, 0, 0, flag, 0, None)
        assert rc == _lib.ABI["SDFR_E_NULL"]
        rc = L.sdfr_render_step_forward_grid_resident(q0, 16, 0, q0, q0, q0, 17, 8, 8, 4.0, 4.0, 4.0, 4.0, 0.01, q0, None,
                                                      0, q0, 1 << 30, None, None, 0, 0, flag, 0, None)
        assert rc == _lib.ABI["SDFR_E_NULL"] and b"g_sdf" in L.sdfr_last_error()
        rc = L.sdfr_render_step_forward_grid_resident(q0, 16, 0, q0, q0, q0, 17, 8, 8, 4.0, 4.0, 4.0, 4.0, 0.01, q0, q0,
                                                      5, q0, 1 << 30, None, None, 0, 0, flag, 0, None)
        assert rc == _lib.ABI["SDFR_E_INVALID"]                    # g_sdf_view_stride must be 0 or R^3
