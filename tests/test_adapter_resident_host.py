"""Pooled device memory and the resident C++ adapter: what can be checked without a GPU. The six new exports and their
Python mirrors; their argument checks on a host-only context (E_POINTER first, then E_INVALIDARG, then
COR_E_INVALIDOPERATION); and the resident check program compiled and linked against the header
(on a host-only context it only checks that the pool refuses resident work)."""
import ctypes as C

import numpy as np
from support import compile_cpp, run_exe

NEW = ("sealhip_pool_alloc", "sealhip_pool_release", "sealhip_pool_trim", "sealhip_pool_stats", "sealhip_memcpy_d2d",
       "sealhip_transparency_note")
MODS = [1073738753, 1099511603713, 1152921504606830593]


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("pool_alloc", "pool_release", "pool_trim", "pool_stats", "memcpy_d2d", "transparency_note"):
        assert callable(getattr(S.Context, name))
    assert issubclass(S.PoolBuffer, S.DeviceBuffer)


def test_pool_entries_on_host_only_context():
    import sealhip as S

    L = S.lib()
    ctx = S.Context(S.SCHEME_BFV, 8, MODS, 1, 786433, device=-1)
    h = ctx.handle
    err = lambda: L.sealhip_last_error_string().decode()
    p = C.c_void_p()
    buf = np.zeros(16, dtype=np.uint64)
    # E_POINTER before anything else, even with invalid sizes
    assert L.sealhip_pool_alloc(None, 0, C.byref(p)) == S.E_POINTER
    assert L.sealhip_pool_alloc(h, 0, None) == S.E_POINTER
    assert L.sealhip_pool_release(None, buf.ctypes.data) == S.E_POINTER
    assert L.sealhip_pool_release(h, None) == S.E_POINTER
    assert L.sealhip_pool_trim(None) == S.E_POINTER
    assert L.sealhip_pool_stats(None, None) == S.E_POINTER
    assert L.sealhip_pool_stats(h, None) == S.E_POINTER
    assert L.sealhip_memcpy_d2d(None, buf.ctypes.data, buf.ctypes.data, 8) == S.E_POINTER
    assert L.sealhip_memcpy_d2d(h, None, buf.ctypes.data, 8) == S.E_POINTER
    assert L.sealhip_memcpy_d2d(h, buf.ctypes.data, None, 8) == S.E_POINTER
    assert L.sealhip_transparency_note(None, 0, buf.ctypes.data, 0, 1) == S.E_POINTER
    assert L.sealhip_transparency_note(h, 0, None, 0, 1) == S.E_POINTER
    # then E_INVALIDARG
    assert L.sealhip_pool_alloc(h, 0, C.byref(p)) == S.E_INVALIDARG and p.value is None
    assert L.sealhip_pool_alloc(h, (1 << 46) + 1, C.byref(p)) == S.E_INVALIDARG
    assert L.sealhip_pool_release(h, buf.ctypes.data) == S.E_INVALIDARG  # never handed out
    assert "not handed out" in err()
    for k, size in ((0, 2), (4, 2), (1, 0), (1, 17)):
        assert L.sealhip_transparency_note(h, k, buf.ctypes.data, size, 1) == S.E_INVALIDARG, (k, size)
    # then the host-only context
    assert L.sealhip_pool_alloc(h, 8, C.byref(p)) == S.COR_E_INVALIDOPERATION and "host-only" in err()
    assert L.sealhip_pool_trim(h) == S.COR_E_INVALIDOPERATION
    assert L.sealhip_memcpy_d2d(h, buf.ctypes.data, buf.ctypes.data, 8) == S.COR_E_INVALIDOPERATION
    assert L.sealhip_transparency_note(h, 1, buf.ctypes.data, 2, 1) == S.COR_E_INVALIDOPERATION
    # the counters are introspection: zeros, no device needed
    assert ctx.pool_stats() == {"bytes_in_use": 0, "bytes_cached": 0, "device_mallocs": 0, "device_frees": 0, "hits": 0,
                                "misses": 0, "cross_lane_hits": 0}


def test_cpp_resident_check_builds_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_resident_check.cpp", link_sealhip=True, opt="-O1")
    assert "host-only resident checks ok" in run_exe(exe, timeout=120)
