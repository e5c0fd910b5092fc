"""Key generation on the device (sealhip_generate_relin_keys, sealhip_generate_galois_keys, sealhip_kswitch_keys_save_seeded):
what can be checked without a GPU. The argument checks of the new entries on a host-only context, in the order E_POINTER,
E_INVALIDARG, COR_E_INVALIDOPERATION; the Python mirrors; and the C++ KeyGenerator's host checks with the reference's
messages (keygenerator.cpp:146-240)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from support import compile_cpp, run_exe

NEW = ("sealhip_generate_relin_keys", "sealhip_generate_galois_keys", "sealhip_kswitch_keys_save_seeded")


def _host_ctx(S, t=786433, scheme=None, logn=8):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    scheme = S.SCHEME_BFV if scheme is None else scheme
    return S.Context(scheme, logn, mods, 2, t if scheme == S.SCHEME_BFV else 0, device=-1), n


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("generate_relin_keys", "generate_galois_keys"):
        assert callable(getattr(S.Context, name))
    assert callable(S.save_kswitch_keys_seeded)


def test_generate_checks_on_host_only_context():
    import sealhip as S

    ctx, n = _host_ctx(S)
    L = S.lib()
    seeds = np.zeros((4, 2, 8), dtype=np.uint64)
    noise = np.zeros((4, 2, n), dtype=np.int32)
    sp, npp = seeds.ctypes.data, noise.ctypes.data
    sk = np.zeros((4, n), dtype=np.uint64).ctypes.data

    def galois(elts, ctx_h=ctx.handle, sk_p=sk, elts_p=True, seeds_p=sp, noise_p=npp, out=None):
        arr = (C.c_uint32 * max(1, len(elts)))(*elts)
        out = out if out is not None else (C.c_void_p * max(1, len(elts)))()
        return out, L.sealhip_generate_galois_keys(ctx_h, sk_p, arr if elts_p else None, len(elts), seeds_p, noise_p, 0, out)

    # null pointers first, before anything else is looked at (also with otherwise invalid elements)
    for kw in ({"ctx_h": None}, {"sk_p": None}, {"elts_p": False}, {"seeds_p": None}, {"noise_p": None}):
        with pytest.raises(TypeError):
            S._check(galois([4, 3], **kw)[1])
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_relin_keys(ctx.handle, sk, 1, sp, npp, 0, None))
    with pytest.raises(TypeError):
        S._check(L.sealhip_kswitch_keys_save_seeded(ctx.handle, None, 1, None, 0, C.byref(C.c_size_t(0))))
    # invalid elements: E_INVALIDARG, every output NULL
    for bad in ([3, 4], [2 * n + 1], [2 * n], [0], [3, 5, 3]):
        out = (C.c_void_p * len(bad))(*([7] * len(bad)))
        with pytest.raises(ValueError):
            S._check(galois(bad, out=out)[1])
        assert all(v is None for v in out)
    with pytest.raises(ValueError, match="Galois element is not valid"):
        S._check(galois([3, 6])[1])
    with pytest.raises(ValueError, match="distinct"):
        S._check(galois([3, 5, 3])[1])
    with pytest.raises(ValueError, match="invalid count"):
        S._check(L.sealhip_generate_relin_keys(ctx.handle, sk, 15, sp, npp, 0, (C.c_void_p * 15)()))
    # no batching: COR_E_INVALIDOPERATION, after the element checks
    ctx_nb, _ = _host_ctx(S, t=65539)
    with pytest.raises(ValueError):
        S._check(galois([4], ctx_h=ctx_nb.handle)[1])
    with pytest.raises(S.LogicError, match="batching"):
        S._check(galois([3], ctx_h=ctx_nb.handle)[1])
    # CKKS always batches, and relin keys need no batching: valid arguments (empty lists included) reach the device
    ctx_ckks, _ = _host_ctx(S, scheme=S.SCHEME_CKKS)
    for h in (ctx.handle, ctx_ckks.handle):
        for elts in ([3, 2 * n - 1], []):
            out, hr = galois(elts, ctx_h=h)
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(hr)
            assert all(v is None for v in out)
    for count in (1, 0):
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(L.sealhip_generate_relin_keys(ctx_nb.handle, sk, count, sp, npp, 0, (C.c_void_p * 1)()))
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(L.sealhip_kswitch_keys_save_seeded(ctx.handle, None, 0, None, 0, C.byref(C.c_size_t(0))))


def test_no_context_without_key_switching():
    """using_keyswitching (context.cpp:495) is false only for a single prime, which sealhip_context_create refuses: every
    context the generators see uses key switching"""
    import sealhip as S

    with pytest.raises(ValueError):
        S.Context(S.SCHEME_BFV, 8, O.coeff_modulus_create(256, [40]), 1, 786433, device=-1)


# ------------------------------------------------------------------ the C++ adapter
def build_keygen_adapter(tmp_path):
    return compile_cpp(tmp_path, "host_adapter_keygen_check.cpp", link_sealhip=True)


def test_cpp_keygenerator_checks_on_host_only_context(tmp_path):
    """relin_keys: "invalid count"; galois_keys: "Galois element is not valid", "step count too large" (invalid_argument) and
    "encryption parameters do not support batching" (logic_error) before any sample is drawn; get_elts_all's list; duplicate
    elements draw no samples; a valid call is refused by the host-only context"""
    assert "host-only keygen checks ok" in run_exe(build_keygen_adapter(tmp_path), timeout=120)
