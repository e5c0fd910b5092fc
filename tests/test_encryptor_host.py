"""Encryptor on the device (sealhip_encryptor_encrypt, sealhip_encryptor_encrypt_symmetric, sealhip_ciphertext_save_seeded):
what can be checked without a GPU. The exports and their Python mirrors; the argument checks of every new entry on host-only
contexts; the C++ Encryptor's host checks; and, on the oracle alone, the level rule of encrypt_zero_internal
(encryptor.cpp:141-176): with nsp special primes the zero encryption runs over the k_first + 1 primes of the previous level,
not over the n_key key primes."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from support import compile_cpp, run_exe

NEW = ("sealhip_encryptor_encrypt", "sealhip_encryptor_encrypt_symmetric", "sealhip_ciphertext_save_seeded")
MODS = [1073738753, 1099511603713, 1152921504606830593, 1152921504606844417]


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("encrypt", "encrypt_symmetric", "save_seeded"):
        assert callable(getattr(S.Context, name))


def test_entries_on_host_only_context():
    """E_POINTER first, then E_INVALIDARG (level, plaintext level), then the host-only context (COR_E_INVALIDOPERATION)"""
    import sealhip as S

    L = S.lib()
    bfv = S.Context(S.SCHEME_BFV, 8, MODS, 2, 786433, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, MODS, 2, 0, device=-1)
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    seeds = np.zeros(8, dtype=np.uint64).ctypes.data
    err = lambda: L.sealhip_last_error_string().decode()
    for ctx in (bfv, ckks):
        h = ctx.handle
        enc = lambda k, pk=p, pl=None, u=p, e=p, ct=p, count=1: L.sealhip_encryptor_encrypt(h, k, pk, pl, 0, u, e, count, ct)
        sym = lambda k, sk=p, pl=None, sd=seeds, e=p, ct=p, count=1: L.sealhip_encryptor_encrypt_symmetric(
            h, k, sk, pl, 0, sd, e, 1, count, ct)
        # null pointers before anything else, even with an invalid level
        for kw in ({"pk": None}, {"u": None}, {"e": None}, {"ct": None}):
            assert enc(0, **kw) == S.E_POINTER
        for kw in ({"sk": None}, {"sd": None}, {"e": None}, {"ct": None}):
            assert sym(0, **kw) == S.E_POINTER
        assert L.sealhip_encryptor_encrypt(None, 2, p, None, 0, p, p, 1, p) == S.E_POINTER
        # the level, with or without a plaintext
        for bad in (0, 5):
            assert enc(bad) == S.E_INVALIDARG
            assert "parms_id is not valid for encryption parameters" in err()
            assert sym(bad) == S.E_INVALIDARG
            assert enc(bad, pl=p) == S.E_INVALIDARG
        # a plaintext at a level it cannot take: BFV only at the first level (2), CKKS not above it
        for bad in ((1, 3, 4) if ctx is bfv else (3, 4)):
            assert enc(bad, pl=p) == S.E_INVALIDARG
            assert "plain is not valid for encryption parameters" in err()
            assert sym(bad, pl=p) == S.E_INVALIDARG
        # valid arguments: the host-only context refuses them, count = 0 included
        for k in (1, 2, 3, 4):
            assert enc(k) == S.COR_E_INVALIDOPERATION and "host-only" in err()
            assert sym(k) == S.COR_E_INVALIDOPERATION
            assert enc(k, count=0) == S.COR_E_INVALIDOPERATION
        assert enc(2, pl=p) == S.COR_E_INVALIDOPERATION
        assert sym(2, pl=p) == S.COR_E_INVALIDOPERATION
        if ctx is ckks:
            assert enc(1, pl=p) == S.COR_E_INVALIDOPERATION


def test_seeded_save_on_host_only_context():
    import sealhip as S

    L = S.lib()
    ctx = S.Context(S.SCHEME_BFV, 8, MODS, 2, 786433, device=-1)
    pid = (9, 8, 7, 6)
    ctx.set_parms_id(2, pid)
    info = S.CiphertextInfo()
    for j in range(4):
        info.parms_id[j] = pid[j]
    info.is_ntt_form, info.size, info.coeff_modulus_size, info.poly_modulus_degree, info.scale = 0, 2, 2, 256, 1.0
    seed = np.zeros(8, dtype=np.uint64)
    src = np.zeros(4, dtype=np.uint64)
    need = C.c_size_t(0)
    h = ctx.handle
    assert L.sealhip_ciphertext_save_seeded(h, C.addressof(info), src.ctypes.data, None, None, 0, C.byref(need)) == S.E_POINTER
    assert L.sealhip_ciphertext_save_seeded(h, None, src.ctypes.data, seed.ctypes.data, None, 0, C.byref(need)) == S.E_POINTER
    # the size query needs no device: c_0 words plus the 64-byte seed
    assert L.sealhip_ciphertext_save_seeded(h, C.addressof(info), src.ctypes.data, seed.ctypes.data, None, 0,
                                            C.byref(need)) == S.S_OK
    plain_size = C.c_size_t(0)
    assert L.sealhip_ciphertext_save_size(h, 1, 2, C.byref(plain_size)) == S.S_OK
    assert need.value == plain_size.value + 64
    info.size = 3
    assert L.sealhip_ciphertext_save_seeded(h, C.addressof(info), src.ctypes.data, seed.ctypes.data, None, 0,
                                            C.byref(need)) == S.E_INVALIDARG
    info.size = 2
    buf = (C.c_char * 1)()
    assert L.sealhip_ciphertext_save_seeded(h, C.addressof(info), src.ctypes.data, seed.ctypes.data, C.addressof(buf), 1,
                                            C.byref(need)) == S.COR_E_INVALIDOPERATION


def test_cpp_encryptor_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_encrypt_check.cpp", link_sealhip=True, opt="-O1")
    assert "host-only encrypt checks ok" in run_exe(exe, timeout=120)


def _compose(ref, cl, pk, rows, k, u, e, plain):
    """encrypt_zero_asymmetric over `rows` key primes, divide and round by the last of them, the first k rows, + Delta m"""
    L, c, n = O.lib(), ref.c, ref.n
    big = np.zeros((2, rows, n), dtype=np.uint64)
    L.ref_encrypt_zero_asymmetric_given(C.byref(c), rows, O.ptr(np.ascontiguousarray(pk[:, :rows])), 0, u.ctypes.data,
                                        e.ctypes.data, O.ptr(big))
    tool = ref.rns_tool(rows)
    for j in range(2):
        L.ref_divide_and_round_q_last_inplace(tool, O.ptr(big[j]))
    ct = np.ascontiguousarray(big[:, :k])
    L.ref_multiply_add_plain_with_scaling_variant(C.byref(c), k, O.ptr(plain), 0, O.ptr(ct[0]))
    return ct


@pytest.mark.parametrize("nsp", [1, 2, 3])
def test_previous_level_rule_decrypts_on_oracle(nsp):
    """the previous level of the first level has k_first + 1 rows: that composition decrypts. Encrypting over the n_key
    rows and dividing by the last key prime (the documented mistake) also decrypts, since an encryption of zero stays one
    on a sub-base, but it gives other words than the reference once nsp > 1"""
    logn, t = 10, 786433
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [50, 50, 50] + [55] * nsp)
    ref = O.RefContext(1, logn, mods, nsp=nsp, t=t)
    cl = O.Client(ref, seed=5 + nsp)
    n_key, k = len(mods), len(mods) - nsp
    pk = np.zeros((2, n_key, n), dtype=np.uint64)
    O.lib().ref_encrypt_zero_symmetric(C.byref(ref.c), n_key, O.ptr(cl.sk), 1, C.byref(cl.state), O.ptr(pk))
    rng = np.random.default_rng(nsp)
    u = rng.integers(-1, 2, size=n, dtype=np.int32)
    e = rng.integers(-19, 20, size=(2, n), dtype=np.int32)
    plain = rng.integers(0, t, size=n, dtype=np.uint64)
    good = _compose(ref, cl, pk, k + 1, k, u, e, plain)
    assert np.array_equal(cl.decrypt_bfv(good, k), plain)
    wrong = _compose(ref, cl, pk, n_key, k, u, e, plain)
    if nsp == 1:
        assert np.array_equal(wrong, good)
    else:
        assert np.array_equal(cl.decrypt_bfv(wrong, k), plain)
        assert not np.array_equal(wrong, good)
