"""Decryptor on the device (sealhip_decryptor_invariant_noise_budget, sealhip_decryptor_decrypt): what can be checked
without a GPU. The exports and their Python mirrors; the restatement of invariant_noise_budget (tests/noise_ref.py) against
planted budgets and, on oracle-only ciphertexts, against the semantics the reference promises; the C++ Decryptor's host
checks; and the argument checks of both entries on host-only contexts."""
import ctypes as C

import numpy as np
import pytest

import noise_ref as R
import oracle_lib as O
from support import compile_cpp, run_exe

NEW = ("sealhip_decryptor_invariant_noise_budget", "sealhip_decryptor_decrypt")


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("invariant_noise_budget", "decrypt"):
        assert callable(getattr(S.Context, name))


@pytest.mark.parametrize("t", [786433, 1 << 20])
@pytest.mark.parametrize("logn,bits", [(6, [40, 50]), (8, [60, 60, 55]), (5, [30])])
def test_restatement_agrees_with_planted(t, logn, bits):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits)
    q = R.prod(mods)
    rng = np.random.default_rng(logn * 7 + len(bits))
    half = (q - 1) // 2
    cases = [
        (np.zeros(n, np.int64), {}),                                       # zero polynomial: bits(Q) - 1
        (rng.integers(-1000, 1000, size=n), {}),
        (rng.integers(-(1 << 20), 1 << 20, size=n), {0: half}),            # W = (Q - 1) / 2
        (np.zeros(n, np.int64), {n - 1: -half}),                           # W = (Q + 1) / 2
        (np.zeros(n, np.int64), {3 % n: -1}),                              # W = Q - 1: norm 1
        (rng.integers(-5, 5, size=n), {n // 2: 1 << (q.bit_length() // 2)}),
    ]
    for x, big in cases:
        rows = R.planted_rows(x, big, mods, t)
        assert R.ref_noise_budget(rows, mods, t) == R.planted_budget(x, big, mods)
    assert R.planted_budget(np.zeros(n, np.int64), {}, mods) == q.bit_length() - 1
    assert R.planted_budget(np.zeros(n, np.int64), {0: half}, mods) == max(0, q.bit_length() - half.bit_length() - 1)


def _bfv_session(logn, bits, t, mode=1):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=mode)
    return ref, O.Client(ref, seed=11), n


def _budget(cl, ct):
    k, size = ct.shape[1], ct.shape[0]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    pw = cl.sk_powers(size - 1)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), size, 0, O.ptr(pw), O.ptr(dot))
    return R.ref_noise_budget(dot, cl.mods[:k], cl.ref.t)


def test_semantics_fresh_and_multiply_chain():
    """a fresh encryption of a plaintext with zero coefficients has a budget in 1 .. bits(Q) - bits(t); along a STRICT
    multiply + relinearize chain the budget does not increase, and while it is above 0 the plaintext arithmetic decrypts"""
    t = 786433
    ref, cl, n = _bfv_session(8, [50, 50, 50, 60], t)
    L = O.lib()
    k = cl.k
    q = R.prod(cl.mods[:k])
    rng = np.random.default_rng(5)
    m = rng.integers(0, t, size=n, dtype=np.uint64)
    m[::3] = 0
    ct = cl.encrypt_bfv(m)
    b0 = _budget(cl, ct)
    assert 1 <= b0 <= q.bit_length() - t.bit_length()
    assert np.array_equal(cl.decrypt_bfv(ct), m)
    rk = cl.relin_key()
    keys = (C.c_void_p * 1)(rk.ctypes.data)
    factor = rng.integers(0, 4, size=n, dtype=np.uint64)
    fct = cl.encrypt_bfv(factor)
    prev, expect, budgets = b0, m, [b0]
    for _ in range(4):
        out = np.zeros((3, k, n), dtype=np.uint64)
        assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(ct), 2, O.ptr(fct), 2, O.ptr(out)) == 0
        assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(out), 3, keys) == 0
        ct = np.ascontiguousarray(out[:2])
        expect = O.negacyclic_mod_t(expect, factor, t)
        b = _budget(cl, ct)
        budgets.append(b)
        assert b <= prev, budgets
        if b > 0:
            assert np.array_equal(cl.decrypt_bfv(ct), expect), budgets
        prev = b
    assert budgets[-1] < budgets[0]


def test_semantics_size_three():
    """a size-3 product (before relinearization) has the budget of its relinearized form within a few bits"""
    t = 65537
    ref, cl, n = _bfv_session(8, [55, 55, 55, 60], t)
    k = cl.k
    rng = np.random.default_rng(6)
    a, b = (rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(2))
    out = np.zeros((3, k, n), dtype=np.uint64)
    assert O.lib().ref_bfv_multiply(C.byref(ref.c), k, O.ptr(cl.encrypt_bfv(a)), 2, O.ptr(cl.encrypt_bfv(b)), 2,
                                    O.ptr(out)) == 0
    b3 = _budget(cl, out)
    assert b3 > 0
    assert np.array_equal(cl.decrypt_bfv(out), O.negacyclic_mod_t(a, b, t))


def test_cpp_decryptor_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_decrypt_check.cpp", link_sealhip=True)
    assert "host-only decrypt checks ok" in run_exe(exe, timeout=120)


def test_entries_on_host_only_context():
    """E_POINTER first; then k / size (E_INVALIDARG), the scheme (COR_E_INVALIDOPERATION for a CKKS noise budget, E_INVALIDARG
    for the wrong form), then the host-only context (COR_E_INVALIDOPERATION), also for count = 0"""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    bfv = S.Context(S.SCHEME_BFV, 8, mods, 2, 786433, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    L = S.lib()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    b32 = np.zeros(4, dtype=np.int32).ctypes.data

    def nb(ctx, k=2, size=2, count=1, ct=p, sk=p, out=b32):
        return L.sealhip_decryptor_invariant_noise_budget(ctx, k, ct, size, count, sk, out)

    def dec(ctx, k=2, size=2, count=1, ct=p, sk=p, ntt=0, out=p):
        return L.sealhip_decryptor_decrypt(ctx, k, ct, size, count, sk, ntt, out)

    for kw in ({"ct": None}, {"sk": None}, {"out": None}):
        for h in (bfv.handle, ckks.handle):
            with pytest.raises(TypeError):
                S._check(nb(h, k=0, **kw))
            with pytest.raises(TypeError):
                S._check(dec(h, size=1, **kw))
    with pytest.raises(TypeError):
        S._check(nb(None))
    with pytest.raises(TypeError):
        S._check(dec(None))
    for h in (bfv.handle, ckks.handle):
        for kw in ({"k": 0}, {"k": 5}, {"size": 1}, {"size": 17}, {"size": 0}):
            with pytest.raises(ValueError):
                S._check(dec(h, ntt=1 if h == ckks.handle else 0, **kw))
            with pytest.raises(ValueError):
                S._check(nb(h, **kw))
    with pytest.raises(S.LogicError, match="unsupported scheme"):
        S._check(nb(ckks.handle))
    with pytest.raises(ValueError, match="cannot be in NTT form"):
        S._check(dec(bfv.handle, ntt=1))
    with pytest.raises(ValueError, match="must be in NTT form"):
        S._check(dec(ckks.handle, ntt=0))
    for count in (1, 0):
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(nb(bfv.handle, count=count))
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(dec(bfv.handle, count=count))
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(dec(ckks.handle, ntt=1, count=count))
    # k = n_key (the key level) is a valid level
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(nb(bfv.handle, k=4, size=16))
