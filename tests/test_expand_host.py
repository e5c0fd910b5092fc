"""Oblivious expansion and the sums against plaintext rows (sealhip_evaluator_expand / _dot_plain,
sealhip_expand_galois_elts): what can be checked without a GPU. The restatement of
tests/expand_ref.py against the definition (the keyless tree on plaintext polynomials against the closed form, decryption
under real keys), the element list, the argument checks of the entries on host-only contexts in the header's order, and the
128-bit capacity of the sum kernel's accumulators (tests/dot_plain_bounds_check.cpp)."""
import ctypes as C
import os

import numpy as np
import pytest

import expand_ref as X
import oracle_lib as O
import ring_pack_ref as R
from support import compile_cpp, rows, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_expand_galois_elts", "sealhip_evaluator_expand", "sealhip_evaluator_dot_plain")
LOGN, N = 4, 16
CASES_16 = {"bfv": (1, [30, 35, 40, 45, 50], 1, 65537), "ckks": (2, [40] * 5 + [41] * 2, 2, 0)}


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS and name in header
    for name in ("expand", "dot_plain"):
        assert callable(getattr(S.Evaluator, name))
    assert callable(S.Context.expand_galois_elts)


@pytest.mark.parametrize("logn", [1, 2, 3, 4, 6])
def test_keyless_tree_against_the_closed_form(logn):
    """output i is n sum_u m[i + n u] X^(n u), for every l and a full random polynomial"""
    q = (1 << 40) - 87
    big_n = 1 << logn
    rng = np.random.default_rng(logn)
    poly = [int(v) for v in rng.integers(0, q, size=big_n)]
    for l in range(logn + 1):
        n = 1 << l
        out = X.expand_keyless(poly, logn, n, q)
        assert len(out) == n
        for i in range(n):
            assert out[i] == X.closed_form(poly, logn, n, q, i), (logn, l, i)


def test_keyless_pack_then_expand():
    """pack_keyless of N constants v_j, then the expansion into N: output j is the constant N^2 v_j"""
    q = (1 << 40) - 87
    rng = np.random.default_rng(28)
    vs = [int(v) for v in rng.integers(0, q, size=N)]
    packed = R.pack_keyless(vs, LOGN, q)
    out = X.expand_keyless(packed, LOGN, N, q)
    for j in range(N):
        assert out[j] == [N * N * vs[j] % q] + [0] * (N - 1), j


def test_element_list():
    import sealhip as S

    mods = O.coeff_modulus_create(1 << 8, [30, 40, 50])
    ctx = S.Context(S.SCHEME_CKKS, 8, mods, 1, 0, device=-1)
    for l in range(9):
        want = sorted((256 >> (t - 1)) + 1 for t in range(1, l + 1))
        assert ctx.expand_galois_elts(1 << l) == want == X.galois_elts(8, 1 << l)
    assert ctx.expand_galois_elts(256) == [3, 5, 9, 17, 33, 65, 129, 257]
    assert ctx.expand_galois_elts(2) == [257]  # N + 1
    L = S.lib()
    cnt = C.c_uint32(77)
    buf = (C.c_uint32 * 8)()
    with pytest.raises(TypeError):
        S._check(L.sealhip_expand_galois_elts(None, 4, buf, 8, C.byref(cnt)))
    with pytest.raises(TypeError):
        S._check(L.sealhip_expand_galois_elts(ctx.handle, 4, buf, 8, None))
    for bad in (0, 3, 6, 512):
        with pytest.raises(ValueError, match="power of two"):
            S._check(L.sealhip_expand_galois_elts(ctx.handle, bad, buf, 8, C.byref(cnt)))
    with pytest.raises(ValueError, match="capacity"):
        S._check(L.sealhip_expand_galois_elts(ctx.handle, 16, buf, 3, C.byref(cnt)))
    assert cnt.value == 4
    assert L.sealhip_expand_galois_elts(ctx.handle, 16, None, 0, C.byref(cnt)) == 0 and cnt.value == 4


def _session(name, seed):
    scheme, bits, nsp, t = CASES_16[name]
    mods = O.coeff_modulus_create(N, bits)
    ref = O.RefContext(scheme, LOGN, mods, nsp=nsp, t=t, mode=1)
    cl = O.Client(ref, seed=seed)
    keys = {g: cl.galois_key(g) for g in X.galois_elts(LOGN, N)}
    return mods, ref, cl, keys


@pytest.mark.parametrize("n", [1, 2, 4, 16])
def test_restatement_decrypts_bfv_strict(n):
    """expand(ct, n, normalize) of a full message: output i decrypts to exactly sum_u m[i + n u] X^(n u), which is the
    constant m[i] when the message lives in the coefficients below n (both are checked)"""
    t = CASES_16["bfv"][3]
    mods, ref, cl, keys = _session("bfv", 3)
    rng = np.random.default_rng(n)
    full = rng.integers(0, t, size=N, dtype=np.uint64)
    low = full.copy()
    low[n:] = 0
    for m in (full, low):
        out = X.expand(ref, mods, cl.k, cl.encrypt_bfv(m), keys, n, normalize=True)
        for i in range(n):
            want = np.zeros(N, dtype=np.uint64)
            want[::n] = m[i::n]
            assert np.array_equal(cl.decrypt_bfv(out[i]), want), (n, i)
    assert np.array_equal(cl.decrypt_bfv(out[n - 1]), np.array([low[n - 1]] + [0] * (N - 1), dtype=np.uint64))


def ckks_rel_error(cl, msg, outs, n):
    """the largest error of the outputs' phases against sum_u m[i + n u] X^(n u), relative to the largest |m|"""
    worst = 0
    for i in range(n):
        want = [0] * N
        want[::n] = msg[i::n]
        got = R.ckks_phase(cl, outs[i])
        worst = max(worst, max(abs(a - b) for a, b in zip(got, want)))
    return worst / max(abs(v) for v in msg)


@pytest.mark.parametrize("n", [1, 2, 4, 16])
def test_restatement_decrypts_ckks(n):
    """scale 2^40, the moduli of CASES_16: the same within X.CKKS_REL_BOUND of the largest message coefficient; the
    measured error must itself stay within X.CKKS_REL_MEASURED, the number the bound was derived from"""
    mods, ref, cl, keys = _session("ckks", 5)
    rng = np.random.default_rng(40 + n)
    msg = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
    out = X.expand(ref, mods, cl.k, cl.encrypt_poly_ntt(msg), keys, n, normalize=True)
    rel = ckks_rel_error(cl, msg, out, n)
    print("ckks restatement n=%d: relative error 2^%.1f" % (n, np.log2(rel) if rel else -np.inf))
    assert rel <= X.CKKS_REL_MEASURED, (n, rel)
    assert X.CKKS_REL_BOUND == X.CKKS_REL_MEASURED * 2.0 ** 10


def test_dot_plain_restatements_agree():
    """multiply_plain_ntt + add left to right is the canonical residue of the integer sum, random and all p - 1"""
    mods = O.coeff_modulus_create(8, [61, 20, 45, 61])
    ref = O.RefContext(2, 3, mods, nsp=1, mode=1)
    k = 3
    rng = np.random.default_rng(9)
    for n_terms, n_sums, size, count in ((1, 1, 2, 1), (17, 2, 3, 2)):
        cts = rows(rng, mods[:k], 8, (count, n_terms, size))
        plain = rows(rng, mods[:k], 8, (n_sums, n_terms))
        assert np.array_equal(X.dot_plain(ref, k, cts, plain), X.dot_plain_int(mods, cts, plain))
    cts = np.stack([np.full((1, 33, 2, 8), p - 1, dtype=np.uint64) for p in mods[:k]], axis=3)
    plain = np.stack([np.full((1, 33, 8), p - 1, dtype=np.uint64) for p in mods[:k]], axis=2)
    assert np.array_equal(X.dot_plain(ref, k, cts, plain), X.dot_plain_int(mods, cts, plain))


def test_entries_on_host_only_context():
    """the header's order: E_POINTER; then the E_INVALIDARG checks, which hold for an empty call too; then the empty call
    (S_OK); then the host-only context (COR_E_INVALIDOPERATION). A key handle cannot exist without a device, so the checks
    that look at a present key (its digits) and the device-side refusals are in tests/test_gpu_expand.py."""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    parity = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, device=-1)
    strict = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    L = S.lib()
    big = np.zeros(1 << 16, dtype=np.uint64)
    base = big.ctypes.data
    base += (-base) % 16
    ct, out, plain = base, base + (1 << 15), base + (1 << 18)  # disjoint for count = 1, k = 2, n = 1
    three = (C.c_uint32 * 1)(3)
    nokey = (C.c_void_p * 1)(None)

    def exp(h, k=2, ct=ct, count=1, n=1, elts=None, keys=None, n_keys=0, normalize=0, o=out):
        return L.sealhip_evaluator_expand(h, k, ct, count, n, elts, keys, n_keys, normalize, o)

    def dot(h, k=2, cts=ct, n_terms=1, size=2, count=1, pl=plain, n_sums=1, o=out):
        return L.sealhip_evaluator_dot_plain(h, k, cts, n_terms, size, count, pl, n_sums, o)

    ok = (strict.handle, ckks.handle)
    every = ok + (parity.handle,)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG)
    for h in every:
        for kw in ({"ct": None}, {"o": None}, {"n_keys": 1, "keys": nokey}, {"n_keys": 1, "elts": three},
                   {"n_keys": 1, "elts": three, "keys": nokey}):
            with pytest.raises(TypeError):
                S._check(exp(h, k=9, **kw))
        for kw in ({"cts": None}, {"pl": None}, {"o": None}):
            with pytest.raises(TypeError):
                S._check(dot(h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(exp(None))
    with pytest.raises(TypeError):
        S._check(dot(None))
    # 2. invalid arguments, also for an empty call, in the documented order (each call also breaks every LATER rule)
    for h in ok:
        for count in (1, 0):
            for k in (0, 3, 4):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(exp(h, k=k, count=count, n=3))
            for bad in (0, 3, 12, 512):
                with pytest.raises(ValueError, match="power of two"):
                    S._check(exp(h, count=count, n=bad, o=out + 8))
            with pytest.raises(ValueError, match="Galois key not present"):
                S._check(exp(h, count=count, n=2, o=out + 8))
            with pytest.raises(ValueError, match="16-byte aligned"):
                S._check(exp(h, count=count, o=ct + 8))
            with pytest.raises(ValueError, match="16-byte aligned"):
                S._check(exp(h, count=count, ct=ct + 8, o=ct))
        with pytest.raises(ValueError, match="overlap"):
            S._check(exp(h, o=ct))
        with pytest.raises(ValueError, match="overlap"):
            S._check(exp(h, o=ct + 16 * 100))
    for count in (1, 0):
        with pytest.raises(ValueError, match="power of two"):  # (n comes before the mode)
            S._check(exp(parity.handle, count=count, n=3))
        with pytest.raises(ValueError, match="STRICT"):        # (... and the mode before the keys)
            S._check(exp(parity.handle, count=count, n=2, o=out + 8))
    for h in every:
        for count in (1, 0):
            for k in (0, 3, 4):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(dot(h, k=k, count=count, size=1))
            for size in (0, 1, 17):
                with pytest.raises(ValueError, match="encrypted is not valid"):
                    S._check(dot(h, count=count, size=size, o=out + 8))
            with pytest.raises(ValueError, match="16-byte aligned"):
                S._check(dot(h, count=count, o=ct + 8))
            with pytest.raises(ValueError, match="16-byte aligned"):
                S._check(dot(h, count=count, pl=plain + 8, o=ct))
        for kw in ({"n_terms": 0}, {"n_sums": 0}):
            with pytest.raises(ValueError, match="must not be empty"):
                S._check(dot(h, o=out + 8, **kw))
        with pytest.raises(ValueError, match="overlap cts"):
            S._check(dot(h, o=ct))
        with pytest.raises(ValueError, match="overlap cts"):
            S._check(dot(h, n_terms=2, o=ct + 8 * 2 * 2 * n))  # (the second term)
        with pytest.raises(ValueError, match="overlap plain"):
            S._check(dot(h, o=plain))
    # 3. nothing to do: S_OK, no device needed
    for h in ok:
        assert exp(h, count=0) == 0
    for h in every:
        assert dot(h, count=0) == 0 and dot(h, count=0, n_terms=0, n_sums=0) == 0
    # 4. a valid call with work to do is refused as host-only
    for h in ok:
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(exp(h))
    for h in every:
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(dot(h))


def test_bounds_check_program(tmp_path):
    exe = compile_cpp(tmp_path, "dot_plain_bounds_check.cpp")
    assert "dot_plain_bounds_check: OK" in run_exe(exe, timeout=120)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_expand_check.cpp", link_sealhip=True)
    assert "host-only expand checks ok" in run_exe(exe, "host", timeout=120)
