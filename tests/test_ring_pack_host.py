"""Ring packing (sealhip_evaluator_extract_lwe / _pack_lwes, sealhip_pack_lwes_galois_elts): what can be
checked without a GPU. The restatement of tests/ring_pack_ref.py against the definitions (an O(N^2) negacyclic product, the
keyless tree on plaintext polynomials, decryption under real keys), the element list, and the argument checks of the three
entries on host-only contexts in the header's order."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import ring_pack_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_pack_lwes_galois_elts", "sealhip_evaluator_extract_lwe", "sealhip_evaluator_pack_lwes")
LOGN, N = 4, 16


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS and name in header
    for name in ("extract_lwe", "pack_lwes"):
        assert callable(getattr(S.Evaluator, name))
    assert callable(S.Context.pack_lwes_galois_elts)


def _negacyclic(a, b, p):
    n = len(a)
    out = [0] * n
    for i in range(n):
        for j in range(n):
            v = int(a[i]) * int(b[j])
            if i + j >= n:
                out[i + j - n] -= v
            else:
                out[i + j] += v
    return [v % p for v in out]


def test_sample_and_embedding_against_the_negacyclic_product():
    """for every j: b + <a, s> is coefficient j of c_0 + c_1 s, and the constant coefficient of the embedding's phase is
    w (b + <a, s>); on both sides of the sign split, with zeros planted so that -0 = 0 is met"""
    mods = [(1 << 30) - 35, 97]
    rng = np.random.default_rng(4)
    ct = np.stack([np.stack([rng.integers(0, p, size=N, dtype=np.uint64) for p in mods]) for _ in range(2)])
    ct[1, :, 3] = 0
    ct[1, :, N - 1] = 0
    s = rng.integers(-1, 2, size=N)
    w = [5, 11]
    for j in range(N):
        a, b = R.extract(ct, mods, j)
        emb = R.embed(a, b, mods, w)
        for r, p in enumerate(mods):
            sr = [int(v) % p for v in s]
            phase = [(int(x) + y) % p for x, y in zip(ct[0, r], _negacyclic(ct[1, r], sr, p))]
            lwe = (int(b[r]) + sum(int(x) * y for x, y in zip(a[r], sr))) % p
            assert lwe == phase[j], (j, r)
            emb_phase = [(int(x) + y) % p for x, y in zip(emb[0, r], _negacyclic(emb[1, r], sr, p))]
            assert emb_phase[0] == w[r] * lwe % p, (j, r)
            assert np.all(emb[0, r, 1:] == 0)
        assert np.all(a < np.array(mods, dtype=np.uint64)[:, None])


@pytest.mark.parametrize("trace", [False, True])
def test_keyless_pack_on_plaintext_polynomials(trace):
    """n m_j at coefficient (N / n) j for every l; with the trace N m_j there and zeros elsewhere -- also when the inputs
    are full polynomials whose other coefficients are junk"""
    q = (1 << 40) - 87
    rng = np.random.default_rng(8)
    for l in range(LOGN + 1):
        n = 1 << l
        ms = [int(v) for v in rng.integers(0, q, size=n)]
        out = R.pack_keyless(ms, LOGN, q, trace)
        polys = [[m] + [int(v) for v in rng.integers(0, q, size=N - 1)] for m in ms]
        junk = R.pack_keyless_polys(polys, LOGN, q, trace)
        factor = N if trace else n
        for j in range(n):
            assert out[(N // n) * j] == factor * ms[j] % q, (l, j)
            assert junk[(N // n) * j] == factor * ms[j] % q, (l, j)
        if trace:
            rest = [c for c in range(N) if c % (N // n)]
            assert all(out[c] == 0 and junk[c] == 0 for c in rest), l


def test_element_list():
    import sealhip as S

    mods = O.coeff_modulus_create(1 << 8, [30, 40, 50])
    ctx = S.Context(S.SCHEME_CKKS, 8, mods, 1, 0, device=-1)
    for l in range(9):
        for trace in (False, True):
            want = [(1 << t) + 1 for t in range(1, (8 if trace else l) + 1)]
            assert ctx.pack_lwes_galois_elts(1 << l, trace) == want == R.galois_elts(8, 1 << l, trace)
    assert ctx.pack_lwes_galois_elts(256, True)[-1] == 257  # N + 1
    L = S.lib()
    cnt = C.c_uint32(77)
    buf = (C.c_uint32 * 8)()
    with pytest.raises(TypeError):
        S._check(L.sealhip_pack_lwes_galois_elts(None, 4, 0, buf, 8, C.byref(cnt)))
    with pytest.raises(TypeError):
        S._check(L.sealhip_pack_lwes_galois_elts(ctx.handle, 4, 0, buf, 8, None))
    for bad in (0, 3, 6, 512):
        with pytest.raises(ValueError, match="power of two"):
            S._check(L.sealhip_pack_lwes_galois_elts(ctx.handle, bad, 0, buf, 8, C.byref(cnt)))
    with pytest.raises(ValueError, match="capacity"):
        S._check(L.sealhip_pack_lwes_galois_elts(ctx.handle, 16, 0, buf, 3, C.byref(cnt)))
    assert cnt.value == 4
    assert L.sealhip_pack_lwes_galois_elts(ctx.handle, 16, 0, None, 0, C.byref(cnt)) == 0 and cnt.value == 4


def _session(scheme, bits, nsp, t, seed):
    mods = O.coeff_modulus_create(N, bits)
    ref = O.RefContext(scheme, LOGN, mods, nsp=nsp, t=t, mode=1)
    cl = O.Client(ref, seed=seed)
    keys = {g: cl.galois_key(g) for g in R.galois_elts(LOGN, N, True)}
    return mods, ref, cl, keys


@pytest.mark.parametrize("n", [1, 2, 4, 16])
def test_restatement_decrypts_bfv_strict(n):
    """pack(extract(ct, idx), normalize, trace) decrypts to exactly m[idx[j]] at (N / n) j and 0 elsewhere"""
    t = 257
    mods, ref, cl, keys = _session(1, [40, 40, 41], 1, t, 3)
    rng = np.random.default_rng(n)
    m = rng.integers(0, t, size=N, dtype=np.uint64)
    ct = cl.encrypt_bfv(m)[None]
    idx = [int(v) for v in rng.permutation(N)[:n]]
    la, lb = R.extract_samples(ref, mods, ct, idx)
    out = R.pack(ref, mods, cl.k, la[0], lb[0], keys, trace=True, normalize=True)
    want = np.zeros(N, dtype=np.uint64)
    for j, i in enumerate(idx):
        want[(N // n) * j] = m[i]
    assert np.array_equal(cl.decrypt_bfv(out), want), (n, idx)
    if n > 1:  # without the trace the packed positions alone are defined
        part = R.pack(ref, mods, cl.k, la[0], lb[0], keys, trace=False, normalize=True)
        assert np.array_equal(cl.decrypt_bfv(part)[:: N // n], want[:: N // n])


@pytest.mark.parametrize("n", [1, 2, 4, 16])
def test_restatement_decrypts_ckks(n):
    """scale 2^40, 50-bit primes: the same within R.CKKS_REL_BOUND of the largest message coefficient"""
    mods, ref, cl, keys = _session(2, [50, 50, 51, 51], 2, 0, 5)
    rng = np.random.default_rng(40 + n)
    msg = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
    ct = cl.encrypt_poly_ntt(msg)[None]
    idx = [int(v) for v in rng.permutation(N)[:n]]
    la, lb = R.extract_samples(ref, mods, ct, idx)
    out = R.pack(ref, mods, cl.k, la[0], lb[0], keys, trace=True, normalize=True)
    want = [0] * N
    for j, i in enumerate(idx):
        want[(N // n) * j] = msg[i]
    got = R.ckks_phase(cl, out)
    rel = max(abs(a - b) for a, b in zip(got, want)) / max(abs(v) for v in msg)
    print("ckks restatement n=%d: relative error 2^%.1f" % (n, np.log2(rel) if rel else -np.inf))
    assert rel <= R.CKKS_REL_BOUND, (n, rel)


def test_entries_on_host_only_context():
    """the header's order: E_POINTER; then the E_INVALIDARG checks, which hold for an empty call too; then the empty call
    (S_OK); then the host-only context (COR_E_INVALIDOPERATION). A key handle cannot exist without a device, so the checks
    that look at a present key (its digits) and the device-side refusals are in tests/test_gpu_ring_pack.py."""
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
    ct, la, lb, out = base, base + (1 << 15), base + (1 << 17), base + (1 << 18)  # disjoint for count = 1, k = 2
    idx = (C.c_uint32 * 3)(0, 255, 7)
    bad_idx = (C.c_uint32 * 3)(0, 256, 7)
    three = (C.c_uint32 * 1)(3)
    nokey = (C.c_void_p * 1)(None)

    def ext(h, k=2, ct=ct, count=1, indices=idx, n_idx=3, a=la, b=lb):
        return L.sealhip_evaluator_extract_lwe(h, k, ct, count, indices, n_idx, a, b)

    def pack(h, k=2, a=la, b=lb, n=1, count=1, elts=None, keys=None, n_keys=0, trace=0, normalize=0, o=out):
        return L.sealhip_evaluator_pack_lwes(h, k, a, b, n, count, elts, keys, n_keys, trace, normalize, o)

    ok = (strict.handle, ckks.handle)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG)
    for h in ok + (parity.handle,):
        for kw in ({"ct": None}, {"a": None}, {"b": None}, {"indices": None}):
            with pytest.raises(TypeError):
                S._check(ext(h, k=9, **kw))
        for kw in ({"a": None}, {"b": None}, {"o": None}, {"n_keys": 1, "keys": nokey}, {"n_keys": 1, "elts": three},
                   {"n_keys": 1, "elts": three, "keys": nokey}):
            with pytest.raises(TypeError):
                S._check(pack(h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(ext(None))
    with pytest.raises(TypeError):
        S._check(pack(None))
    assert ext(strict.handle, indices=None, n_idx=0) == 0  # (no indices, none needed)
    # 2. invalid arguments, also for an empty call, in the documented order (each call also breaks every LATER rule)
    for h in ok + (parity.handle,):
        for count in (1, 0):
            for k in (0, 3, 4):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(ext(h, k=k, count=count, indices=bad_idx, a=la + 8))
            with pytest.raises(ValueError, match="index out of range"):
                S._check(ext(h, count=count, indices=bad_idx, a=la + 8))
            with pytest.raises(ValueError, match="16-byte aligned"):
                S._check(ext(h, count=count, a=ct + 8))
        with pytest.raises(ValueError, match="overlap"):
            S._check(ext(h, a=ct))
        with pytest.raises(ValueError, match="overlap"):
            S._check(ext(h, b=ct + 8 * 100))
        with pytest.raises(ValueError, match="overlap"):
            S._check(ext(h, b=la + 16))
    for h in ok:
        for count in (1, 0):
            for k in (0, 3, 4):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(pack(h, k=k, count=count, n=3))
            for bad in (0, 3, 12, 512):
                with pytest.raises(ValueError, match="power of two"):
                    S._check(pack(h, count=count, n=bad, o=out + 8))
            with pytest.raises(ValueError, match="Galois key not present"):
                S._check(pack(h, count=count, n=2, o=out + 8))
            with pytest.raises(ValueError, match="Galois key not present"):
                S._check(pack(h, count=count, n=1, trace=1, o=out + 8))
            with pytest.raises(ValueError, match="16-byte aligned"):
                S._check(pack(h, count=count, o=out + 8))
            with pytest.raises(ValueError, match="16-byte aligned"):
                S._check(pack(h, count=count, a=la + 8, o=la))
        with pytest.raises(ValueError, match="overlap"):
            S._check(pack(h, o=la))
        with pytest.raises(ValueError, match="overlap"):
            S._check(pack(h, o=lb))
    for count in (1, 0):
        with pytest.raises(ValueError, match="power of two"):  # (n comes before the mode)
            S._check(pack(parity.handle, count=count, n=3))
        with pytest.raises(ValueError, match="STRICT"):        # (... and the mode before the keys)
            S._check(pack(parity.handle, count=count, n=2, o=out + 8))
    # 3. nothing to do: S_OK, no device needed
    for h in ok + (parity.handle,):
        assert ext(h, count=0) == 0 and ext(h, n_idx=0) == 0
    for h in ok:
        assert pack(h, count=0) == 0
    # 4. a valid call with work to do is refused as host-only
    for h in ok + (parity.handle,):
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(ext(h))
    for h in ok:
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(pack(h))


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    from support import compile_cpp, run_exe

    exe = compile_cpp(tmp_path, "host_adapter_ring_pack_check.cpp", link_sealhip=True)
    assert "host-only ring pack checks ok" in run_exe(exe, "host", timeout=120)
