"""The key switch's mod-down merged with the CKKS rescale (the sealhip_evaluator_*_rescale entries): what
can be checked without a GPU. The exports and their mirrors; the argument checks on host-only contexts, in the header's
order; the CPU restatement (tests/ks_rescale_ref.py) itself: with acc = 0 it is ref_mod_switch_scale_to_next word for word,
its exact quotient agrees with Python's big integers, and it decrypts within the error of the composition it replaces; the
kernels' arithmetic executed on the CPU (tests/ks_rescale_bounds_check.cpp); the C++ adapter's checks."""
import ctypes as C
import os

import numpy as np
import pytest

import hoist_bsgs_ref as BS
import hoist_dot_ref as HD
import hoist_ref as H
import ks_rescale_ref as R
import oracle_lib as O
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_relinearize_rescale", "sealhip_evaluator_dot_product_rescale",
       "sealhip_evaluator_apply_galois_dot_plain_rescale", "sealhip_evaluator_rotate_vector_dot_plain_rescale",
       "sealhip_evaluator_apply_galois_bsgs_plain_rescale", "sealhip_evaluator_rotate_vector_bsgs_plain_rescale")
SETS = [([40, 40, 40, 41], 1), ([36] * 4 + [37] * 2, 2), ([36] * 5 + [37] * 3, 3)]


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS and name in header
        assert callable(getattr(S.Evaluator, name[len("sealhip_evaluator_"):]))
    adapter = open(os.path.join(ROOT, "gemini-seal_amd", "host", "evaluator.hpp")).read()
    for name in NEW:
        assert "void " + name[len("sealhip_evaluator_"):] + "(" in adapter  # (the step forms go through the element entries)


def test_entries_on_host_only_context():
    """E_POINTER first; then, in this order, a BFV context ("CKKS only"), the level (k < 2, k above the first level), size,
    stride and the unmerged entries' own errors (E_INVALIDARG), also for an empty batch; then the empty batch (S_OK); then the
    host-only context (COR_E_INVALIDOPERATION). A key handle cannot exist without a device, so the checks that look INTO a key
    and the overlap with real operands run in tests/test_gpu_ks_rescale.py."""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    bfv = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    strict = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, mode=S.MODE_STRICT, device=-1)
    L = S.lib()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    far = p + (1 << 40)  # (never dereferenced: an address that overlaps nothing)
    ident = (C.c_uint32 * 2)(1, 1)
    nokey = (C.c_void_p * 2)(None, None)
    fake = (C.c_void_p * 1)(p)
    step0 = (C.c_int32 * 2)(0, 0)
    step1 = (C.c_int32 * 2)(0, 1)
    terms = (C.c_void_p * 1)(p)

    def relin(ctx, k=2, ct=p, size=3, stride=None, count=1, keys=fake, n_keys=1, out=far):
        stride = 3 * k * n if stride is None else stride
        return L.sealhip_evaluator_relinearize_rescale(ctx, k, ct, size, stride, count, keys, n_keys, out)

    def dotp(ctx, k=2, a=terms, b=terms, n_terms=1, count=1, keys=fake, n_keys=1, out=far):
        return L.sealhip_evaluator_dot_product_rescale(ctx, k, a, b, n_terms, count, keys, n_keys, out)

    def dot(ctx, k=2, ct=p, count=1, elts=ident, keys=nokey, n_elts=2, plain=p, n_sums=1, out=far):
        return L.sealhip_evaluator_apply_galois_dot_plain_rescale(ctx, k, ct, count, elts, keys, n_elts, plain, n_sums, out)

    def rot(ctx, k=2, ct=p, count=1, steps=step0, n_steps=2, elts=None, keys=None, n_keys=0, plain=p, n_sums=1, out=far):
        return L.sealhip_evaluator_rotate_vector_dot_plain_rescale(ctx, k, ct, count, steps, n_steps, elts, keys, n_keys, plain,
                                                                   n_sums, out)

    def bsgs(ctx, k=2, ct=p, count=1, baby=ident, bkeys=nokey, n_baby=2, giant=ident, gkeys=nokey, n_giant=2, plain=p, out=far):
        return L.sealhip_evaluator_apply_galois_bsgs_plain_rescale(ctx, k, ct, count, baby, bkeys, n_baby, giant, gkeys, n_giant,
                                                                   plain, out)

    def rbsgs(ctx, k=2, ct=p, count=1, bs=step0, n_baby=2, gs=step0, n_giant=2, elts=None, keys=None, n_keys=0, plain=p,
              out=far):
        return L.sealhip_evaluator_rotate_vector_bsgs_plain_rescale(ctx, k, ct, count, bs, n_baby, gs, n_giant, elts, keys,
                                                                    n_keys, plain, out)

    entries = (relin, dotp, dot, rot, bsgs, rbsgs)
    ok = (ckks.handle, strict.handle)
    # 1. null pointers, before anything else (a BFV context and k = 9 would be E_INVALIDARG)
    for h in ok + (bfv.handle,):
        for fn in entries:
            with pytest.raises(TypeError):
                S._check(fn(h, k=9, out=None))
        for fn in (relin, dot, rot, bsgs, rbsgs):
            with pytest.raises(TypeError):
                S._check(fn(h, k=9, ct=None))
        for fn in (relin, dotp):
            with pytest.raises(TypeError):
                S._check(fn(h, k=9, keys=None, n_keys=0))  # (the merged entries need the key)
            with pytest.raises(TypeError):
                S._check(fn(h, k=9, keys=(C.c_void_p * 1)(None)))
        with pytest.raises(TypeError):
            S._check(dotp(h, k=9, a=None))
        with pytest.raises(TypeError):
            S._check(dotp(h, k=9, b=(C.c_void_p * 1)(None)))
        for fn in (dot, rot, bsgs, rbsgs):
            with pytest.raises(TypeError):
                S._check(fn(h, k=9, plain=None))
        with pytest.raises(TypeError):
            S._check(dot(h, k=9, elts=(C.c_uint32 * 2)(1, 3)))  # (a null key for an element other than 1)
        with pytest.raises(TypeError):
            S._check(bsgs(h, k=9, giant=(C.c_uint32 * 2)(1, 3)))
    for fn in entries:
        with pytest.raises(TypeError):
            S._check(fn(None))
    # 2. invalid arguments, also for an empty batch. BFV first, whatever else is wrong
    for fn in entries:
        for count in (1, 0):
            for k in (2, 9, 0):
                with pytest.raises(ValueError, match="CKKS only"):
                    S._check(fn(bfv.handle, k=k, count=count))
    with pytest.raises(ValueError, match="CKKS only"):
        S._check(relin(bfv.handle, size=2, stride=1))
    for h in ok:
        for fn in entries:
            for count in (1, 0):
                for k in (0, 3, 4, 9):  # (k = 3 is the key level of these contexts: two special primes)
                    with pytest.raises(ValueError, match="level k out of range"):
                        S._check(fn(h, k=k, count=count))
                with pytest.raises(ValueError, match="end of modulus switching chain reached"):
                    S._check(fn(h, k=1, count=count))
        # ... the level before the size, the size before the stride
        with pytest.raises(ValueError, match="end of modulus switching chain reached"):
            S._check(relin(h, k=1, size=2, stride=1))
        for count in (1, 0):
            for size in (2, 4, 0):
                with pytest.raises(ValueError, match="size 3"):
                    S._check(relin(h, size=size, stride=1, count=count))
            with pytest.raises(ValueError, match="item stride"):
                S._check(relin(h, stride=3 * 2 * n - 1, count=count))
            with pytest.raises(ValueError, match="not enough relinearization keys"):
                S._check(relin(h, n_keys=0, count=count))
            with pytest.raises(ValueError, match="not enough relinearization keys"):
                S._check(dotp(h, n_keys=0, count=count))
        # the unmerged entries' own errors
        with pytest.raises(ValueError, match="term lists must not be empty"):
            S._check(dotp(h, n_terms=0))
        for bad in (0, 4, 2 * n, 2 * n + 1):
            for count in (1, 0):
                with pytest.raises(ValueError, match="Galois element is not valid"):
                    S._check(dot(h, count=count, elts=(C.c_uint32 * 2)(1, bad), keys=(C.c_void_p * 2)(None, p)))
                with pytest.raises(ValueError, match="Galois element is not valid"):
                    S._check(bsgs(h, count=count, baby=(C.c_uint32 * 2)(1, bad), bkeys=(C.c_void_p * 2)(None, p)))
        with pytest.raises(ValueError, match="Galois key not present"):
            S._check(rot(h, steps=step1))
        with pytest.raises(ValueError, match="Galois key not present"):
            S._check(rbsgs(h, gs=step1))
        for kw in ({"n_elts": 0}, {"n_sums": 0}):
            with pytest.raises(ValueError, match="empty sum"):
                S._check(dot(h, **kw))
        for kw in ({"n_baby": 0}, {"n_giant": 0}):
            with pytest.raises(ValueError, match="empty sum"):
                S._check(bsgs(h, **kw))
    for h in ok:
        for kw in ({"out": p}, {"out": p + 8}, {"ct": far, "out": far + 8 * (2 * 2 * n - 1)}):
            for fn in (dot, rot, bsgs, rbsgs):
                with pytest.raises(ValueError, match="overlap"):
                    S._check(fn(h, **kw))
    # 3. nothing to do: S_OK, no device needed (relinearize_rescale and dot_product_rescale need a key: on the GPU)
    for h in ok:
        for fn in (dot, rot, bsgs, rbsgs):
            assert fn(h, count=0) == 0
        assert dot(h, count=0, n_elts=0) == 0 and rbsgs(h, count=0, n_baby=0) == 0
    # 4. a valid call with work to do is refused as host-only (element 1 / step 0 needs no key)
    for h in ok:
        for fn in (dot, rot, bsgs, rbsgs):
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(fn(h))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits,nsp", SETS)
def test_no_key_switch_term_is_rescale_to_next(bits, nsp, mode):
    """acc = 0 in the merged formula: ref_mod_switch_scale_to_next of base, word for word, at every level"""
    n = 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, 6, mods, nsp=nsp, t=0, mode=mode)
    rng = np.random.default_rng(nsp)
    for k in range(ref.k_first, 1, -1):
        base = np.stack([np.stack([rng.integers(0, p, size=n, dtype=np.uint64) for p in mods[:k]]) for _ in range(2)])
        assert np.array_equal(R.finish_rescale(ref, k, base, None), R.rescale(ref, k, base)), k


@pytest.mark.parametrize("bits", [[61, 61, 60], [50, 51, 60, 61, 58], [61] * 5 + [60] * 5 + [59]])
def test_exact_quotient_against_big_integers(bits):
    """steps 2-5 on one coefficient against floor((X + half) / D) in Python integers: dropped sets of 2, 4 and 10 primes (the
    last prime of the list is the kept one); random X, and the X whose scaled residues z_d are all 0 and all d - 1"""
    primes = [int(p) for p in O.coeff_modulus_create(64, bits)]
    dset, q = primes[:-1], primes[-1]
    assert len(set(primes)) == len(primes)
    D = 1
    for d in dset:
        D *= d
    half = D // 2
    rng = np.random.default_rng(len(bits))

    def check(X):
        Y = X % D
        z = R.scaled_residues([Y % d for d in dset], dset, D, half)
        v = R.quotient(z, dset)
        assert 0 <= v < len(dset)
        total = sum(zi * (D // d) for zi, d in zip(z, dset))
        assert total - v * D == (Y + half) % D, "the quotient is exact"
        temp = R.convert(z, v, dset, D, half, q)
        out = (X - temp) * pow(D % q, -1, q) % q
        assert out == ((X + half) // D) % q
        return z

    def crt(z):
        """the Y whose scaled residues are z"""
        s = sum(zi * (D // d) for zi, d in zip(z, dset)) % D
        return (s - half) % D

    assert check(crt([0] * len(dset))) == [0] * len(dset)
    assert check(crt([d - 1 for d in dset])) == [d - 1 for d in dset]
    for _ in range(2000):
        X = int.from_bytes(rng.bytes(96), "little") % (D * q)
        check(X)
    for X in (0, 1, half, half + 1, D - 1, D, D * q - 1):
        check(X)


def _galois_int(m, g, n):
    """x -> x^g on an integer polynomial of Z[x] / (x^N + 1)"""
    out = [0] * n
    for i in range(n):
        j = (i * g) % (2 * n)
        out[j % n] = -int(m[i]) if j >= n else int(m[i])
    return out


def _negacyclic_int(a, b, n):
    out = [0] * n
    for i in range(n):
        if a[i]:
            for j in range(n):
                if i + j < n:
                    out[i + j] += a[i] * b[j]
                else:
                    out[i + j - n] -= a[i] * b[j]
    return out


def _weighted_sum(m, elts, weights, n):
    want = [0] * n
    for g, w in zip(elts, weights):
        term = _negacyclic_int([int(v) for v in w], _galois_int(m, g, n), n)
        want = [a + b for a, b in zip(want, term)]
    return want


def _ckks_error(cl, ct, want):
    k = ct.shape[1]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
    got, _ = cl.centered_from_ntt_rows(dot)
    return max(abs(a - b) for a, b in zip(got, want))


def _divided(want, q):
    """round(want / q), halves up: the plaintext after the rescale"""
    return [(2 * v + q) // (2 * q) for v in want]


def _bar(e_m, e_c, tag):
    """e_merged <= 2 * e_composed + 1: both errors have the same bound (the key switch's noise divided by q_{k-1} plus the
    rounding of the division; the merged form rounds once where the composition rounds twice), and the factor 2 covers one
    sample's spread -- the bar tests/test_hoist_dot_host.py uses for the same reason"""
    print(tag, "merged", e_m, "composed", e_c)
    assert e_m <= 2 * e_c + 1, (tag, e_m, e_c)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits,nsp", SETS)
def test_relinearize_rescale_decrypts(bits, nsp, mode):
    """multiply -> relinearize -> rescale on fresh encryptions of 25-bit messages, at every level from the first to 2"""
    n = 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, 6, mods, nsp=nsp, t=0, mode=mode)
    cl = O.Client(ref, seed=5)
    rng = np.random.default_rng(3)
    ma = [int(v) for v in rng.integers(-(1 << 24), 1 << 24, size=n)]
    mb = [int(v) for v in rng.integers(-(1 << 24), 1 << 24, size=n)]
    a, b = cl.encrypt_poly_ntt(ma), cl.encrypt_poly_ntt(mb)
    rk = cl.relin_key()
    want = _negacyclic_int(ma, mb, n)
    for k in range(cl.k, 1, -1):
        ak, bk = np.ascontiguousarray(a[:, :k]), np.ascontiguousarray(b[:, :k])  # (CKKS mod_switch_to_next drops the last prime)
        prod = R.DC.ckks_dot_product(ref, k, [ak], [bk], None)
        merged = R.relinearize_rescale(ref, k, prod, rk)
        assert np.array_equal(merged, R.dot_product_rescale(ref, k, [ak], [bk], rk))  # (one term: the same words)
        comp = R.rescale(ref, k, R.DC.dot_product(ref, k, [ak], [bk], rk))
        w = _divided(want, int(mods[k - 1]))
        _bar(_ckks_error(cl, merged, w), _ckks_error(cl, comp, w), ("relinearize", bits, nsp, mode, k))


@pytest.mark.parametrize("mode", [0, 1])
def test_dot_product_rescale_decrypts(mode):
    bits, nsp = SETS[1]
    n = 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, 6, mods, nsp=nsp, t=0, mode=mode)
    cl = O.Client(ref, seed=7)
    rng = np.random.default_rng(11)
    ms = [[int(v) for v in rng.integers(-(1 << 22), 1 << 22, size=n)] for _ in range(6)]
    cts = [cl.encrypt_poly_ntt(m) for m in ms]
    rk = cl.relin_key()
    want = [0] * n
    for i in range(3):
        want = [x + y for x, y in zip(want, _negacyclic_int(ms[i], ms[3 + i], n))]
    for k in (cl.k, 2):
        a = [np.ascontiguousarray(c[:, :k]) for c in cts[:3]]
        b = [np.ascontiguousarray(c[:, :k]) for c in cts[3:]]
        merged = R.dot_product_rescale(ref, k, a, b, rk)
        comp = R.rescale(ref, k, R.DC.dot_product(ref, k, a, b, rk))
        w = _divided(want, int(mods[k - 1]))
        _bar(_ckks_error(cl, merged, w), _ckks_error(cl, comp, w), ("dot_product", mode, k))


@pytest.mark.parametrize("mode", [0, 1])
def test_dot_plain_rescale_decrypts(mode):
    bits, nsp = SETS[2]
    n = 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, 6, mods, nsp=nsp, t=0, mode=mode)
    cl = O.Client(ref, seed=5)
    rng = np.random.default_rng(17)
    msg = [int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=n)]
    ct = cl.encrypt_poly_ntt(msg)
    elts = [1, H.elt_from_step(n, 1), H.elt_from_step(n, -5), 2 * n - 1, 3]
    keys = [None if g == 1 else cl.galois_key(g) for g in elts]
    w = rng.integers(-(1 << 20), 1 << 20, size=(len(elts), n))
    plains = np.stack([HD.lift_plain(ref, w[i]) for i in range(len(elts))])[None]
    want = _weighted_sum(msg, elts, w, n)
    for k in (cl.k, 2):
        c = np.ascontiguousarray(ct[:, :k])
        merged = R.dot_plain_rescale_one(ref, k, c, elts, keys, plains)[0]
        comp = R.rescale(ref, k, HD.dot_plain_one(ref, k, c, elts, keys, plains)[0])
        wd = _divided(want, int(mods[k - 1]))
        _bar(_ckks_error(cl, merged, wd), _ckks_error(cl, comp, wd), ("dot_plain", mode, k))


@pytest.mark.parametrize("mode", [0, 1])
def test_bsgs_plain_rescale_decrypts(mode):
    bits, nsp = SETS[0]
    n = 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, 6, mods, nsp=nsp, t=0, mode=mode)
    cl = O.Client(ref, seed=9)
    rng = np.random.default_rng(23)
    msg = [int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=n)]
    ct = cl.encrypt_poly_ntt(msg)
    baby, giant = [1, H.elt_from_step(n, 1), H.elt_from_step(n, 2)], [1, H.elt_from_step(n, 3), 2 * n - 1]
    bkeys = [None if g == 1 else cl.galois_key(g) for g in baby]
    gkeys = [None if g == 1 else cl.galois_key(g) for g in giant]
    w = rng.integers(-(1 << 18), 1 << 18, size=(len(giant), len(baby), n))
    plains = np.stack([np.stack([HD.lift_plain(ref, w[j, i]) for i in range(len(baby))]) for j in range(len(giant))])
    want = [0] * n
    for j, h in enumerate(giant):
        inner = _weighted_sum(msg, baby, w[j], n)
        want = [x + y for x, y in zip(want, _galois_int(inner, h, n))]
    for k in (cl.k, 2):
        c = np.ascontiguousarray(ct[:, :k])
        merged = R.bsgs_plain_rescale_one(ref, k, c, baby, bkeys, giant, gkeys, plains)
        comp = R.rescale(ref, k, BS.bsgs_one(ref, k, c, baby, bkeys, giant, gkeys, plains))
        wd = _divided(want, int(mods[k - 1]))
        _bar(_ckks_error(cl, merged, wd), _ckks_error(cl, comp, wd), ("bsgs", mode, k))


def test_kernel_arithmetic_on_the_cpu(tmp_path):
    exe = compile_cpp(tmp_path, "ks_rescale_bounds_check.cpp")
    assert "ks_rescale_bounds_check: OK" in run_exe(exe, timeout=300)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_ks_rescale_check.cpp", link_sealhip=True)
    assert "host-only ks rescale checks ok" in run_exe(exe, "host", timeout=120)
