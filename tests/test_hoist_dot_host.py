"""Plaintext-weighted sums of rotations (sealhip_evaluator_apply_galois_dot_plain / _rotate_vector_dot_plain, DESIGN.md section
16): what can be checked without a GPU. The exports and their mirrors; the argument checks on host-only contexts, in the
header's order; and the CPU restatement (tests/hoist_dot_ref.py) itself: it decrypts exactly to sum_i w_i * sigma_{g_i}(m)
(BFV STRICT) and within the error of the composition it replaces (CKKS), with other words than the composition."""
import ctypes as C
import os

import numpy as np
import pytest

import hoist_dot_ref as HD
import hoist_ref as H
import oracle_lib as O
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_apply_galois_dot_plain", "sealhip_evaluator_rotate_vector_dot_plain")


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("apply_galois_dot_plain", "rotate_vector_dot_plain"):
        assert callable(getattr(S.Evaluator, name))
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert name in header


def test_entries_on_host_only_context():
    """E_POINTER first (a NULL key only for element 1); then the level, the element, the BFV PARITY refusal and the empty sum
    (E_INVALIDARG); then the empty batch (S_OK); then the host-only context (COR_E_INVALIDOPERATION). A key handle cannot
    exist without a device, so the check that looks INTO a key -- its digit count -- is exercised in
    tests/test_gpu_hoist_dot.py; element 1 needs no key, so the element checks run here with it next to the bad element."""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    parity = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, device=-1)
    strict = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    L = S.lib()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    ident = (C.c_uint32 * 2)(1, 1)
    three = (C.c_uint32 * 2)(1, 3)
    nokey = (C.c_void_p * 2)(None, None)
    step0 = (C.c_int32 * 2)(0, 0)
    step1 = (C.c_int32 * 2)(0, 1)

    def dot(ctx, k=2, ct=p, count=1, elts=ident, keys=nokey, n_elts=2, plain=p, n_sums=1, out=p):
        return L.sealhip_evaluator_apply_galois_dot_plain(ctx, k, ct, count, elts, keys, n_elts, plain, n_sums, out)

    def rot(ctx, k=2, ct=p, count=1, steps=step0, n_steps=2, elts=None, keys=None, n_keys=0, plain=p, n_sums=1, out=p):
        return L.sealhip_evaluator_rotate_vector_dot_plain(ctx, k, ct, count, steps, n_steps, elts, keys, n_keys, plain, n_sums,
                                                           out)

    ok = (strict.handle, ckks.handle)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG); a null key is a null pointer unless the element is 1
    for h in ok + (parity.handle,):
        for kw in ({"ct": None}, {"out": None}, {"plain": None}, {"elts": None}, {"keys": None}, {"elts": three}):
            with pytest.raises(TypeError):
                S._check(dot(h, k=9, **kw))
        for kw in ({"ct": None}, {"out": None}, {"plain": None}, {"steps": None}, {"n_keys": 1, "keys": nokey},
                   {"n_keys": 1, "elts": three}):
            with pytest.raises(TypeError):
                S._check(rot(h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(dot(None))
    with pytest.raises(TypeError):
        S._check(rot(None))
    # 2. invalid arguments, also for an empty batch: the level (k = 3 is the key level of these contexts)
    for h in ok:
        for k in (0, 3, 4, 5):
            for count in (1, 0):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(dot(h, k=k, count=count))
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(rot(h, k=k, count=count))
        for bad in (0, 4, 2 * n, 2 * n + 1):
            for count in (1, 0):
                with pytest.raises(ValueError, match="Galois element is not valid"):
                    S._check(dot(h, count=count, elts=(C.c_uint32 * 2)(1, bad), keys=(C.c_void_p * 2)(None, p)))
        with pytest.raises(ValueError, match="Galois key not present"):
            S._check(rot(h, steps=step1))
        with pytest.raises(ValueError, match="Galois key not present"):
            S._check(rot(h, steps=step1, n_keys=1, elts=three, keys=(C.c_void_p * 1)(p)))  # (1 is not the element of step 1)
    for count, n in ((1, 2), (0, 2), (1, 0)):
        with pytest.raises(ValueError, match="STRICT"):
            S._check(dot(parity.handle, count=count, n_elts=n))
        with pytest.raises(ValueError, match="STRICT"):
            S._check(rot(parity.handle, count=count, n_steps=n))
    for h in ok:
        for kw in ({"n_elts": 0}, {"n_sums": 0}):
            with pytest.raises(ValueError, match="empty sum"):
                S._check(dot(h, **kw))
        for kw in ({"n_steps": 0}, {"n_sums": 0}):
            with pytest.raises(ValueError, match="empty sum"):
                S._check(rot(h, **kw))
    # 3. nothing to do: S_OK, no device needed (an empty sum of an empty batch included)
    for h in ok:
        for k in (1, 2):
            assert dot(h, k=k, count=0) == 0 and dot(h, k=k, count=0, n_elts=0) == 0 and dot(h, k=k, count=0, n_sums=0) == 0
            assert rot(h, k=k, count=0) == 0 and rot(h, k=k, count=0, n_steps=0) == 0
    # 4. a valid call with work to do is refused as host-only (element 1 / step 0 needs no key)
    for h in ok:
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(dot(h))
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(rot(h))


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


def _elts(n):
    return [H.elt_from_step(n, 1), 1, H.elt_from_step(n, -5), 2 * n - 1, 3]


@pytest.mark.parametrize("bits,nsp", [([40, 40, 40, 41], 1), ([36] * 5 + [37] * 3, 3)])
def test_restatement_bfv_strict_decrypts_exactly(bits, nsp):
    """N = 64, t = 257, weights uniform in [0, t), centred and lifted to every key prime: at the first level and one level
    below the restatement decrypts exactly to sum_i w_i * sigma_{g_i}(m) mod (x^N + 1, t); its words are not those of the
    composition (the hoisted rotation per element, the plaintext product, the add)"""
    logn, n, t = 6, 64, 257
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(1, logn, mods, nsp=nsp, t=t, mode=1)
    cl = O.Client(ref, seed=3)
    L = O.lib()
    rng = np.random.default_rng(len(bits))
    m = rng.integers(0, t, size=n, dtype=np.uint64)
    top = cl.encrypt_bfv(m)
    below = np.zeros((2, cl.k - 1, n), dtype=np.uint64)
    assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), cl.k, O.ptr(top), 2, O.ptr(below)) == 0
    elts = _elts(n)
    keys = [None if g == 1 else cl.galois_key(g) for g in elts]
    w = rng.integers(0, t, size=(len(elts), n), dtype=np.int64)
    centred = np.where(w > t // 2, w - t, w)
    plains = np.stack([HD.lift_plain(ref, centred[i]) for i in range(len(elts))])[None]
    want = np.array([v % t for v in _weighted_sum([int(v) for v in m], elts, centred, n)], dtype=np.uint64)
    for ct in (top, below):
        k = ct.shape[1]
        out = HD.dot_plain_one(ref, k, ct, elts, keys, plains)[0]
        assert np.array_equal(cl.decrypt_bfv(out), want), k
        comp = HD.composed_one(ref, k, ct, elts, keys, plains[0])
        assert np.array_equal(cl.decrypt_bfv(comp), want), k
        assert not np.array_equal(comp, out), k  # same plaintext, other words: one mod-down of the weighted sum


def _ckks_error(cl, ct, want):
    k = ct.shape[1]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
    got, _ = cl.centered_from_ntt_rows(dot)
    return max(abs(a - b) for a, b in zip(got, want))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits,nsp", [([40, 40, 40, 41], 1), ([36] * 4 + [37] * 2, 2)])
def test_restatement_ckks_error_of_the_composition(bits, nsp, mode):
    """e_fused <= 2 * e_composed + 1 on the same ciphertext and keys, at the first level and one below: both errors have the
    same bound (the fused result carries one mod-down rounding that no plaintext amplifies, the composition one per
    rotation, each multiplied by its plaintext; the encryption noise times the plaintexts is common to both), and the
    factor 2 covers one sample's spread -- the bar tests/test_hoist_host.py uses for the same reason"""
    logn, n = 6, 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, logn, mods, nsp=nsp, t=0, mode=mode)
    cl = O.Client(ref, seed=5)
    rng = np.random.default_rng(17 + nsp)
    msg = [int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=n)]
    ct = cl.encrypt_poly_ntt(msg)
    elts = [1] + _elts(n)[:1] + _elts(n)[2:]
    keys = [None if g == 1 else cl.galois_key(g) for g in elts]
    w = rng.integers(-(1 << 10), 1 << 10, size=(len(elts), n))
    plains = np.stack([HD.lift_plain(ref, w[i]) for i in range(len(elts))])[None]
    want = _weighted_sum(msg, elts, w, n)
    for k in (cl.k, cl.k - 1):
        c = np.ascontiguousarray(ct[:, :k])  # (CKKS mod_switch_to_next drops the last prime)
        out = HD.dot_plain_one(ref, k, c, elts, keys, plains)[0]
        comp = HD.composed_one(ref, k, c, elts, keys, plains[0])
        e_f, e_c = _ckks_error(cl, out, want), _ckks_error(cl, comp, want)
        print("ckks nsp=%d mode=%d k=%d: fused %d composed %d" % (nsp, mode, k, e_f, e_c))
        assert e_f <= 2 * e_c + 1, (k, e_f, e_c)
        assert not np.array_equal(comp, out)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_hoist_dot_check.cpp", link_sealhip=True)
    assert "host-only hoist dot checks ok" in run_exe(exe, "host", timeout=120)
