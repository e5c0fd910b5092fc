"""Baby-step/giant-step matrix-vector products (sealhip_evaluator_apply_galois_bsgs_plain / _rotate_vector_bsgs_plain, DESIGN.md
section 17): what can be checked without a GPU. The exports and their mirrors; the argument checks on host-only contexts, in
the header's order; and the CPU restatement (tests/hoist_bsgs_ref.py) itself: it decrypts exactly to
sum_j sigma_{h_j}( sum_i w_ji * sigma_{g_i}(m) ) (BFV STRICT), within the error of the composition it replaces (CKKS), and its
degenerate shapes are, word for word, what they reduce to."""
import ctypes as C
import os

import numpy as np
import pytest

import hoist_bsgs_ref as HB
import hoist_dot_ref as HD
import hoist_ref as H
import oracle_lib as O
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_apply_galois_bsgs_plain", "sealhip_evaluator_rotate_vector_bsgs_plain")


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("apply_galois_bsgs_plain", "rotate_vector_bsgs_plain"):
        assert callable(getattr(S.Evaluator, name))
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert name in header
    assert "tests/hoist_bsgs_ref.py" in header


def test_entries_on_host_only_context():
    """E_POINTER first (a NULL key only for element 1, on either axis); then the level, the element, the BFV PARITY refusal and
    the empty sum (E_INVALIDARG); then the empty batch (S_OK); then the host-only context (COR_E_INVALIDOPERATION). The check
    that looks INTO a key -- its digit count -- needs a device and is exercised in tests/test_gpu_hoist_bsgs.py."""
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

    def app(ctx, k=2, ct=p, count=1, baby=ident, bkeys=nokey, n_baby=2, giant=ident, gkeys=nokey, n_giant=2, plain=p, out=p):
        return L.sealhip_evaluator_apply_galois_bsgs_plain(ctx, k, ct, count, baby, bkeys, n_baby, giant, gkeys, n_giant, plain,
                                                           out)

    def rot(ctx, k=2, ct=p, count=1, baby=step0, n_baby=2, giant=step0, n_giant=2, elts=None, keys=None, n_keys=0, plain=p,
            out=p):
        return L.sealhip_evaluator_rotate_vector_bsgs_plain(ctx, k, ct, count, baby, n_baby, giant, n_giant, elts, keys, n_keys,
                                                            plain, out)

    ok = (strict.handle, ckks.handle)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG); a null key is a null pointer unless the element is 1
    for h in ok + (parity.handle,):
        for kw in ({"ct": None}, {"out": None}, {"plain": None}, {"baby": None}, {"bkeys": None}, {"baby": three},
                   {"giant": None}, {"gkeys": None}, {"giant": three}):
            with pytest.raises(TypeError):
                S._check(app(h, k=9, **kw))
        for kw in ({"ct": None}, {"out": None}, {"plain": None}, {"baby": None}, {"giant": None}, {"n_keys": 1, "keys": nokey},
                   {"n_keys": 1, "elts": three}):
            with pytest.raises(TypeError):
                S._check(rot(h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(app(None))
    with pytest.raises(TypeError):
        S._check(rot(None))
    # 2. invalid arguments, also for an empty batch
    for h in ok:
        for k in (0, 3, 4, 5):
            for count in (1, 0):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(app(h, k=k, count=count))
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(rot(h, k=k, count=count))
        for bad in (0, 4, 2 * n, 2 * n + 1):
            for count in (1, 0):
                for axis in ("baby", "giant"):
                    kw = {axis: (C.c_uint32 * 2)(1, bad), axis[0] + "keys": (C.c_void_p * 2)(None, p)}
                    with pytest.raises(ValueError, match="Galois element is not valid"):
                        S._check(app(h, count=count, **kw))
        for axis in ("baby", "giant"):
            with pytest.raises(ValueError, match="Galois key not present"):
                S._check(rot(h, **{axis: step1}))
            with pytest.raises(ValueError, match="Galois key not present"):
                S._check(rot(h, n_keys=1, elts=three, keys=(C.c_void_p * 1)(p), **{axis: step1}))
    for count, nb, ng in ((1, 2, 2), (0, 2, 2), (1, 0, 2), (1, 2, 0)):
        with pytest.raises(ValueError, match="STRICT"):
            S._check(app(parity.handle, count=count, n_baby=nb, n_giant=ng))
        with pytest.raises(ValueError, match="STRICT"):
            S._check(rot(parity.handle, count=count, n_baby=nb, n_giant=ng))
    for h in ok:
        for kw in ({"n_baby": 0}, {"n_giant": 0}):
            with pytest.raises(ValueError, match="empty sum"):
                S._check(app(h, **kw))
            with pytest.raises(ValueError, match="empty sum"):
                S._check(rot(h, **kw))
    # 3. nothing to do: S_OK, no device needed (an empty sum of an empty batch included)
    for h in ok:
        for k in (1, 2):
            assert app(h, k=k, count=0) == 0 and app(h, k=k, count=0, n_baby=0) == 0 and app(h, k=k, count=0, n_giant=0) == 0
            assert rot(h, k=k, count=0) == 0 and rot(h, k=k, count=0, n_baby=0) == 0 and rot(h, k=k, count=0, n_giant=0) == 0
    # 4. a valid call with work to do is refused as host-only (element 1 / step 0 needs no key)
    for h in ok:
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(app(h))
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


def _matvec(m, baby, giant, weights, n):
    """sum_j sigma_{h_j}( sum_i w_ji * sigma_{g_i}(m) ) over the integers"""
    want = [0] * n
    for j, h in enumerate(giant):
        inner = [0] * n
        for i, g in enumerate(baby):
            term = _negacyclic_int([int(v) for v in weights[j][i]], _galois_int(m, g, n), n)
            inner = [a + b for a, b in zip(inner, term)]
        want = [a + b for a, b in zip(want, _galois_int(inner, h, n))]
    return want


def _axes(n):
    """baby and giant elements, the identity on each axis (second baby, first giant) and a repeat among the giants"""
    baby = [H.elt_from_step(n, 1), 1, H.elt_from_step(n, -5)]
    giant = [1, H.elt_from_step(n, 3), 2 * n - 1, H.elt_from_step(n, 3)]
    return baby, giant


def _keys(cl, elts):
    cache = {}
    for g in elts:
        if g != 1 and g not in cache:
            cache[g] = cl.galois_key(g)
    return [cache.get(g) for g in elts]


@pytest.mark.parametrize("bits,nsp", [([40, 40, 40, 41], 1), ([36] * 5 + [37] * 3, 3)])
def test_restatement_bfv_strict_decrypts_exactly(bits, nsp):
    """N = 64, t = 257, weights uniform in [0, t), centred and lifted to every key prime: at the first level and one level
    below the restatement decrypts exactly to sum_j sigma_{h_j}( sum_i w_ji sigma_{g_i}(m) ) mod (x^N + 1, t), with an identity
    on each axis; its words are not those of the composition"""
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
    baby, giant = _axes(n)
    bkeys, gkeys = _keys(cl, baby), _keys(cl, giant)
    w = rng.integers(0, t, size=(len(giant), len(baby), n), dtype=np.int64)
    centred = np.where(w > t // 2, w - t, w)
    plains = np.stack([np.stack([HD.lift_plain(ref, centred[j, i]) for i in range(len(baby))]) for j in range(len(giant))])
    want = np.array([v % t for v in _matvec([int(v) for v in m], baby, giant, centred, n)], dtype=np.uint64)
    for ct in (top, below):
        k = ct.shape[1]
        out = HB.bsgs_one(ref, k, ct, baby, bkeys, giant, gkeys, plains)
        assert np.array_equal(cl.decrypt_bfv(out), want), k
        comp = HB.composed_one(ref, k, ct, baby, bkeys, giant, gkeys, plains)
        assert np.array_equal(cl.decrypt_bfv(comp), want), k
        assert not np.array_equal(comp, out), k  # same plaintext, other words


def _ckks_error(cl, ct, want):
    k = ct.shape[1]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
    got, _ = cl.centered_from_ntt_rows(dot)
    return max(abs(a - b) for a, b in zip(got, want))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits,nsp", [([40, 40, 40, 41], 1), ([36] * 4 + [37] * 2, 2)])
def test_restatement_ckks_error_of_the_composition(bits, nsp, mode):
    """e_fused <= 2 * e_composed on the same ciphertext and keys, at the first level and one below, against the exact integer
    arithmetic: both errors are sums of rounding and key-switch terms with the same bound (the composition rounds every inner
    sum twice more), and the factor 2 covers one sample's spread"""
    logn, n = 6, 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, logn, mods, nsp=nsp, t=0, mode=mode)
    cl = O.Client(ref, seed=5)
    rng = np.random.default_rng(17 + nsp)
    msg = [int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=n)]
    ct = cl.encrypt_poly_ntt(msg)
    baby, giant = _axes(n)
    bkeys, gkeys = _keys(cl, baby), _keys(cl, giant)
    w = rng.integers(-(1 << 10), 1 << 10, size=(len(giant), len(baby), n))
    plains = np.stack([np.stack([HD.lift_plain(ref, w[j, i]) for i in range(len(baby))]) for j in range(len(giant))])
    want = _matvec(msg, baby, giant, w, n)
    for k in (cl.k, cl.k - 1):
        c = np.ascontiguousarray(ct[:, :k])  # (CKKS mod_switch_to_next drops the last prime)
        out = HB.bsgs_one(ref, k, c, baby, bkeys, giant, gkeys, plains)
        comp = HB.composed_one(ref, k, c, baby, bkeys, giant, gkeys, plains)
        e_f, e_c = _ckks_error(cl, out, want), _ckks_error(cl, comp, want)
        print("ckks nsp=%d mode=%d k=%d: fused %d composed %d ratio %.3f" % (nsp, mode, k, e_f, e_c, e_f / max(e_c, 1)))
        assert e_f <= 2 * e_c, (k, e_f, e_c)
        assert not np.array_equal(comp, out)


@pytest.mark.parametrize("scheme", [1, 2])
def test_degenerate_shapes_are_what_they_reduce_to(scheme):
    """all giants = 1: the canonical sum of the inner sums' parts finished once, which is HD.dot_plain over the baby list
    repeated per giant (repeated elements add canonically); n_giant = 1, h = 1: HD.dot_plain; every element 1: no key switch."""
    logn, n, t = 6, 64, 257
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    ref = O.RefContext(scheme, logn, mods, nsp=1, t=t if scheme == 1 else 0, mode=1)
    cl = O.Client(ref, seed=9)
    rng = np.random.default_rng(scheme)
    k = cl.k
    if scheme == 1:
        ct = cl.encrypt_bfv(rng.integers(0, t, size=n, dtype=np.uint64))
    else:
        ct = cl.encrypt_poly_ntt([int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=n)])
    baby, _ = _axes(n)
    bkeys = _keys(cl, baby)
    plains = np.stack([np.stack([HD.lift_plain(ref, rng.integers(-100, 100, size=n)) for _ in baby]) for _ in range(3)])
    ones = [1, 1, 1]
    got = HB.bsgs_one(ref, k, ct, baby, bkeys, ones, [None] * 3, plains)
    flat = plains.reshape((1, 3 * len(baby)) + plains.shape[2:])
    assert np.array_equal(got, HD.dot_plain_one(ref, k, ct, baby * 3, bkeys * 3, flat)[0])
    got = HB.bsgs_one(ref, k, ct, baby, bkeys, [1], [None], plains[:1])
    assert np.array_equal(got, HD.dot_plain_one(ref, k, ct, baby, bkeys, plains[:1])[0])
    got = HB.bsgs_one(ref, k, ct, [1, 1], [None, None], ones, [None] * 3, plains[:, :2])
    flat = np.ascontiguousarray(plains[:, :2]).reshape((1, 6) + plains.shape[2:])
    assert np.array_equal(got, HD.dot_plain_one(ref, k, ct, [1] * 6, [None] * 6, flat)[0])


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_bsgs_check.cpp", link_sealhip=True)
    assert "host-only bsgs checks ok" in run_exe(exe, "host", timeout=120)
