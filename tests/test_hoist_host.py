"""Hoisted rotation (sealhip_evaluator_apply_galois_many / _rotate_vector_many): what can be checked
without a GPU. The exports and their mirrors; the argument checks on host-only contexts, in the header's order; the block
property of the NTT-form Galois table the kernel's gathered loads rely on; and the CPU restatement (tests/hoist_ref.py)
itself: it decrypts to the rotated plaintext (BFV STRICT) and within the error of the sequential rotation (CKKS)."""
import ctypes as C
import os

import numpy as np
import pytest

import hoist_ref as H
import oracle_lib as O
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_apply_galois_many", "sealhip_evaluator_rotate_vector_many")


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("apply_galois_many", "rotate_vector_many"):
        assert callable(getattr(S.Evaluator, name))
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert name in header


def test_entries_on_host_only_context():
    """E_POINTER first; then the level, the element and the BFV PARITY refusal (E_INVALIDARG); then the empty call (S_OK);
    then the host-only context (COR_E_INVALIDOPERATION). A key handle cannot exist without a device (sealhip_kswitch_key_load
    needs one), so the checks that look INTO a key -- its digit count -- and the element checks of apply_galois_many, which
    come after the null check of the element's key, are exercised in tests/test_gpu_hoist.py; here the elements go
    through rotate_vector_many's steps."""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    parity = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, device=-1)
    strict = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    L = S.lib()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    one = (C.c_uint32 * 1)(3)
    nokey = (C.c_void_p * 1)(None)
    step0 = (C.c_int32 * 2)(0, 0)
    step1 = (C.c_int32 * 2)(0, 1)

    def many(ctx, k=2, ct=p, count=1, elts=None, keys=None, n_elts=0, out=p):
        return L.sealhip_evaluator_apply_galois_many(ctx, k, ct, count, elts, keys, n_elts, out)

    def rot(ctx, k=2, ct=p, count=1, steps=step0, n_steps=2, elts=None, keys=None, n_keys=0, out=p):
        return L.sealhip_evaluator_rotate_vector_many(ctx, k, ct, count, steps, n_steps, elts, keys, n_keys, out)

    ok = (strict.handle, ckks.handle)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG)
    for h in ok + (parity.handle,):
        for kw in ({"ct": None}, {"out": None}, {"n_elts": 1, "keys": nokey}, {"n_elts": 1, "elts": one},
                   {"n_elts": 1, "elts": one, "keys": nokey}):
            with pytest.raises(TypeError):
                S._check(many(h, k=9, **kw))
        for kw in ({"ct": None}, {"out": None}, {"steps": None}, {"n_keys": 1, "keys": nokey}, {"n_keys": 1, "elts": one}):
            with pytest.raises(TypeError):
                S._check(rot(h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(many(None))
    with pytest.raises(TypeError):
        S._check(rot(None))
    # 2. invalid arguments, also for an empty call: the level (k = 3 is the key level of these contexts: no ciphertext level)
    for h in ok:
        for k in (0, 3, 4, 5):
            for count in (1, 0):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(many(h, k=k, count=count))
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(rot(h, k=k, count=count))
        with pytest.raises(ValueError, match="Galois key not present"):
            S._check(rot(h, steps=step1))
        with pytest.raises(ValueError, match="Galois key not present"):
            S._check(rot(h, steps=step1, n_keys=1, elts=one, keys=nokey))  # (3 is not the element of step 1)
    for count, n_steps in ((1, 2), (0, 2), (1, 0)):
        with pytest.raises(ValueError, match="STRICT"):
            S._check(many(parity.handle, count=count))
        with pytest.raises(ValueError, match="STRICT"):
            S._check(rot(parity.handle, count=count, n_steps=n_steps))
    # 3. nothing to do: S_OK, no device needed
    for h in ok:
        for k in (1, 2):
            assert many(h, k=k, count=1) == 0 and many(h, k=k, count=0) == 0
            assert rot(h, k=k, n_steps=0) == 0 and rot(h, k=k, count=0) == 0
    # 4. a valid call with work to do is refused as host-only (step 0 needs no key)
    for h in ok:
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(rot(h))


@pytest.mark.parametrize("logn", [4, 12, 15])
def test_galois_table_block_property(logn):
    """T_g maps every aligned block of 2^b indices onto an aligned block of 2^b indices and permutes only inside it, for
    every b and every odd g: a wave's 64 gathered words lie in the lines one aligned straight read touches (hoist.hip).
    And T_{g^-1} inverts T_g (the identity the restatement rests on)."""
    n = 1 << logn
    elts = [3, 5, 25, 2 * n - 1, H.elt_from_step(n, 1), H.elt_from_step(n, -3), (0x5DEECE66D % (2 * n)) | 1]
    idx = np.arange(n, dtype=np.int64)
    for g in elts:
        tab = H.galois_table(logn, g).astype(np.int64)
        assert np.array_equal(np.sort(tab), idx), g
        for b in range(1, 5):
            blocks = (tab >> b).reshape(-1, 1 << b)
            assert np.all(blocks == blocks[:, :1]), (g, b)            # one destination block per source block
            assert len(np.unique(blocks[:, 0])) == n >> b, (g, b)     # ... and the blocks are permuted among themselves
        inv = H.galois_table(logn, pow(g, -1, 2 * n)).astype(np.int64)
        assert np.array_equal(tab[inv], idx) and np.array_equal(inv[tab], idx), g


def _galois_plain(m, g, n, t):
    """x -> x^g on a plaintext polynomial mod t"""
    out = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        j = (i * g) % (2 * n)
        v = int(m[i]) % t
        out[j % n] = (t - v) % t if j >= n else v
    return out


@pytest.mark.parametrize("bits,nsp", [([40, 40, 40, 41], 1), ([36] * 5 + [37] * 3, 3)])
def test_restatement_bfv_strict_decrypts(bits, nsp):
    """N = 64, t = 257: at the first level and one level below the restatement decrypts to the plaintext under x -> x^g"""
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
    assert np.array_equal(cl.decrypt_bfv(below), m)
    for g in (H.elt_from_step(n, 1), H.elt_from_step(n, -5), 2 * n - 1, 3):
        key = cl.galois_key(g)
        want = _galois_plain(m, g, n, t)
        for ct in (top, below):
            k = ct.shape[1]
            out = H.hoisted_rotation(ref, k, ct, g, key)
            assert np.array_equal(cl.decrypt_bfv(out), want), (g, k)
            seq = ct.copy()
            assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(seq), g, O.ptr(key)) == 0
            assert np.array_equal(cl.decrypt_bfv(seq), want), (g, k)
            assert not np.array_equal(seq, out), (g, k)  # same plaintext, other words: the mod-up does not commute


def _ckks_error(cl, ct, want):
    k = ct.shape[1]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
    got, _ = cl.centered_from_ntt_rows(dot)
    return max(abs(a - b) for a, b in zip(got, want))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits,nsp", [([40, 40, 40, 41], 1), ([36] * 4 + [37] * 2, 2)])
def test_restatement_ckks_error_of_the_sequential_rotation(bits, nsp, mode):
    """err_hoisted <= 2 * err_sequential + 1 on the same ciphertext and key: both noise terms have the same bound, the
    factor 2 covers one sample's spread"""
    logn, n = 6, 64
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, logn, mods, nsp=nsp, t=0, mode=mode)
    cl = O.Client(ref, seed=5)
    L = O.lib()
    rng = np.random.default_rng(17 + nsp)
    msg = [int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=n)]
    ct = cl.encrypt_poly_ntt(msg)
    for g in (H.elt_from_step(n, 1), H.elt_from_step(n, -5), 2 * n - 1, 3):
        key = cl.galois_key(g)
        want = [0] * n
        for i in range(n):
            j = (i * g) % (2 * n)
            want[j % n] = -msg[i] if j >= n else msg[i]
        for k in (cl.k, cl.k - 1):
            c = np.ascontiguousarray(ct[:, :k])  # (CKKS mod_switch_to_next drops the last prime)
            out = H.hoisted_rotation(ref, k, c, g, key)
            seq = c.copy()
            assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(seq), g, O.ptr(key)) == 0
            e_h, e_s = _ckks_error(cl, out, want), _ckks_error(cl, seq, want)
            print("ckks nsp=%d mode=%d g=%d k=%d: hoisted %d sequential %d" % (nsp, mode, g, k, e_h, e_s))
            assert e_h <= 2 * e_s + 1, (g, k, e_h, e_s)
            assert not np.array_equal(seq, out)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_hoist_check.cpp", link_sealhip=True)
    assert "host-only hoist checks ok" in run_exe(exe, "host", timeout=120)
