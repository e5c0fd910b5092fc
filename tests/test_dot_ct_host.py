"""Ciphertext inner product (sealhip_evaluator_dot_product / _max_terms): what can be checked without
a GPU. The exports and their mirrors; the argument checks on host-only contexts, in the header's order; the bound on the number
of terms against its Python-integer form; the 128-bit capacity of the kernel's sums (tests/dot_ct_bounds_check.cpp); and the CPU
restatement (tests/dot_ct_ref.py) itself: one term is ref_bfv_multiply, 17 terms decrypt to sum m_a m_b."""
import ctypes as C
import os

import numpy as np
import pytest

import dot_ct_ref as D
import noise_ref as R
import oracle_lib as O
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_dot_product", "sealhip_evaluator_dot_product_max_terms")
T39 = (1 << 39) + 1
# (log n, prime bits, t, k) -> room, max_terms: the table of DESIGN.md section 18
TABLE = [
    (15, [55] * 8, 786433, 7, 56, (1 << 56) - 1),
    (16, [50] * 16, 786433, 15, 170, (1 << 64) - 1),
    (12, [36, 36, 37], 786433, 2, 72, (1 << 64) - 1),
    (12, [59] * 7, T39, 6, 10, 1023),
    (15, [59] * 7, T39, 6, 7, 127),
]


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("dot_product", "dot_product_max_terms"):
        assert callable(getattr(S.Evaluator, name))
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert name in header


def _call(L, ctx, k=2, a=None, b=None, n_terms=1, count=1, keys=None, n_keys=0, out=0x3000000):
    """one term at two made-up device addresses far from `out` unless told otherwise (nothing is dereferenced on the host)"""
    a = [0x1000000] * n_terms if a is None else a
    b = [0x2000000] * n_terms if b is None else b
    pa = (C.c_void_p * max(1, len(a)))(*a) if a is not False else None
    pb = (C.c_void_p * max(1, len(b)))(*b) if b is not False else None
    return L.sealhip_evaluator_dot_product(ctx, k, pa, pb, n_terms, count, keys, n_keys, out)


def test_entries_on_host_only_context():
    """E_POINTER first; then the level, BFV PARITY, an empty term list, too many terms, keys given but none counted and an
    overlap (E_INVALIDARG); then the empty batch (S_OK); then the host-only context (COR_E_INVALIDOPERATION). A key handle
    cannot exist without a device, so the check that looks INTO a key -- its digit count -- is in tests/test_gpu_dot_ct.py."""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    parity = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, device=-1)
    strict = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    L = S.lib()
    ok = (strict.handle, ckks.handle)
    nokey = (C.c_void_p * 1)(None)
    somekey = (C.c_void_p * 1)(0x4000000)  # (never read: the refusals below come first)
    mt = C.c_uint64(0)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG)
    for h in ok + (parity.handle,):
        for kw in ({"out": None}, {"a": False}, {"b": False}, {"a": [None]}, {"b": [None]}, {"a": [0x1000000, None], "n_terms": 2},
                   {"keys": nokey, "n_keys": 1}):
            with pytest.raises(TypeError):
                S._check(_call(L, h, k=9, **kw))
        with pytest.raises(TypeError):
            S._check(L.sealhip_evaluator_dot_product_max_terms(h, 9, None))
    with pytest.raises(TypeError):
        S._check(_call(L, None))
    with pytest.raises(TypeError):
        S._check(L.sealhip_evaluator_dot_product_max_terms(None, 1, C.byref(mt)))
    # 2. invalid arguments, also for an empty batch: the level (k = 3 is the key level of these contexts)
    for h in ok:
        for k in (0, 3, 4, 5):
            for count in (1, 0):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(_call(L, h, k=k, count=count))
            with pytest.raises(ValueError, match="level k out of range"):
                S._check(L.sealhip_evaluator_dot_product_max_terms(h, k, C.byref(mt)))
        with pytest.raises(ValueError, match="must not be empty"):
            S._check(_call(L, h, n_terms=0, count=1))
        for count in (1, 0):
            with pytest.raises(ValueError, match="not enough relinearization keys"):
                S._check(_call(L, h, keys=somekey, n_keys=0, count=count))
        # out over an operand: the same address, its last word, and an operand that starts inside out
        poly = 2 * n
        for out_words in (3 * poly,):  # (no keys: out is a size-3 batch)
            base = 0x1000000
            for a, b, out in (([base], None, base), (None, [base], base), ([base], None, base + (2 * poly - 1) * 8),
                              ([base + (out_words - 1) * 8], None, base), ([0x5000000, base], [0x6000000, 0x7000000], base)):
                with pytest.raises(ValueError, match="overlap"):
                    S._check(_call(L, h, a=a, b=b, n_terms=len(a or b), out=out))
            # ... and right next to it is fine (refused only as host-only)
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_call(L, h, a=[base], out=base + 2 * poly * 8))
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_call(L, h, a=[base + out_words * 8], out=base))
    for count, n_terms in ((1, 1), (0, 1), (1, 0), (0, 0)):
        with pytest.raises(ValueError, match="STRICT"):
            S._check(_call(L, parity.handle, count=count, n_terms=n_terms))
    # 3. nothing to do: S_OK, no device needed (an empty term list is fine with an empty batch)
    for h in ok:
        for k in (1, 2):
            assert _call(L, h, k=k, count=0) == 0 and _call(L, h, k=k, count=0, n_terms=0) == 0
    # 4. a valid call with work to do is refused as host-only
    for h in ok:
        for n_terms in (1, 17, 40):
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_call(L, h, n_terms=n_terms))
    # CKKS admits 2^32 - 1 terms
    assert S.Evaluator(ckks).dot_product_max_terms(2) == (1 << 32) - 1


@pytest.mark.parametrize("logn,bits,t,k,room,want", TABLE)
def test_max_terms_is_the_python_integer_formula(logn, bits, t, k, room, want):
    """room = bits(prod Bsk) - (bits(t) + log2 N + bits(Q) + 4), max(1, 2^room - 1) saturating: the C++ (hostmath.cpp
    HostRnsTool::dot_max_terms), the Python form (dot_ct_ref.max_terms) and the table of DESIGN.md section 18 agree, and
    8 n t N Q <= prod(Bsk) really holds at the reported count"""
    import sealhip as S

    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits)
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT, device=-1)
    got = S.Evaluator(ctx).dot_product_max_terms(k)
    bsk = D.bsk_primes(n, mods[:k], t)
    py, py_room = D.max_terms(n, mods[:k], bsk, t)
    print("logn %d k %d: room %d max_terms %d" % (logn, k, py_room, got))
    assert (got, py_room) == (py, room) and got == want
    Q, M = R.prod(mods[:k]), R.prod(bsk)
    assert 8 * min(got, (1 << 64) - 1) * t * n * Q <= M
    # the boundary, through the entry itself: max_terms accepted (refused only as host-only), one more refused
    if got < (1 << 20):
        L = S.lib()
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(_call(L, ctx.handle, k=k, n_terms=got))
        with pytest.raises(ValueError, match="too many terms"):
            S._check(_call(L, ctx.handle, k=k, n_terms=got + 1))
        with pytest.raises(ValueError, match="too many terms"):
            S._check(_call(L, ctx.handle, k=k, n_terms=got + 1, count=0))


def test_one_term_is_bfv_multiply():
    logn, n, t = 8, 256, 65537
    mods = O.coeff_modulus_create(n, [40, 40, 40, 40])
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    rng = np.random.default_rng(1)
    L = O.lib()
    for k in (3, 2, 1):
        a = np.stack([rng.integers(0, p, size=(2, n), dtype=np.uint64) for p in mods[:k]], axis=1)
        b = np.stack([rng.integers(0, p, size=(2, n), dtype=np.uint64) for p in mods[:k]], axis=1)
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        want = np.zeros((3, k, n), dtype=np.uint64)
        assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a), 2, O.ptr(b), 2, O.ptr(want)) == 0
        assert np.array_equal(D.bfv_dot_product(ref, k, [a], [b]), want), k


@pytest.fixture(scope="module")
def seventeen():
    """17 encrypted pairs at N = 2^8 on [40, 40, 41] (k = 2), their one-floor sum and its relinearization"""
    logn, n, t = 8, 256, 65537
    mods = O.coeff_modulus_create(n, [40, 40, 41])
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    cl = O.Client(ref, seed=11)
    rng = np.random.default_rng(17)
    ma = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(17)]
    mb = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(17)]
    a, b = [cl.encrypt_bfv(m) for m in ma], [cl.encrypt_bfv(m) for m in mb]
    want = np.zeros(n, dtype=np.uint64)
    for x, y in zip(ma, mb):
        want = (want + O.negacyclic_mod_t(x, y, t)) % np.uint64(t)
    s3 = D.bfv_dot_product(ref, cl.k, a, b)
    s2 = D.bfv_dot_product(ref, cl.k, a, b, cl.relin_key())
    return ref, cl, a, b, want, s3, s2


def _budget(cl, ct):
    k, size = ct.shape[1], ct.shape[0]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), size, 0, O.ptr(cl.sk_powers(size - 1)),
                                  O.ptr(dot))
    return R.ref_noise_budget(dot, cl.mods[:k], int(cl.ref.c.t))


def test_seventeen_terms_decrypt_before_and_after_relinearization(seventeen):
    ref, cl, a, b, want, s3, s2 = seventeen
    assert s3.shape == (3, cl.k, cl.n) and s2.shape == (2, cl.k, cl.n)
    assert np.array_equal(cl.decrypt_bfv(s3), want)
    assert np.array_equal(cl.decrypt_bfv(s2), want)
    b3, b2 = _budget(cl, s3), _budget(cl, s2)
    print("noise budget of the one-floor sum of 17 products: %d bits, relinearized %d; fresh %d" % (b3, b2, _budget(cl, a[0])))
    assert b3 > 10 and b2 > 10


def test_seventeen_terms_are_not_the_composition_but_close(seventeen):
    """the composition floors per term: other words, the same plaintext, and a noise budget within a bit or two"""
    ref, cl, a, b, want, s3, _ = seventeen
    L = O.lib()
    acc = None
    for x, y in zip(a, b):
        prod = np.zeros((3, cl.k, cl.n), dtype=np.uint64)
        assert L.ref_bfv_multiply(C.byref(ref.c), cl.k, O.ptr(x), 2, O.ptr(y), 2, O.ptr(prod)) == 0
        if acc is None:
            acc = prod
        else:
            nxt = np.zeros_like(acc)
            L.ref_evaluator_add(C.byref(ref.c), cl.k, O.ptr(acc), 3, O.ptr(prod), 3, O.ptr(nxt))
            acc = nxt
    assert np.array_equal(cl.decrypt_bfv(acc), want)
    assert not np.array_equal(acc, s3)
    assert abs(_budget(cl, acc) - _budget(cl, s3)) <= 2


def test_repeated_operands_in_the_restatement(seventeen):
    """a sum of squares and a repeated pair: the lifted operand is shared, the words are those of separate copies"""
    ref, cl, a, b, _, _, _ = seventeen
    got = D.bfv_dot_product(ref, cl.k, [a[0], a[1], a[0]], [a[0], b[1], a[0]])
    want = D.bfv_dot_product(ref, cl.k, [a[0].copy(), a[1].copy(), a[0].copy()], [a[0].copy(), b[1].copy(), a[0].copy()])
    assert np.array_equal(got, want)


def test_ckks_restatement_is_linear_in_the_terms():
    """the CKKS definition is a sum of canonical residues: any order of the terms gives the same words"""
    logn, n = 6, 64
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    ref = O.RefContext(2, logn, mods, nsp=1, t=0, mode=0)
    rng = np.random.default_rng(5)
    k = 3
    terms = [np.ascontiguousarray(np.stack([rng.integers(0, p, size=(2, n), dtype=np.uint64) for p in mods[:k]], axis=1))
             for _ in range(6)]
    x = D.ckks_dot_product(ref, k, terms[:3], terms[3:])
    y = D.ckks_dot_product(ref, k, terms[2::-1], terms[:2:-1])
    assert np.array_equal(x, y)


def test_sum_capacity_bounds_program(tmp_path):
    """ntt_bounds.hpp section 8 (dot_group_admits) and the kernel's accumulation against exact arithmetic"""
    exe = compile_cpp(tmp_path, "dot_ct_bounds_check.cpp")
    assert "dot_ct_bounds_check: OK" in run_exe(exe, timeout=120)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_dot_ct_check.cpp", link_sealhip=True)
    assert "host-only dot_ct checks ok" in run_exe(exe, "host", timeout=120)
