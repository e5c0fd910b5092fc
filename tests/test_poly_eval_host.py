"""Polynomial evaluation on ciphertexts (sealhip_evaluator_linear_combination / _evaluate_polynomial):
what can be checked without a GPU. The exports and their mirrors; the argument checks on host-only contexts, in the header's
order; the 128-bit capacity of the kernel's sums (tests/lincomb_bounds_check.cpp); the C++ adapter's checks; and the CPU
restatement (tests/poly_eval_ref.py) itself: degree one is multiply_plain plus the scaling-variant add, g = 1 is the plain
power-basis sum, and a degree-7 polynomial decrypts to p(m) with noise budget to spare."""
import ctypes as C
import os

import numpy as np
import pytest

import noise_ref as R
import oracle_lib as O
import poly_eval_ref as P
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_linear_combination", "sealhip_evaluator_evaluate_polynomial")


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("linear_combination", "evaluate_polynomial"):
        assert callable(getattr(S.Evaluator, name))
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert name in header
    for word in ("tests/poly_eval_ref.py", "NOT capturable", "capturable after one warm-up call"):
        assert word in header


def _lin(L, ctx, k=2, terms=None, n_terms=1, size=2, count=1, weights=0x2000000, constant=None, n_sums=1, out=0x3000000):
    """made-up device addresses far apart unless told otherwise (nothing is dereferenced on the host)"""
    terms = [0x1000000] * n_terms if terms is None else terms
    pt = (C.c_void_p * max(1, len(terms)))(*terms) if terms is not False else None
    return L.sealhip_evaluator_linear_combination(ctx, k, pt, n_terms, size, count, weights, constant, n_sums, out)


def _poly(L, ctx, k=2, ct=0x1000000, count=1, coeffs=(1, 2, 3), degree=None, n_baby=0, keys=None, n_keys=0, out=0x3000000):
    ca = (C.c_uint64 * max(1, len(coeffs)))(*coeffs) if coeffs is not None else None
    degree = len(coeffs) - 1 if degree is None else degree
    return L.sealhip_evaluator_evaluate_polynomial(ctx, k, ct, count, ca, degree, n_baby, keys, n_keys, out)


@pytest.fixture(scope="module")
def host_contexts():
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    parity = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, device=-1)
    strict = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    return S, n, parity, strict, ckks


def test_linear_combination_on_host_only_context(host_contexts):
    """E_POINTER first; then the level, the size, empty lists and overlaps (E_INVALIDARG); then the empty batch (S_OK); then the
    host-only context (COR_E_INVALIDOPERATION). Both schemes and both BFV modes are served."""
    S, n, parity, strict, ckks = host_contexts
    L = S.lib()
    every = (strict.handle, ckks.handle, parity.handle)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG)
    for h in every:
        for kw in ({"out": None}, {"weights": None}, {"terms": False}, {"terms": [None]}, {"terms": [0x1000000, None], "n_terms": 2}):
            with pytest.raises(TypeError):
                S._check(_lin(L, h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(_lin(L, None))
    # 2. invalid arguments, also for an empty batch (k = 3 is the key level of these contexts)
    for h in every:
        for k in (0, 3, 4, 5):
            for count in (1, 0):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(_lin(L, h, k=k, count=count))
        for size in (0, 1, 17):
            for count in (1, 0):
                with pytest.raises(ValueError, match="not valid for encryption parameters"):
                    S._check(_lin(L, h, size=size, count=count))
        with pytest.raises(ValueError, match="must not be empty"):
            S._check(_lin(L, h, n_terms=0))
        with pytest.raises(ValueError, match="must not be empty"):
            S._check(_lin(L, h, n_sums=0))
        # out over a term, over the weights, over the constant; two sums of size 3 at k = 2
        base, item, k = 0x1000000, 3 * 2 * n, 2
        out_words = 2 * item
        for kw in ({"terms": [base], "out": base}, {"terms": [base], "out": base + (item - 1) * 8},
                   {"terms": [base + (out_words - 1) * 8], "out": base}, {"terms": [0x5000000, base], "n_terms": 2, "out": base},
                   {"weights": base, "out": base - (out_words - 1) * 8}, {"weights": base - (2 * 1 * k - 1) * 8, "out": base},
                   {"constant": base + (out_words - 1) * 8, "out": base}):
            kw = dict({"size": 3, "n_sums": 2}, **kw)
            kw.setdefault("terms", [0x7000000])
            with pytest.raises(ValueError, match="overlap"):
                S._check(_lin(L, h, **kw))
        # ... and right next to it is fine (refused only as host-only)
        for kw in ({"terms": [base], "out": base + item * 8}, {"terms": [base + out_words * 8], "out": base},
                   {"weights": base + out_words * 8, "out": base}, {"constant": base - 2 * k * 8, "out": base}):
            kw = dict({"size": 3, "n_sums": 2}, **kw)
            kw.setdefault("terms", [0x7000000])
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_lin(L, h, **kw))
    # 3. nothing to do: S_OK, no device needed (empty lists are fine with an empty batch)
    for h in every:
        for k in (1, 2):
            assert _lin(L, h, k=k, count=0) == 0 and _lin(L, h, k=k, count=0, n_terms=0, n_sums=0) == 0
    # 4. a valid call with work to do is refused as host-only
    for h in every:
        for n_terms, n_sums in ((1, 1), (17, 9), (40, 3)):
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_lin(L, h, n_terms=n_terms, n_sums=n_sums, constant=0x4000000))


def test_evaluate_polynomial_on_host_only_context(host_contexts):
    """E_POINTER first; then the level, the scheme, the mode, the coefficients, the degree, n_baby, the keys and the overlap
    (E_INVALIDARG), in that order; then the empty batch; then the host-only context. A key handle cannot exist without a device,
    so the check that looks INTO a key -- its digit count -- is in tests/test_gpu_poly_eval.py."""
    S, n, parity, strict, ckks = host_contexts
    L = S.lib()
    h = strict.handle
    nokey = (C.c_void_p * 1)(None)
    somekey = (C.c_void_p * 1)(0x4000000)  # (never read: the refusals below come first)
    # 1. null pointers
    for ctx in (h, ckks.handle, parity.handle):
        for kw in ({"out": None}, {"ct": None}, {"coeffs": None, "degree": 2}, {"keys": nokey, "n_keys": 1}):
            with pytest.raises(TypeError):
                S._check(_poly(L, ctx, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(_poly(L, None))
    # 2. invalid arguments, each ahead of the ones after it, also for an empty batch
    for count in (1, 0):
        for k in (0, 3, 4):
            with pytest.raises(ValueError, match="level k out of range"):
                S._check(_poly(L, ckks.handle, k=k, count=count))
        with pytest.raises(ValueError, match="BFV only"):
            S._check(_poly(L, ckks.handle, coeffs=(65537,), count=count))
        with pytest.raises(ValueError, match="STRICT"):
            S._check(_poly(L, parity.handle, coeffs=(65537,), count=count))
        with pytest.raises(ValueError, match="plain modulus"):
            S._check(_poly(L, h, coeffs=(1, 65537, 0), n_baby=1, count=count))
        for coeffs in ((5,), (5, 0, 0), (0,)):
            with pytest.raises(ValueError, match="constant"):
                S._check(_poly(L, h, coeffs=coeffs, n_baby=1, count=count))
        for coeffs, n_baby in (((1, 2, 3), 1), ((1, 2, 3), 4), ((1, 2, 3, 0, 0), 4), ((1, 2), 3)):
            with pytest.raises(ValueError, match="n_baby"):
                S._check(_poly(L, h, coeffs=coeffs, n_baby=n_baby, count=count))
        with pytest.raises(ValueError, match="not enough relinearization keys"):
            S._check(_poly(L, h, count=count, out=0x1000000))
        with pytest.raises(ValueError, match="not enough relinearization keys"):
            S._check(_poly(L, h, keys=somekey, n_keys=0, count=count))
    # degree one needs no key: the overlap check is reached, and a clean call is refused only as host-only
    base, words = 0x1000000, 2 * 2 * n
    for out in (base, base + (words - 1) * 8, base - (words - 1) * 8):
        with pytest.raises(ValueError, match="overlap"):
            S._check(_poly(L, h, coeffs=(3, 4), ct=base, out=out))
    for out in (base + words * 8, base - words * 8):
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(_poly(L, h, coeffs=(3, 4, 0), ct=base, out=out))
    # 3. nothing to do
    for k in (1, 2):
        assert _poly(L, h, k=k, coeffs=(3, 4), count=0) == 0
    # 4. host-only, with every legal n_baby of a degree-one polynomial
    for n_baby in (0, 2):
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(_poly(L, h, coeffs=(0, 4), n_baby=n_baby))


def test_too_many_outer_terms():
    """59-bit primes and a 40-bit t leave room for 1023 terms at N = 2^12 (the table of DESIGN.md section 18): a polynomial with
    n_baby = 2 and 1024 surviving giant steps is refused, one with 1023 passes on to the key check"""
    import sealhip as S

    t = (1 << 39) + 1
    mods = O.coeff_modulus_create(1 << 12, [59] * 7)
    ctx = S.Context(S.SCHEME_BFV, 12, mods, 1, t, mode=S.MODE_STRICT, device=-1)
    assert S.Evaluator(ctx).dot_product_max_terms(6) == 1023
    L = S.lib()
    with pytest.raises(ValueError, match="too many giant steps"):
        S._check(_poly(L, ctx.handle, k=6, coeffs=[1] * (2 * 1025), n_baby=2))
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        S._check(_poly(L, ctx.handle, k=6, coeffs=[1] * (2 * 1024), n_baby=2))
    # (inner sums that are identically zero do not count: 1034 giant steps, 1023 of them alive)
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        S._check(_poly(L, ctx.handle, k=6, coeffs=[1] * (2 * 1023) + [0] * 20 + [1, 1], n_baby=2))


def test_sum_capacity_bounds_program(tmp_path):
    """ntt_bounds.hpp lincomb_group_admits and the kernel's accumulation against exact arithmetic"""
    exe = compile_cpp(tmp_path, "lincomb_bounds_check.cpp")
    assert "lincomb_bounds_check: OK" in run_exe(exe, timeout=120)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_poly_eval_check.cpp", link_sealhip=True)
    assert "host-only poly_eval checks ok" in run_exe(exe, "host", timeout=120)


# ---------------------------------------------------------------- the restatement itself
def test_shapes():
    assert P.shape([1, 2, 3, 4, 5, 6, 7, 8])[1:] == (7, 3, 3)
    assert P.shape([1] * 9, 3)[1:] == (8, 3, 3)
    assert P.shape([1] * 10, 10)[1:] == (9, 10, 1)
    assert P.shape([1] * 21, 4)[1:] == (20, 4, 6)
    assert P.shape([1, 2, 0, 0])[1:] == (1, 2, 1)
    assert P.shape([1] * 16)[1:] == (15, 4, 4) and P.shape([1] * 17)[1:] == (16, 5, 4)


@pytest.fixture(scope="module")
def session():
    """N = 2^8, t = 65537, six primes [40]*5 + [41] (k = 5): four multiplication depths and the scalar weights fit"""
    logn, n, t = 8, 256, 65537
    mods = O.coeff_modulus_create(n, [40] * 5 + [41])
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    cl = O.Client(ref, seed=20)
    rng = np.random.default_rng(20)
    m = rng.integers(0, t, size=n, dtype=np.uint64)
    return ref, cl, rng, m, cl.encrypt_bfv(m), cl.relin_key()


def _budget(cl, ct):
    k, size = ct.shape[1], ct.shape[0]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), size, 0, O.ptr(cl.sk_powers(size - 1)),
                                  O.ptr(dot))
    return R.ref_noise_budget(dot, cl.mods[:k], int(cl.ref.c.t))


def _plain_eval(m, coeffs, t):
    """p(m) mod (x^N + 1, t) by Horner with negacyclic_mod_t"""
    n = len(m)
    acc = np.zeros(n, dtype=np.uint64)
    for c in reversed(coeffs):
        acc = O.negacyclic_mod_t(acc, m, t)
        acc[0] = (int(acc[0]) + int(c)) % t
    return acc


def test_degree_one_is_multiply_plain_plus_scaling_variant(session):
    ref, cl, rng, m, ct, key = session
    L, k, n = O.lib(), cl.k, cl.n
    for c0, c1 in ((123, 40000), (0, 7), (65536, 1)):
        want = ct.copy()
        plain = np.zeros(n, dtype=np.uint64)
        plain[0] = c1
        assert L.ref_multiply_plain(C.byref(ref.c), k, O.ptr(want), 2, O.ptr(plain)) == 0
        plain[0] = c0
        L.ref_multiply_add_plain_with_scaling_variant(C.byref(ref.c), k, O.ptr(plain), 0, O.ptr(want[0]))
        got = P.evaluate_polynomial(ref, k, ct, [c0, c1])
        assert np.array_equal(got, want)
        # ... and the two tables say the same: w(c) B_1 + K(c) with the oracle's scalar product
        t = int(ref.c.t)
        lin = P.linear_combination(ref, k, [ct], [[P.bfv_weight(c1, t, cl.mods[:k])]], [P.bfv_constant(ref, k, c0)])
        assert np.array_equal(lin[0], want)


def test_one_giant_step_is_the_power_basis_sum(session):
    ref, cl, rng, m, ct, key = session
    k, t = cl.k, int(ref.c.t)
    coeffs = [int(v) for v in rng.integers(0, t, size=5)]
    got = P.evaluate_polynomial(ref, k, ct, coeffs, key, n_baby=5)
    assert P.shape(coeffs, 5)[3] == 1
    powers = {1: ct}
    for e in range(2, 5):
        powers[e] = P._product(ref, k, powers[(e + 1) // 2], powers[e // 2], key)
    want = P.inner_sum(ref, k, powers, coeffs)
    assert np.array_equal(got, want)
    assert np.array_equal(cl.decrypt_bfv(got), _plain_eval(m, coeffs, t))


@pytest.mark.parametrize("case", ["random", "sparse"])
def test_degree_seven_decrypts_to_p_of_m(session, case):
    """d = 7: m = 3, g = 3. `sparse` has zero coefficients inside and an inner sum (c_3, c_4, c_5) that is identically zero."""
    ref, cl, rng, m, ct, key = session
    k, t = cl.k, int(ref.c.t)
    coeffs = [int(v) for v in np.random.default_rng(7).integers(1, t, size=8)]
    if case == "sparse":
        for e in (1, 3, 4, 5):
            coeffs[e] = 0
    assert P.shape(coeffs)[1:] == (7, 3, 3)
    got = P.evaluate_polynomial(ref, k, ct, coeffs, key)
    comp = P.composition(ref, k, ct, coeffs, key)
    want = _plain_eval(m, coeffs, t)
    assert np.array_equal(cl.decrypt_bfv(got), want)
    assert np.array_equal(cl.decrypt_bfv(comp), want)
    b_got, b_comp = _budget(cl, got), _budget(cl, comp)
    print("%s d = 7: noise budget of the restatement %d bits, of the composition %d bits, fresh %d" %
          (case, b_got, b_comp, _budget(cl, ct)))
    assert b_got > 10
