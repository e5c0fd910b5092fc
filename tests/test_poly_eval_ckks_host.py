"""Polynomial evaluation on CKKS ciphertexts with planned levels and scales (sealhip_evaluator_linear_combination_levels /
_polynomial_plan_ckks / _evaluate_polynomial_ckks): what can be checked without a GPU. The exports and
their mirrors; the argument checks on host-only contexts in the header's order; plan and tables from the library against the
Python restatement (tests/poly_eval_ckks_ref.py) bit for bit; the planner header under the sanitizers as a stand-alone program
(tests/poly_plan_check.cpp); and the restatement itself: at N = 64 with data primes alternating 39 and 41 bits and Delta = 2^40
-- treating a prime as Delta anywhere is then an error of order 1 -- the result decrypts to p(message)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import poly_eval_ckks_ref as PC
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_linear_combination_levels", "sealhip_evaluator_polynomial_plan_ckks",
       "sealhip_evaluator_evaluate_polynomial_ckks")


@pytest.fixture(autouse=True, scope="module")
def _library_has_the_entries():
    """the restatement is only meaningful next to the library it restates: every test here needs the exports"""
    import sealhip as S

    for name in NEW:
        assert hasattr(S.lib(), name), name


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS and name in header
    for name in ("linear_combination_levels", "polynomial_plan_ckks", "evaluate_polynomial_ckks"):
        assert callable(getattr(S.Evaluator, name))
    for word in ("CKKS only", "term_levels", "term_sizes", "mod_switch_to any lower level", "tests/poly_eval_ckks_ref.py",
                 "sealhip_poly_plan", "NOT capturable"):
        assert word in header


def _lin(L, ctx, k=2, terms=None, levels=None, sizes=None, n_terms=1, size=2, count=1, weights=0x2000000, constant=None,
         n_sums=1, out=0x3000000):
    """made-up device addresses far apart unless told otherwise (nothing is dereferenced on the host); every term at level k
    and of the sum's size unless told otherwise"""
    terms = [0x1000000] * n_terms if terms is None else terms
    pt = (C.c_void_p * max(1, len(terms)))(*terms) if terms is not False else None
    levels = [k] * n_terms if levels is None else levels
    sizes = [size] * n_terms if sizes is None else sizes
    lv = (C.c_uint32 * max(1, len(levels)))(*levels) if levels is not False else None
    sz = (C.c_uint32 * max(1, len(sizes)))(*sizes) if sizes is not False else None
    return L.sealhip_evaluator_linear_combination_levels(ctx, k, pt, lv, sz, n_terms, size, count, weights, constant, n_sums, out)


@pytest.fixture(scope="module")
def host_contexts():
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 50, 60])  # first level 3, two special primes
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    ckks_strict = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, mode=S.MODE_STRICT, device=-1)
    bfv = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    return S, n, ckks, ckks_strict, bfv


def test_linear_combination_levels_on_host_only_context(host_contexts):
    """E_POINTER first; then the level, the scheme, the terms' levels, the size, the terms' sizes, empty lists and overlaps
    (E_INVALIDARG), each ahead of the ones after it; then the empty batch (S_OK); then the host-only context
    (COR_E_INVALIDOPERATION). Both CKKS modes are served, BFV is not."""
    S, n, ckks, ckks_strict, bfv = host_contexts
    L = S.lib()
    served = (ckks.handle, ckks_strict.handle)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG, and so would the BFV context)
    for h in served + (bfv.handle,):
        for kw in ({"out": None}, {"weights": None}, {"terms": False}, {"terms": [None]}, {"levels": False}, {"sizes": False},
                   {"terms": [0x1000000, None], "n_terms": 2}):
            with pytest.raises(TypeError):
                S._check(_lin(L, h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(_lin(L, None))
    # 2. invalid arguments, also for an empty batch
    for count in (1, 0):
        for h in served + (bfv.handle,):
            for k in (0, 4, 5, 6):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(_lin(L, h, k=k, count=count))
        # the scheme, ahead of everything about the terms
        with pytest.raises(ValueError, match="CKKS only"):
            S._check(_lin(L, bfv.handle, levels=[1], size=1, count=count))
        for h in served:
            for levels in ([1], [4], [3, 1], [2, 2, 9]):
                with pytest.raises(ValueError, match="a term's level"):
                    S._check(_lin(L, h, levels=levels, n_terms=len(levels), size=1, count=count))
            for size in (0, 1, 17):
                with pytest.raises(ValueError, match="not valid for encryption parameters"):
                    S._check(_lin(L, h, size=size, sizes=[5], count=count))
            for sizes, size in (([1], 2), ([3], 2), ([2, 4], 3), ([3, 3, 0], 3)):
                with pytest.raises(ValueError, match="a term's size"):
                    S._check(_lin(L, h, sizes=sizes, n_terms=len(sizes), size=size, n_sums=0, count=count))
    for h in served:
        with pytest.raises(ValueError, match="must not be empty"):
            S._check(_lin(L, h, n_terms=0))
        with pytest.raises(ValueError, match="must not be empty"):
            S._check(_lin(L, h, n_sums=0))
        # out over a term (whose extent is its OWN size and level), over the weights, over the constant; two sums of size 3
        base, k = 0x1000000, 2
        item = 3 * k * n
        out_words = 2 * item
        term_words = 2 * 3 * n  # a size-2 term at level 3
        for kw in ({"terms": [base], "out": base}, {"terms": [base], "out": base + (term_words - 1) * 8},
                   {"terms": [base + (out_words - 1) * 8], "out": base}, {"weights": base, "out": base - (out_words - 1) * 8},
                   {"weights": base - (2 * 1 * k - 1) * 8, "out": base}, {"constant": base + (out_words - 1) * 8, "out": base}):
            kw = dict({"size": 3, "n_sums": 2, "levels": [3], "sizes": [2]}, **kw)
            kw.setdefault("terms", [0x7000000])
            with pytest.raises(ValueError, match="overlap"):
                S._check(_lin(L, h, **kw))
        # ... and right next to it is fine (refused only as host-only)
        for kw in ({"terms": [base], "out": base + term_words * 8}, {"terms": [base + out_words * 8], "out": base},
                   {"weights": base + out_words * 8, "out": base}, {"constant": base - 2 * k * 8, "out": base}):
            kw = dict({"size": 3, "n_sums": 2, "levels": [3], "sizes": [2]}, **kw)
            kw.setdefault("terms", [0x7000000])
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_lin(L, h, **kw))
    # 3. nothing to do: S_OK, no device needed (empty lists are fine with an empty batch)
    for h in served:
        for k in (1, 3):
            assert _lin(L, h, k=k, count=0) == 0 and _lin(L, h, k=k, count=0, n_terms=0, n_sums=0) == 0
        assert _lin(L, h, k=1, count=0, levels=[3, 1], sizes=[2, 3], n_terms=2, size=3) == 0
    # 4. a valid call with work to do is refused as host-only
    for h in served:
        for n_terms, n_sums in ((1, 1), (17, 9), (40, 3)):
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_lin(L, h, k=1, levels=[1 + i % 3 for i in range(n_terms)], sizes=[2 + i % 2 for i in range(n_terms)],
                              n_terms=n_terms, size=3, n_sums=n_sums, constant=0x4000000))


# ---------------------------------------------------------------- the plan query and the evaluation's checks
def _plan(L, ctx, k=3, scale=2.0 ** 40, coeffs=(1.0, 2.0, 3.0), degree=None, basis=0, n_baby=0, scale_out=0.0, plan=True,
          w=None, kc=None):
    import sealhip as S

    ca = (C.c_double * max(1, len(coeffs)))(*coeffs) if coeffs is not None else None
    degree = len(coeffs) - 1 if degree is None else degree
    pl = S.PolyPlan()
    return L.sealhip_evaluator_polynomial_plan_ckks(ctx, k, scale, ca, degree, basis, n_baby, scale_out,
                                                    C.addressof(pl) if plan else None, w, kc)


def _eval(L, ctx, k=3, ct=0x1000000, count=1, scale=2.0 ** 40, coeffs=(1.0, 2.0, 3.0), degree=None, basis=0, n_baby=0,
          scale_out=0.0, keys=None, n_keys=0, out=0x3000000):
    ca = (C.c_double * max(1, len(coeffs)))(*coeffs) if coeffs is not None else None
    degree = len(coeffs) - 1 if degree is None else degree
    return L.sealhip_evaluator_evaluate_polynomial_ckks(ctx, k, ct, count, scale, ca, degree, basis, n_baby, scale_out, keys,
                                                        n_keys, out, None, None)


def test_plan_and_evaluate_check_order_on_host_only_context(host_contexts):
    """E_POINTER first; then the level, the scheme, the scale, the coefficients, the basis, the degree, n_baby, the length of
    the chain, the keys and the overlap (E_INVALIDARG), each ahead of the ones after it; then the empty batch; then the
    host-only context. The plan query answers on a host-only context. (A key handle cannot exist without a device: the check
    that looks INTO a key is in tests/test_gpu_poly_eval_ckks.py.)"""
    S, n, ckks, ckks_strict, bfv = host_contexts
    L = S.lib()
    nan, inf = float("nan"), float("inf")
    nokey = (C.c_void_p * 1)(None)
    somekey = (C.c_void_p * 1)(0x4000000)  # (never read: the refusals below come first)
    calls = (lambda h, **kw: _plan(L, h, **kw), lambda h, **kw: _eval(L, h, **kw), lambda h, **kw: _eval(L, h, count=0, **kw))
    # 1. null pointers
    for h in (ckks.handle, bfv.handle):
        for kw in ({"coeffs": None, "degree": 2}, {"plan": False}):
            with pytest.raises(TypeError):
                S._check(_plan(L, h, k=9, **kw))
        for kw in ({"out": None}, {"ct": None}, {"coeffs": None, "degree": 2}, {"keys": nokey, "n_keys": 1}):
            with pytest.raises(TypeError):
                S._check(_eval(L, h, k=9, **kw))
    with pytest.raises(TypeError):
        S._check(_plan(L, None))
    with pytest.raises(TypeError):
        S._check(_eval(L, None))
    # 2. invalid arguments, each ahead of the ones after it, for the plan, the evaluation and the evaluation of an empty batch
    for call in calls:
        for h in (ckks.handle, ckks_strict.handle, bfv.handle):
            for k in (0, 4, 5):
                with pytest.raises(ValueError, match="level k out of range"):
                    S._check(call(h, k=k, scale=nan))
        with pytest.raises(ValueError, match="CKKS only"):
            S._check(call(bfv.handle, scale=nan))
        for h in (ckks.handle, ckks_strict.handle):
            for scale in (nan, inf, 0.0, -1.0):
                with pytest.raises(ValueError, match="scale out of bounds"):
                    S._check(call(h, scale=scale, coeffs=(1.0, nan)))
            for scale_out in (nan, inf, -1.0):
                with pytest.raises(ValueError, match="scale out of bounds"):
                    S._check(call(h, scale_out=scale_out, coeffs=(1.0, nan)))
            for coeffs in ((1.0, nan), (inf, 1.0), (1.0, 2.0, -inf, 0.0)):
                with pytest.raises(ValueError, match="not finite"):
                    S._check(call(h, coeffs=coeffs, basis=2))
            for basis in (2, 7):
                with pytest.raises(ValueError, match="basis"):
                    S._check(call(h, coeffs=(5.0,), basis=basis))
            for coeffs in ((5.0,), (5.0, 0.0, 0.0), (0.0,)):
                with pytest.raises(ValueError, match="constant"):
                    S._check(call(h, coeffs=coeffs, n_baby=1))
            for coeffs, n_baby in (((1.0, 2.0, 3.0), 1), ((1.0, 2.0, 3.0), 4), ((1.0, 2.0, 3.0, 0.0, 0.0), 4), ((1.0, 2.0), 3)):
                with pytest.raises(ValueError, match="n_baby"):
                    S._check(call(h, coeffs=coeffs, n_baby=n_baby, k=1))
            # the chain: degree 1 takes one level, degree 2 two, degree 7 (m = 3, g = 3) four
            for k, coeffs in ((1, (1.0, 2.0)), (2, (1.0, 2.0, 3.0)), (3, [1.0] * 8)):
                with pytest.raises(ValueError, match="end of modulus switching chain reached"):
                    S._check(call(h, k=k, coeffs=coeffs))
    for h in (ckks.handle, ckks_strict.handle):
        for count in (1, 0):
            with pytest.raises(ValueError, match="not enough relinearization keys"):
                S._check(_eval(L, h, count=count, out=0x1000000))
            with pytest.raises(ValueError, match="not enough relinearization keys"):
                S._check(_eval(L, h, keys=somekey, n_keys=0, count=count, out=0x1000000))
        # degree one needs no key: the overlap check is reached (ct is 2 x 3 x n words, out 2 x 2 x n)
        base, ct_words, out_words = 0x1000000, 2 * 3 * n, 2 * 2 * n
        for out in (base, base + (ct_words - 1) * 8, base - (out_words - 1) * 8):
            with pytest.raises(ValueError, match="overlap"):
                S._check(_eval(L, h, coeffs=(3.0, 4.0), ct=base, out=out))
        for out in (base + ct_words * 8, base - out_words * 8):
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(_eval(L, h, coeffs=(3.0, 4.0, 0.0), ct=base, out=out))
        # 3. nothing to do, 4. host-only; the plan query answers
        assert _eval(L, h, coeffs=(3.0, 4.0), count=0) == 0
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(_eval(L, h, coeffs=(0.0, 4.0), n_baby=2))
        assert _plan(L, h) == 0 and _plan(L, h, coeffs=(3.0, 4.0), k=2) == 0


# ---------------------------------------------------------------- plan and tables, bit for bit
BITS = [39, 41] * 6 + [42]  # twelve data primes alternating 39 and 41 bits, one special prime
_rng = np.random.default_rng(21)
PLAN_CASES = {
    "d1": (list(_rng.uniform(-1, 1, 2)), 0),
    "d2": (list(_rng.uniform(-1, 1, 3)), 0),
    "d3": (list(_rng.uniform(-1, 1, 4)), 0),
    "d5 m2": (list(_rng.uniform(-1, 1, 6)), 2),
    "d7 auto": (list(_rng.uniform(-1, 1, 8)), 0),                                   # m = 3, g = 3
    "d8 m3": (list(_rng.uniform(-1, 1, 9)), 3),
    "d20 m4 zero chunk": ([0.0 if 8 <= e <= 11 else float(v) for e, v in enumerate(_rng.uniform(-1, 1, 21))], 4),
    "d3 coefficient 1e6": ([0.5, 1.0e6, -0.25, 1.0e6], 0),      # a weight of 2^61 under a 41-bit prime, constants of 2^80
    "d3 coefficient 1e7": ([0.5, 1.0e7, -0.25, 1.0e7], 0),      # weights beyond 2^64
    "d15": (list(_rng.uniform(-1, 1, 16)), 0),
    "trailing zeros": (list(_rng.uniform(-1, 1, 6)) + [0.0, 0.0], 3),
}


@pytest.fixture(scope="module")
def plan_context():
    import sealhip as S

    mods = O.coeff_modulus_create(64, BITS)
    ctx = S.Context(S.SCHEME_CKKS, 6, mods, 1, 0, device=-1)
    return S, mods, S.Evaluator(ctx)


@pytest.mark.parametrize("basis", [0, 1])
@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_and_tables_equal_the_restatement(plan_context, case, basis):
    S, mods, ev = plan_context
    coeffs, n_baby = PLAN_CASES[case]
    for k, scale, scale_out in ((12, 2.0 ** 40, 0.0), (11, 2.0 ** 40 * 1.0001, 2.0 ** 38)):
        want = PC.plan(mods[:12], k, scale, coeffs, basis, n_baby, scale_out)
        got = ev.polynomial_plan_ckks(k, scale, coeffs, basis, n_baby, scale_out)
        for name in ("d", "m", "g", "out_level", "n_products"):
            assert got[name] == want[name], (case, name)
        assert got["inner_level"] == want["L_in"]
        assert np.float64(got["out_scale"]).tobytes() == np.float64(want["out_scale"]).tobytes()
        assert np.array_equal(got["weights"], want["W"]), case
        assert np.array_equal(got["constants"], want["K"]), case
        assert got["temp_bytes_per_item"] > 0 and got["temp_bytes_per_item"] % (8 * 64) == 0
        formed = [0] + want["J"]
        for j in range(want["g"]):
            assert (j in formed) or not (got["weights"][j].any() or got["constants"][j].any())
    if case.startswith("d3 coefficient"):
        pl = PC.plan(mods[:12], 12, 2.0 ** 40, coeffs, basis, n_baby, 0.0)
        up = pl["tau"][0] * float(mods[pl["L_in"] - 1])
        assert abs(coeffs[0] * up) > 2.0 ** 62  # (every constant is far beyond 2^62)
        assert abs(coeffs[1] * (up / pl["sc"][1])) > (2.0 ** 64 if "1e7" in case else 2.0 ** 60)
    if case == "d20 m4 zero chunk" and basis == 0:
        assert PC.plan(mods[:12], 12, 2.0 ** 40, coeffs, 0, 4)["J"] == [1, 3, 4, 5]


def test_chebyshev_chunks_reproduce_chebval():
    """the T_m-adic expansion is p: sum_j r_j(x) T_m(x)^j against numpy's chebval to 1e-13 (relative to sum |c_e|) for d <= 63"""
    rng = np.random.default_rng(5)
    x = np.linspace(-1, 1, 41)
    for d, m in ((1, 2), (7, 3), (8, 3), (20, 4), (31, 6), (63, 8)):
        c = list(rng.uniform(-1, 1, d + 1))
        g = (d + m) // m
        chunks = PC.chunks_of(c, d, m, g, 1)
        tm = np.polynomial.chebyshev.chebval(x, [0.0] * m + [1.0])
        acc = sum(np.polynomial.chebyshev.chebval(x, ch) * tm ** j for j, ch in enumerate(chunks))
        err = np.max(np.abs(acc - np.polynomial.chebyshev.chebval(x, c)))
        assert err <= 1e-13 * sum(abs(v) for v in c), (d, m, err)


def test_planner_program_under_sanitizers(tmp_path):
    """gemini-seal_amd/csrc/poly_plan.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = compile_cpp(tmp_path, "poly_plan_check.cpp", sanitize=True)
    assert "poly_plan_check: OK" in run_exe(exe, timeout=120)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_poly_eval_ckks_check.cpp", link_sealhip=True)
    assert "host-only poly_eval_ckks checks ok" in run_exe(exe, "host", timeout=120)


# ---------------------------------------------------------------- decryption
def _bar(e_call, e_comp):
    return e_call <= 2 * e_comp + 1


def _ring_eval(coeffs, basis, msg):
    """p(msg) in R[X]/(X^N + 1), floating point"""
    n = len(msg)

    def mul(a, b):
        full = np.convolve(a, b)
        out = full[:n].copy()
        out[:n - 1] -= full[n:]
        return out

    one = np.zeros(n)
    one[0] = 1.0
    acc = np.zeros(n)
    if basis == 0:
        power = one
        for c in coeffs:
            acc = acc + c * power
            power = mul(power, msg)
        return acc
    t_prev, t_cur = one, np.array(msg, dtype=float)
    acc = coeffs[0] * t_prev
    for c in coeffs[1:]:
        acc = acc + c * t_cur
        t_prev, t_cur = t_cur, 2.0 * mul(msg, t_cur) - t_prev
    return acc


def _decrypt(cl, ct, scale):
    """(c_0 + c_1 s) / scale as floats, from the CRT over the ciphertext's rows"""
    L = O.lib()
    k = ct.shape[1]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    L.ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(ct), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
    centred, _ = cl.centered_from_ntt_rows(dot)
    return np.array([v / scale for v in centred])


DELTA = 2.0 ** 40
_MESSAGES = {"constant": {0: 0.37}, "four": {0: 0.3, 1: -0.25, 5: 0.2, 17: 0.15}}  # l1 norm at most 1


@pytest.fixture(scope="module")
def crypto():
    out = {}
    for mode in (0, 1):
        mods = O.coeff_modulus_create(64, BITS[:8] + BITS[-1:])  # eight data primes
        ref = O.RefContext(2, 6, mods, nsp=1, t=0, mode=mode)
        cl = O.Client(ref, seed=40 + mode)
        out[mode] = (ref, cl, cl.relin_key())
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("basis", [0, 1])
@pytest.mark.parametrize("d", [3, 7, 15])
def test_decrypts_to_the_polynomial_of_the_message(crypto, d, basis, mode):
    """within 2^-20 sum |c_e| of the float evaluation in R[X]/(X^N + 1); against composition(), the project's bar
    e_call <= 2 e_comp + 1 in units of 2^-40. Errors measured here (max over the two messages, in units of sum |c_e|):
    see DESIGN.md section 21."""
    ref, cl, key = crypto[mode]
    rng = np.random.default_rng(100 * d + basis)
    coeffs = [float(v) for v in rng.uniform(-1, 1, d + 1)]
    norm = sum(abs(c) for c in coeffs)
    k = cl.k
    for name, msg in _MESSAGES.items():
        m = np.zeros(cl.n)
        for i, v in msg.items():
            m[i] = v
        ct = cl.encrypt_poly_ntt([int(round(v * DELTA)) for v in m])
        want = _ring_eval(coeffs, basis, m)
        pl, words = PC.evaluate(ref, k, ct, DELTA, coeffs, key, basis)
        _, comp = PC.composition(ref, k, ct, DELTA, coeffs, key, basis)
        assert words.shape == (2, pl["out_level"], cl.n) and pl["out_scale"] == DELTA
        e_call = np.max(np.abs(_decrypt(cl, words, pl["out_scale"]) - want))
        e_comp = np.max(np.abs(_decrypt(cl, comp, pl["out_scale"]) - want))
        print("d %d basis %d mode %d %s: call %.3e composition %.3e (units of sum |c_e|: %.3e %.3e)"
              % (d, basis, mode, name, e_call, e_comp, e_call / norm, e_comp / norm))
        assert e_call <= 2.0 ** -20 * norm, (name, e_call, norm)
        assert _bar(e_call * DELTA, e_comp * DELTA), (name, e_call, e_comp)
