"""Towards CKKS bootstrapping: what can be checked without a GPU. The exports and their mirrors; the
EvalMod coefficients against numpy's Chebyshev interpolation and in a float64 model of ModRaise + EvalMod; the plan from the
library against the restatement (tests/bootstrap_ref.py over tests/poly_eval_ckks_ref.py) bit for bit; the planner header under
the sanitizers as a stand-alone program (tests/evalmod_plan_check.cpp); the argument checks of mod_raise, double_angle and
eval_mod on host-only contexts in the header's order."""
import ctypes as C
import os

import numpy as np
import pytest
from numpy.polynomial import chebyshev as NC

import bootstrap_ref as B
import oracle_lib as O
import poly_eval_ckks_ref as PC
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_mod_raise", "sealhip_evaluator_double_angle", "sealhip_evalmod_coeffs",
       "sealhip_evaluator_evalmod_plan", "sealhip_evaluator_eval_mod", "sealhip_evaluator_bootstrap_plan",
       "sealhip_bootstrap_tables_create", "sealhip_bootstrap_tables_destroy", "sealhip_bootstrap_tables_plan",
       "sealhip_evaluator_bootstrap")
GRID = np.linspace(-1.0, 1.0, 20001)


@pytest.fixture(scope="module")
def S():
    import sealhip

    for name in NEW:
        assert hasattr(sealhip.lib(), name), name
    return sealhip


def test_new_exports_exist(S):
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert name in S.SYMBOLS and name in header
    for name in ("mod_raise", "double_angle", "evalmod_plan", "eval_mod", "bootstrap_plan", "bootstrap"):
        assert callable(getattr(S.Evaluator, name))
    assert callable(S.evalmod_coeffs)
    for word in ("K >= max|I| + 1", "does not sample sparse secrets", "(2 pi m / q_0)^2 / 6", "precision", "should be near",
                 "tests/bootstrap_ref.py", "sealhip_evalmod_plan"):
        assert word in header, word


def _target(K, r, x):
    return np.cos((2.0 * np.pi * K * x - np.pi / 2.0) / 2.0 ** r)


# ------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("K,r,d", [(12, 3, 31), (12, 2, 47), (8, 3, 23), (1, 0, 7)])
def test_coefficients_against_numpy_interpolation(S, K, r, d):
    """on 20001 points of [-1, 1] the library polynomial's largest error against the function is at most
    max(2 x numpy.polynomial.chebyshev.chebinterpolate's, 2^-40): below the floor both are the rounding noise of a degree-d
    series in doubles"""
    ours = np.array(S.evalmod_coeffs(K, r, d))
    assert ours.shape == (d + 1,)
    theirs = NC.chebinterpolate(lambda x: _target(K, r, x), d)
    f = _target(K, r, GRID)
    err_ours = float(np.max(np.abs(NC.chebval(GRID, ours) - f)))
    err_numpy = float(np.max(np.abs(NC.chebval(GRID, theirs) - f)))
    print("K=%d r=%d d=%d: library %.3e numpy %.3e" % (K, r, d, err_ours, err_numpy))
    assert err_ours <= max(2 * err_numpy, 2.0 ** -40)


def _model_error(coeffs, K, r):
    """u = I + m / q_0 with I uniform in (-K, K) and |m / q_0| <= 2^-11: the polynomial at u / K, r doublings, over 2 pi;
    the largest error relative to the largest |m / q_0|"""
    rng = np.random.default_rng(2024)
    v = rng.uniform(-(2.0 ** -11), 2.0 ** -11, size=200000)
    I = rng.integers(-(K - 1), K, size=v.size).astype(np.float64)
    y = NC.chebval((I + v) / K, np.asarray(coeffs))
    for _ in range(r):
        y = 2.0 * y * y - 1.0
    return float(np.max(np.abs(y / (2.0 * np.pi) - v)) / np.max(np.abs(v)))


def test_end_to_end_model_in_float64(S):
    """with the library's coefficients the sine term alone remains, (2 pi 2^-11)^2 / 6 = 1.57e-6 < 2^-18; a polynomial of
    too low a degree does NOT pass, so the test can tell a bad polynomial"""
    for K, r, d in ((12, 3, 31), (12, 2, 47)):
        err = _model_error(S.evalmod_coeffs(K, r, d), K, r)
        print("K=%d r=%d d=%d: relative error %.3e" % (K, r, d, err))
        assert err < 2.0 ** -18
    bad = _model_error(S.evalmod_coeffs(12, 3, 23), 12, 3)
    print("K=12 r=3 d=23: relative error %.3e" % bad)
    assert not bad < 2.0 ** -18


# ------------------------------------------------------------------ plan
@pytest.fixture(scope="module")
def host(S):
    n = 256
    mods = O.get_primes(n, 50, 16) + O.get_primes(n, 60, 2)  # first level 16, two special primes
    return S, mods, S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)


@pytest.mark.parametrize("K,r,d,n_baby", [(12, 3, 31, 8), (12, 2, 47, 0), (4, 1, 7, 0), (1, 0, 7, 0), (12, 8, 7, 0)])
@pytest.mark.parametrize("s_x,scale_out", [(2.0 ** 50, 0.0), (2.0 ** 49.96, 2.0 ** 50.1)])
def test_plan_is_the_restatement_bit_for_bit(host, K, r, d, n_baby, s_x, scale_out):
    S, mods, ctx = host
    k = 16
    got = S.Evaluator(ctx).evalmod_plan(k, s_x, K, r, d, n_baby=n_baby, scale_out=scale_out)
    want = B.evalmod_plan(mods[:16], k, s_x, got["coeffs"], r, n_baby=n_baby, scale_out=scale_out)
    assert (got["poly_level"], got["out_level"]) == (want["poly_level"], want["out_level"])
    assert got["poly_scale_out"] == want["t0"] and got["scales"] == want["scales"], (got["scales"], want["scales"])
    assert got["out_scale"] == want["scales"][-1] and got["n_products"] == want["n_products"]
    assert got["n_baby"] == want["poly"]["m"]
    target = scale_out if scale_out else s_x
    assert abs(got["out_scale"] / target - 1.0) <= 2.0 ** (r + 3) * 2.0 ** -53
    # the polynomial the call evaluates is the existing planner's at scale_out = t_0
    poly = S.Evaluator(ctx).polynomial_plan_ckks(k, s_x, got["coeffs"], basis=1, n_baby=n_baby, scale_out=got["poly_scale_out"])
    assert poly["out_level"] == got["poly_level"] and np.array_equal(poly["weights"], want["poly"]["W"])
    assert np.array_equal(poly["constants"], want["poly"]["K"])
    if (d, n_baby) == (31, 8):
        assert k - got["poly_level"] == 6, "degree 31 with eight baby steps takes six levels"


def test_plan_refusals_on_host_only_context(host):
    S, mods, ctx = host
    ev = S.Evaluator(ctx)
    with pytest.raises(ValueError, match="end of modulus switching chain reached"):
        ev.evalmod_plan(9, 2.0 ** 50, 12, 3, 31, n_baby=8)  # six levels and three steps below level 9: level 0
    ev.evalmod_plan(10, 2.0 ** 50, 12, 3, 31, n_baby=8)
    with pytest.raises(ValueError, match="r must be at most 8"):
        ev.evalmod_plan(16, 2.0 ** 50, 12, 9, 31)
    with pytest.raises(ValueError, match="K must be at least 1"):
        ev.evalmod_plan(16, 2.0 ** 50, 0, 3, 31)
    for bad_k in (0, 17):
        with pytest.raises(ValueError, match="level k out of range"):
            ev.evalmod_plan(bad_k, 2.0 ** 50, 12, 3, 31)
    n = 256
    small = O.get_primes(n, 40, 16) + O.get_primes(n, 60, 2)
    ctx40 = S.Context(S.SCHEME_CKKS, 8, small, 2, 0, device=-1)
    with pytest.raises(ValueError, match="scale out of bounds"):
        S.Evaluator(ctx40).evalmod_plan(16, 2.0 ** 53.6, 12, 3, 31, n_baby=8)
    bfv = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).evalmod_plan(16, 2.0 ** 50, 12, 3, 31)
    with pytest.raises(TypeError):
        S._check(S.lib().sealhip_evaluator_evalmod_plan(ctx.handle, 16, 2.0 ** 50, 12, 3, 31, 0, 0.0, None))
    with pytest.raises(TypeError):
        S._check(S.lib().sealhip_evalmod_coeffs(12, 3, 31, None))


def test_plan_header_under_sanitizers(tmp_path):
    exe = compile_cpp(tmp_path, "evalmod_plan_check.cpp", sanitize=True)
    assert "evalmod_plan_check: OK" in run_exe(exe, timeout=300)


# ------------------------------------------------------------------ the calls' checks on host-only contexts
A, B_, OUT = 0x1000000, 0x2000000, 0x3000000  # made-up device addresses far apart (nothing is dereferenced on the host)


def test_mod_raise_checks_on_host_only_context(host):
    """E_POINTER first; then the scheme, the levels, k_out < 2, the overlap, the alignment (E_INVALIDARG), each ahead of the
    ones after it; then the empty batch (S_OK); then the host-only context (COR_E_INVALIDOPERATION)"""
    S, mods, ctx = host
    L, h = S.lib(), ctx.handle
    bfv = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    call = lambda hh, k_in, ct, count, k_out, out: S._check(L.sealhip_evaluator_mod_raise(hh, k_in, ct, count, k_out, out))
    for args in ((None, 1, A, 1, 2, OUT), (h, 99, None, 1, 2, OUT), (bfv.handle, 1, A, 1, 0, None)):
        with pytest.raises(TypeError):
            call(*args)
    for count in (1, 0):
        with pytest.raises(ValueError, match="CKKS only"):
            call(bfv.handle, 0, A, count, 1, A)
        for k_in, k_out in ((0, 2), (17, 2), (1, 17), (1, 0)):
            with pytest.raises(ValueError, match="level k out of range"):
                call(h, k_in, A, count, k_out, A + 8)
        with pytest.raises(ValueError, match="at least 2"):
            call(h, 1, A, count, 1, A + 8)
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(h, 1, A + 8, count, 2, OUT)
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(h, 1, A, count, 2, OUT + 8)
    with pytest.raises(ValueError, match="overlap"):
        call(h, 3, A, 2, 5, A + 8 * (2 * 2 * 3 * 256 - 2))  # out begins at the last two words of ct
    with pytest.raises(ValueError, match="overlap"):
        call(h, 3, A + 8 * (2 * 2 * 5 * 256 - 2), 2, 5, A)  # ct begins at the last two words of out
    call(h, 3, A, 0, 5, A + 8 * (2 * 2 * 3 * 256 - 2))  # an empty batch overlaps nothing
    with pytest.raises(S.LogicError):
        call(h, 3, A, 2, 5, A + 8 * (2 * 2 * 3 * 256))  # back to back is no overlap: the host-only context speaks, last


def test_mod_raise_host_only_comes_last(host):
    S, mods, ctx = host
    L, h = S.lib(), ctx.handle
    S._check(L.sealhip_evaluator_mod_raise(h, 1, A, 0, 2, OUT))
    with pytest.raises(S.LogicError):
        S._check(L.sealhip_evaluator_mod_raise(h, 1, A, 1, 2, OUT))


def test_double_angle_and_eval_mod_checks_on_host_only_context(host):
    S, mods, ctx = host
    L, h = S.lib(), ctx.handle
    bfv = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    scale = C.c_double(0.0)
    nokeys = (C.c_void_p * 1)(None)
    da = lambda hh, k, ct, count, s, keys, nk, out, osc: S._check(
        L.sealhip_evaluator_double_angle(hh, k, ct, count, s, keys, nk, out, osc))
    for args in ((None, 2, A, 1, 2.0 ** 40, nokeys, 0, OUT, C.byref(scale)), (h, 99, None, 1, 2.0 ** 40, nokeys, 0, OUT, C.byref(scale)),
                 (h, 99, A, 1, 2.0 ** 40, nokeys, 0, None, C.byref(scale)), (h, 99, A, 1, 2.0 ** 40, nokeys, 0, OUT, None),
                 (h, 99, A, 1, 2.0 ** 40, None, 0, OUT, C.byref(scale)), (h, 99, A, 1, 2.0 ** 40, nokeys, 1, OUT, C.byref(scale))):
        with pytest.raises(TypeError):
            da(*args)
    for count in (1, 0):
        with pytest.raises(ValueError, match="CKKS only"):
            da(bfv.handle, 0, A, count, -1.0, nokeys, 0, A, C.byref(scale))
        for k in (0, 17):
            with pytest.raises(ValueError, match="level k out of range"):
                da(h, k, A, count, -1.0, nokeys, 0, A, C.byref(scale))
        with pytest.raises(ValueError, match="end of modulus switching chain reached"):
            da(h, 1, A, count, -1.0, nokeys, 0, A, C.byref(scale))
        for bad in (-1.0, 0.0, float("nan"), float("inf"), 1e160):
            with pytest.raises(ValueError, match="scale out of bounds"):
                da(h, 4, A, count, bad, nokeys, 0, A, C.byref(scale))
        with pytest.raises(ValueError, match="not enough relinearization keys"):
            da(h, 4, A, count, 2.0 ** 40, nokeys, 0, A, C.byref(scale))
    assert scale.value == 0.0, "a refused call writes nothing"
    # eval_mod: the plan's refusals come first, then the keys
    em = lambda hh, k, count, s, K, r, d, nb, keys, nk, out: S._check(
        L.sealhip_evaluator_eval_mod(hh, k, A, count, s, K, r, d, nb, 0.0, keys, nk, out, None, None))
    with pytest.raises(TypeError):
        em(h, 99, 1, 2.0 ** 50, 12, 3, 31, 8, nokeys, 0, None)
    for count in (1, 0):
        with pytest.raises(ValueError, match="CKKS only"):
            em(bfv.handle, 16, count, 2.0 ** 50, 12, 3, 31, 8, nokeys, 0, A)
        with pytest.raises(ValueError, match="level k out of range"):
            em(h, 17, count, 2.0 ** 50, 12, 9, 31, 8, nokeys, 0, A)
        with pytest.raises(ValueError, match="r must be at most 8"):
            em(h, 16, count, 2.0 ** 50, 12, 9, 31, 8, nokeys, 0, A)
        with pytest.raises(ValueError, match="end of modulus switching chain reached"):
            em(h, 9, count, 2.0 ** 50, 12, 3, 31, 8, nokeys, 0, A)
        with pytest.raises(ValueError, match="not enough relinearization keys"):
            em(h, 16, count, 2.0 ** 50, 12, 3, 31, 8, nokeys, 0, A)


def test_cpp_adapter_on_host_only_context(tmp_path):
    """tests/host_adapter_bootstrap_check.cpp "host": the plans' refusals and the operand checks arrive before the missing
    device does"""
    exe = compile_cpp(tmp_path, "host_adapter_bootstrap_check.cpp", link_sealhip=True)
    assert "host-only bootstrap checks ok" in run_exe(exe, "host", timeout=120)


def test_bootstrap_plan_on_host_only_context(host):
    """levels, S = q_0 K, the gain q_0 / (2 pi s_r) and the union of both transforms' steps, bit for bit; the refusals"""
    S, mods, ctx = host
    ev = S.Evaluator(ctx)
    plan = ev.bootstrap_plan(16, [4, 3], [4, 3], 1, 3, 31, n_baby=8)
    em = ev.evalmod_plan(14, float(mods[0]) * 1, 1, 3, 31, n_baby=8)
    assert (plan["k_top"], plan["c2s_out_level"], plan["evalmod_out_level"], plan["out_level"]) == (16, 14, 5, 3)
    assert plan["raise_scale"] == float(mods[0]) * 1 and plan["evalmod"]["scales"] == em["scales"]
    assert plan["s2c_gain"] == float(mods[0]) / (6.283185307179586476925286766559 * em["out_scale"])
    p1, p2 = ev.dft_plan(S.DFT_COEFFS_TO_SLOTS, 16, [4, 3]), ev.dft_plan(S.DFT_SLOTS_TO_COEFFS, 5, [4, 3])
    assert plan["key_steps"] == sorted(set(p1["key_steps"]) | set(p2["key_steps"])) and plan["needs_conjugation"] == 1
    assert plan["table_words"] == p1["table_words"] + p2["table_words"]
    assert plan["temp_bytes_per_item"] == 2 * 256 * 8 * (16 + 2 * 14 + 2 * 5)
    with pytest.raises(ValueError, match="end of modulus switching chain reached"):
        ev.bootstrap_plan(12, [4, 3], [4, 3], 1, 3, 31, n_baby=8)  # EvalMod would end at level 1: no room for SlotToCoeff
    with pytest.raises(ValueError, match="sum to"):
        ev.bootstrap_plan(16, [4, 2], [4, 3], 1, 3, 31, n_baby=8)
    with pytest.raises(ValueError, match="K must be at least 1"):
        ev.bootstrap_plan(16, [4, 3], [4, 3], 0, 3, 31, n_baby=8)
    with pytest.raises(S.LogicError):
        S.BootstrapTables(ctx, 16, [4, 3], [4, 3], 1, 3, 31, n_baby=8)
    with pytest.raises(ValueError, match="scale out of bounds"):
        ev.bootstrap_plan(16, [4, 3], [4, 3], 12, 3, 31, n_baby=8)  # S = 12 q_0 over primes of q_0's size
