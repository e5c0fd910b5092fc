"""BFV multiply and square through the exact-k BEHZ kernels (bfv_lift_exact_kernel / bfv_floor_sk_exact_kernel, rns.hip) at both
split positions of their carry-free dot products (dotacc.hpp DotAccSplit<S, ...>), word for word against the CPU oracle.

Ring N = 2^14, the smallest with the fused kernels; 3 items per call; PARITY and STRICT; levels k = 1, 7, 8, 15 and two
plain moduli, so that |B| = k and |B| = k + 1 are both met. Two sets of ciphertext primes:
  w58  58-bit primes: the level predicate (ntt_bounds.hpp section 5, behz_split_admits) admits S = 30 at every level; the
       tables are packed at 30 and the S = 30 instances run.
  w60  60-bit primes, distinct from the context's 60-bit auxiliary primes: at k = 7 and 8 the floor rows' cross products
       (2 k + 1 of 2^60 and one of 2^61) no longer fit one accumulator, the predicate refuses, and the S = 31 instances --
       the ones every level ran before -- still serve the level. At k = 1 three products fit and S = 30 is admitted even
       at this width. At k = 15 the level leaves the exact-k class altogether (k q + 2 m_sk passes 2^64: section 7) and
       the run-time-k instance, which has no split, takes it; S is recorded as 31.
Operands per call: every word q_i - 1, q_i - 1 alternating with 0, all zero, and seeded random, spread over the three
items of both operands. The selected split is read back through sealhip_debug_behz_dot_split. No tolerance is involved."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from support import S as sealhip

pytestmark = pytest.mark.gpu

LOGN, N = 14, 1 << 14
LEVELS = (1, 7, 8, 15)
NKEY = max(LEVELS) + 1  # one special prime
TOP, ALT, ZERO, RANDOM = 0, 1, 2, 3
# (a, b) per item: multiply sees every pattern in both operands over the two triples; square reads a only
ITEMS = (((TOP, TOP), (ALT, RANDOM), (RANDOM, ZERO)), ((TOP, ALT), (ZERO, TOP), (RANDOM, RANDOM)))
SQUARE_ITEMS = ((TOP, TOP), (ALT, ALT), (RANDOM, RANDOM)), ((ZERO, ZERO), (ALT, ALT), (TOP, TOP))
# prime set -> level -> (split, exact-k instance?)
EXPECT = {"w58": {k: (30, True) for k in LEVELS},
          "w60": {1: (30, True), 7: (31, True), 8: (31, True), 15: (31, False)}}


@pytest.fixture(scope="module")
def modsets():
    aux = set(int(p) for p in O.aux_primes(N, NKEY + 3))
    wide = [p for p in O.ntt_primes_below(N, 1 << 60, 2 * NKEY + 3) if int(p) not in aux][:NKEY]
    assert len(wide) == NKEY and all(int(p).bit_length() == 60 for p in wide)
    return {"w58": O.ntt_primes_below(N, 1 << 58, NKEY), "w60": wide}


@pytest.fixture(scope="module")
def contexts(sealhip, modsets):
    """(prime set, t index, mode) -> (engine context, oracle context), built on first use and kept for the module's cases"""
    made = {}

    def get(ps, ti, mode):
        if (ps, ti, mode) not in made:
            t, mods = O.BFV_PLAN_T[ti], modsets[ps]
            made[ps, ti, mode] = (sealhip.Context(sealhip.SCHEME_BFV, LOGN, mods, 1, t, mode=mode),
                                  O.RefContext(1, LOGN, mods, nsp=1, t=t, mode=mode))
        return made[ps, ti, mode]

    return get


def _operand(rng, q, pattern):
    if pattern == RANDOM:
        return np.stack([np.stack([rng.integers(0, p, size=N, dtype=np.uint64) for p in q]) for _ in range(2)])
    out = np.stack([np.full((2, N), p - 1, dtype=np.uint64) for p in q], axis=1)
    if pattern == ALT:
        out[:, :, 1::2] = 0
    elif pattern == ZERO:
        out[:] = 0
    return out


@pytest.mark.parametrize("ps", ["w58", "w60"])
def test_levels_select_the_split(sealhip, modsets, contexts, ps):
    """the split each level's tables are packed with, the instance the plan names, and |B| = k and k + 1 both met"""
    extra = set()
    for ti in (0, 1):
        ctx, _ = contexts(ps, ti, 0)
        for k in LEVELS:
            split, exact = EXPECT[ps][k]
            assert ctx.debug_behz_dot_split(k) == split, (ps, ti, k)
            for sq in (False, True):
                plan = ctx.debug_bfv_multiply_plan(k, 2, 2, sq)
                code = k if exact else O.BEHZ_GENERIC
                assert plan["lift_kernel"] == code and plan["floor_kernel"] == code, (ps, ti, k, plan)
                if exact:
                    extra.add((k, plan["B"] - k))
    assert extra >= {(k, e) for k in (1, 7, 8) for e in (0, 1)}, sorted(extra)


@pytest.mark.parametrize("k", LEVELS)
@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
@pytest.mark.parametrize("ti", [0, 1], ids=["t20", "t59"])
@pytest.mark.parametrize("ps", ["w58", "w60"])
def test_multiply_and_square_at_both_splits(sealhip, modsets, contexts, ps, ti, mode, k):
    ctx, ref = contexts(ps, ti, mode)
    assert ctx.debug_behz_dot_split(k) == EXPECT[ps][k][0]
    ev = sealhip.Evaluator(ctx)
    L = O.lib()
    q = [int(p) for p in modsets[ps][:k]]
    rng = np.random.default_rng(5000 * (ps == "w60") + 1000 * ti + 100 * mode + k)
    items = ITEMS[(k + ti) % 2]
    sq_items = SQUARE_ITEMS[(k + ti) % 2]
    a = np.stack([_operand(rng, q, pa) for pa, _ in items])
    b = np.stack([_operand(rng, q, pb) for _, pb in items])
    s = np.stack([_operand(rng, q, pa) for pa, _ in sq_items])
    count = len(items)
    out = ctx.alloc(count * 3 * k * N)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, out)
    got_mul = out.download((count, 3, k, N))
    out2 = ctx.alloc(count * 3 * k * N)
    ev.square(ctx.upload(s), 2, k, count, out2)
    got_sq = out2.download((count, 3, k, N))
    ref.rns_tool(k)  # built once, here: the oracle calls below run on several threads and only read the context

    def oracle(i, square):
        exp = np.zeros((3, k, N), dtype=np.uint64)
        if square:
            assert L.ref_bfv_square(C.byref(ref.c), k, O.ptr(s[i]), 2, O.ptr(exp)) == 0
        else:
            assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(exp)) == 0
        return exp

    with ThreadPoolExecutor(6) as pool:
        futs = [(pool.submit(oracle, i, square), i, square) for square in (False, True) for i in range(count)]
        for fut, i, square in futs:
            got = got_sq[i] if square else got_mul[i]
            assert np.array_equal(got, fut.result()), ("square" if square else "multiply", i, (sq_items if square else items)[i])
