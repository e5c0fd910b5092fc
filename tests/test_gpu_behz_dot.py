"""BFV multiply and square through the exact-k BEHZ kernels (bfv_lift_exact_kernel / bfv_floor_sk_exact_kernel, rns.hip) with the
operands highest in the dot products' accumulators (dotacc.hpp DotAcc31), word for word against the CPU oracle.

Ring N = 2^14, the smallest with the fused kernels; 58-bit ciphertext primes, the widest the fused tensor product admits;
3 items per call. Levels k = 1, 2, 7, 8, 15 take the exact-k instances, k = 16 the run-time-k instance, which keeps the
128-bit multiply-accumulate. Two plain moduli: with t = 786433 the auxiliary base has |B| = k primes, with the 59-bit t
it has k + 1 at k = 1, 2, 7, 8 (rns.cpp:568-573; at k = 15 the extra prime would leave the exact-k class: ntt_bounds.hpp
section 7). PARITY and STRICT. Operands per call: every word q_i - 1, all zero, q_i - 1 alternating with 0, and seeded
random, spread over the three items of both operands. No tolerance is involved."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from support import S as sealhip

pytestmark = pytest.mark.gpu

LOGN, N = 14, 1 << 14
LEVELS = (1, 2, 7, 8, 15, 16)
TOP, ALT, ZERO, RANDOM = 0, 1, 2, 3
# (a, b) per item: multiply sees every pattern in both operands over the two triples; square reads a only
ITEMS = (((TOP, TOP), (ALT, RANDOM), (RANDOM, ZERO)), ((TOP, ALT), (ZERO, TOP), (RANDOM, RANDOM)))
SQUARE_ITEMS = ((TOP, TOP), (ALT, ALT), (RANDOM, RANDOM)), ((ZERO, ZERO), (ALT, ALT), (TOP, TOP))


@pytest.fixture(scope="module")
def mods():
    return O.ntt_primes_below(N, 1 << 58, max(LEVELS) + 1)


@pytest.fixture(scope="module")
def contexts(sealhip, mods):
    """(t index, mode) -> (engine context, oracle context), built on first use and kept for the module's cases"""
    made = {}

    def get(ti, mode):
        if (ti, mode) not in made:
            t = O.BFV_PLAN_T[ti]
            made[ti, mode] = (sealhip.Context(sealhip.SCHEME_BFV, LOGN, mods, 1, t, mode=mode),
                              O.RefContext(1, LOGN, mods, nsp=1, t=t, mode=mode))
        return made[ti, mode]

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


def test_levels_reach_the_instances(sealhip, mods, contexts):
    """the plans the engine reports: exact-k instances at k <= 15 (|B| = k and k + 1 both met at k = 1, 2, 7, 8), the
    run-time-k instance at 16, the paired-column lift and the deferred top layer on the (2, 2) path"""
    extra = set()
    for ti in (0, 1):
        ctx, _ = contexts(ti, 0)
        for k in LEVELS:
            for sq in (False, True):
                plan = ctx.debug_bfv_multiply_plan(k, 2, 2, sq)
                want = O.bfv_multiply_plan(LOGN, mods, O.BFV_PLAN_T[ti], k, 2, 2, square=sq)
                assert plan == want, (ti, k, sq, plan, want)
                code = k if k <= O.BEHZ_EXACT_MAX_K else O.BEHZ_GENERIC
                assert plan["lift_kernel"] == code and plan["floor_kernel"] == code, (ti, k, plan)
                assert plan["deferred_top"] == 2 and plan["lift_top"] == (1 if k <= O.BEHZ_EXACT_MAX_K else 0), (ti, k, plan)
                extra.add((k, plan["B"] - k))
    assert extra >= {(k, e) for k in (1, 2, 7, 8) for e in (0, 1)} | {(15, 0)}, sorted(extra)


@pytest.mark.parametrize("k", LEVELS)
@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
@pytest.mark.parametrize("ti", [0, 1], ids=["t20", "t59"])
def test_multiply_and_square_at_the_top_of_the_accumulators(sealhip, mods, contexts, ti, mode, k):
    ctx, ref = contexts(ti, mode)
    ev = sealhip.Evaluator(ctx)
    L = O.lib()
    q = [int(p) for p in mods[:k]]
    rng = np.random.default_rng(1000 * ti + 100 * mode + k)
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
