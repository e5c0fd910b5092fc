"""The kernels of csrc/rns.hip at planted rounding boundaries: every output word against the Python integers of
tests/rns_ref.py and, where the oracle has the function, the oracle held to the integers first (tests/test_rns_host.py does
the same on the CPU, so a failure here names the side that disagreed).

Every kernel here branches on a comparison at a half-way point -- r_m_tilde >= 2^31, alpha_sk > m_sk / 2, last + half past
q_last, Q.p < L.p, v_gamma > gamma / 2, r == 0 -- which random words meet with probability 2^-32 or less. The operands are
solved (rns_ref's planters) so that the deciding intermediate sits at 0, 1, on either side of the comparison and at the top
of its range, in both lanes and at the corner columns of a row. Chains: 61-bit primes (P61), the ring's smallest NTT primes
(PMIN) and 61 / 20 / 45 / 61 bits (PMIX). Nothing rests on a tolerance: word for word."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import linear_layer_ref as R
import oracle_lib as O
import rns_ref as M
import test_rns_host as H
from support import S, session_memo

pytestmark = pytest.mark.gpu

L = O.lib()
T_IDS = {H.T_SMALL: "t_small", H.T_59: "t_59", 2: "t=2", (1 << 60) - 93: "t=2^60-93"}


class Session:
    """a context and the oracle's over one chain"""

    def __init__(self, S, scheme, logn, mods, t, strict=False):
        self.logn, self.n, self.mods, self.t = logn, 1 << logn, [int(p) for p in mods], t
        self.ctx = S.Context(scheme, logn, self.mods, 1, t, mode=S.MODE_STRICT if strict else S.MODE_PARITY)
        self.ev = S.Evaluator(self.ctx)
        self.ref = O.RefContext(scheme, logn, self.mods, nsp=1, t=t, mode=1 if strict else 0)


session = session_memo(Session)


def same(got, exp, what, oracle=None):
    """got == exp word for word; the oracle, where there is one, is held to the integers first"""
    if oracle is not None:
        assert np.array_equal(oracle, exp), "%s: the ORACLE disagrees with the integers" % (what,)
    if not np.array_equal(got, exp):
        at = tuple(int(v[0]) for v in np.nonzero(got != exp))
        raise AssertionError("%s: the KERNEL disagrees with the integers at %s: got %d, expected %d (%d words differ)"
                             % (what, at, int(got[at]), int(exp[at]), int((got != exp).sum())))


def filled(ctx, shape):
    """a device buffer of `shape` words, none of which is a value a kernel would leave (every word must be written)"""
    return ctx.upload(np.full(shape, (1 << 64) - 7, dtype=np.uint64))


# ---------------------------------------------------------------- a. the four base-conversion entries
BCONV_ENTRIES = ("fastbconv_m_tilde", "sm_mrq", "fast_floor", "fastbconv_sk")
BCONV_CASES = [(3, k) for k in H.BCONV_LEVELS] + [(9, k) for k in H.SMALL_LEVELS]
_bconv_operands = {}


def bconv_operands(name, logn, k, t):
    key = (name, logn, k, t)
    if key not in _bconv_operands:
        _bconv_operands.clear()  # (the four entries of one case run back to back)
        _bconv_operands[key] = H.bconv_operands(H.rns(name, logn, k, t, H.key_count(logn)), 1 << logn, 1000 * logn + k)
    return _bconv_operands[key]


@pytest.mark.parametrize("entry", BCONV_ENTRIES)
@pytest.mark.parametrize("t", [H.T_SMALL, H.T_59], ids=T_IDS.get)
@pytest.mark.parametrize("name", H.CHAINS)
@pytest.mark.parametrize("logn,k", BCONV_CASES, ids=["N=%d-k=%d" % (1 << lg, k) for lg, k in BCONV_CASES])
def test_base_conversions_at_every_bucket_edge(S, logn, k, name, t, entry):
    """fastbconv_m_tilde, sm_mrq, fast_floor and fastbconv_sk at either side of every row-count bucket (4, 8, 16, 32, 64)
    and at k = 1 and 63, with |B| = k and |B| = k + 1; r_m_tilde and alpha_sk planted, boundary words elsewhere; N = 8
    (a block spans items, the last block is partial) and, up to k = 9, N = 2^9"""
    n = 1 << logn
    s = session(S, S.SCHEME_BFV, logn, H.chain64(name, logn, H.key_count(logn)), t)
    ref = H.rns(name, logn, k, t, H.key_count(logn))
    assert s.ctx.bsk_size(k) == ref.Bsk_size == ref.B_size + 1
    assert [int(p) for p in s.ctx.debug_rns_constants(k, 0)] == ref.Bsk
    if name == "P61":
        assert ref.B_size == (k + 1 if t == H.T_59 else k)
    x, _ = bconv_operands(name, logn, k, t)[entry]
    exp = getattr(ref, entry)(x)
    count = x.shape[0]
    if n == 8:
        assert (count * n) % 256, "the last block is partial"
    out = filled(s.ctx, exp.shape)
    getattr(s.ctx, entry)(k, s.ctx.upload(x), count, out)
    same(out.download(exp.shape), exp, "%s %s N=%d k=%d |B|=%d" % (entry, name, n, k, ref.B_size),
         H.oracle_bconv(s.ref, ref, entry, x))
    before = out.download(exp.shape)
    getattr(s.ctx, entry)(k, s.ctx.upload(x), 0, out)  # an empty batch is a no-op
    assert np.array_equal(out.download(exp.shape), before)


# ---------------------------------------------------------------- b. level-down
def down_case(S, scheme, logn, name, k, strict=False):
    s = session(S, scheme, logn, R.chain(name, logn), 2 if scheme == S.SCHEME_BFV else 0, strict)
    ref = H.rns_down(name, logn, k)
    return s, ref, H.down_operand(ref, 1 << logn, 10 * logn + k)


def ciphertexts(x, size):
    """ct[count][size][k][n] from x[count][k][n]: polynomial j of item i is x[i + j]"""
    return np.ascontiguousarray(np.stack([np.roll(x, -j, axis=0) for j in range(size)], axis=1))


DOWN_RINGS = [3, 8, 9]


@pytest.mark.parametrize("k", H.DOWN_LEVELS)
@pytest.mark.parametrize("name", H.CHAINS)
@pytest.mark.parametrize("logn", DOWN_RINGS)
def test_divide_and_round_q_last_on_planted_last_words(S, logn, name, k):
    """the last row at 0, 1, either side of half and of p - half, p - 2 and p - 1 against every boundary word of the rows above"""
    s, ref, x = down_case(S, S.SCHEME_BFV, logn, name, k)
    exp, last = ref.divide_and_round_q_last(x, deciding=True)
    d = s.ctx.upload(x)
    s.ctx.divide_and_round_q_last_inplace(k, d, len(x))
    got = d.download(x.shape)
    what = "divide_and_round_q_last %s N=%d k=%d" % (name, s.n, k)
    same(np.ascontiguousarray(got[:, :k - 1]), exp, what, H.oracle_down(s.ref, k, x, False))
    assert np.array_equal(got[:, k - 1], M._u64(last)), what + ": the rounded last row"


def run_down_ntt(S, logn, name, k, strict, call):
    """the NTT form in a PARITY or STRICT context: call(session, device buffer, items) -> [items][k - 1][n]. STRICT is held to
    the integers always; PARITY where the reference's uncorrected forward transform cannot pass 2^64 (H.lazy_forward_exact)
    and to the oracle, whose words are PARITY's contract, in every case"""
    s, ref, x = down_case(S, S.SCHEME_BFV if call is inplace_ntt else S.SCHEME_CKKS, logn, name, k, strict)
    xn = H.oracle_ntt_rows(s.ref, x)
    what = "%s %s N=%d k=%d %s" % (call.__name__, name, s.n, k, "STRICT" if strict else "PARITY")
    ora = H.oracle_down(s.ref, k, xn, True, strict=int(strict))
    got = call(s, xn, k)
    if strict or H.lazy_forward_exact(ref.q, logn):
        same(got, ref.divide_and_round_q_last_ntt(xn, H.math_ntts(ref, logn)), what, ora)
    assert np.array_equal(got, ora), what + ": the kernel disagrees with the oracle"


def inplace_ntt(s, xn, k):
    d = s.ctx.upload(xn)
    s.ctx.divide_and_round_q_last_ntt_inplace(k, d, len(xn))
    return np.ascontiguousarray(d.download(xn.shape)[:, :k - 1])


def rescale(s, xn, k):
    ct = ciphertexts(xn, 2)
    out = filled(s.ctx, (len(ct), 2, k - 1, s.n))
    s.ev.rescale_to_next(s.ctx.upload(ct), 2, k, len(ct), out)
    got = out.download((len(ct), 2, k - 1, s.n))
    assert np.array_equal(got[:, 1], np.roll(got[:, 0], -1, axis=0)), "the second polynomial is the next item's first"
    return np.ascontiguousarray(got[:, 0])


@pytest.mark.parametrize("strict", [False, True], ids=["parity", "strict"])
@pytest.mark.parametrize("call", [inplace_ntt, rescale], ids=["inplace", "rescale_to_next"])
@pytest.mark.parametrize("k", H.DOWN_LEVELS)
@pytest.mark.parametrize("name", H.CHAINS)
@pytest.mark.parametrize("logn", DOWN_RINGS)
def test_divide_and_round_q_last_ntt_on_planted_last_words(S, logn, name, k, call, strict):
    """divide_and_round_q_last_ntt_inplace and Evaluator.rescale_to_next (CKKS) on the transform of the planted rows"""
    run_down_ntt(S, logn, name, k, strict, call)


@pytest.mark.parametrize("size,strided", [(2, False), (3, False), (2, True)], ids=["size2", "size3", "size2-strided"])
@pytest.mark.parametrize("k", H.DOWN_LEVELS)
@pytest.mark.parametrize("name", H.CHAINS)
@pytest.mark.parametrize("logn", DOWN_RINGS)
def test_mod_switch_to_next_on_planted_last_words(S, logn, name, k, size, strided):
    """Evaluator.mod_switch_to_next (BFV) at sizes 2 and 3, and at size 2 inside size-3 items (a non-contiguous stride)"""
    s, ref, x = down_case(S, S.SCHEME_BFV, logn, name, k)
    held = 3 if strided else size
    ct = ciphertexts(x, held)
    count = len(ct)
    exp = np.stack([np.roll(ref.divide_and_round_q_last(x), -j, axis=0) for j in range(size)], axis=1)
    ora = np.zeros_like(exp)
    for i in range(count):
        assert L.ref_mod_switch_scale_to_next(C.byref(s.ref.c), k, O.ptr(np.ascontiguousarray(ct[i, :size])), size, O.ptr(ora[i])) == 0
    out = filled(s.ctx, exp.shape)
    s.ev.mod_switch_to_next(s.ctx.upload(ct), size, k, count, out, item_stride=held * k * s.n if strided else 0)
    same(out.download(exp.shape), exp, "mod_switch_to_next %s N=%d k=%d size %d of %d" % (name, s.n, k, size, held), ora)


def test_level_down_at_many_blocks_per_row(S):
    """N = 2^13 on PMIX at k = 4: the coefficient form against the integers, the NTT form against the oracle"""
    logn, name, k = 13, "PMIX", 4
    s, ref, x = down_case(S, S.SCHEME_BFV, logn, name, k)
    x = x[:2]
    d = s.ctx.upload(x)
    s.ctx.divide_and_round_q_last_inplace(k, d, len(x))
    same(np.ascontiguousarray(d.download(x.shape)[:, :k - 1]), ref.divide_and_round_q_last(x),
         "divide_and_round_q_last PMIX N=8192", H.oracle_down(s.ref, k, x, False))
    xn = H.oracle_ntt_rows(s.ref, x)
    assert np.array_equal(inplace_ntt(s, xn, k), H.oracle_down(s.ref, k, xn, True))


# ---------------------------------------------------------------- c. decrypt_scale_and_round
@pytest.mark.parametrize("k", H.DSR_LEVELS)
@pytest.mark.parametrize("t", H.DSR_T, ids=T_IDS.get)
@pytest.mark.parametrize("name", H.CHAINS)
@pytest.mark.parametrize("logn", [3, 9])
def test_decrypt_scale_and_round_on_planted_v_gamma(S, logn, name, t, k):
    """v_gamma at 0, 1, either side of gamma / 2 and gamma - 1 where a prime of the level exceeds gamma (P61, PMIX), the two
    kinds of r = 0 column, and boundary words in every row on all three chains"""
    s = session(S, S.SCHEME_BFV, logn, H.chain64(name, logn), t)
    ref = H.rns(name, logn, k, t)
    x, idx, _ = H.dsr_operand(ref, s.n, 100 * logn + k, name)
    assert (idx is None) == ((name, "vg") in H.NOT_PLANTABLE)
    exp = ref.decrypt_scale_and_round(x)
    out = filled(s.ctx, exp.shape)
    s.ctx.decrypt_scale_and_round(k, s.ctx.upload(x), len(x), out)
    same(out.download(exp.shape), exp, "decrypt_scale_and_round %s N=%d k=%d t=%d" % (name, s.n, k, t),
         H.oracle_dsr(s.ref, k, x))


# ---------------------------------------------------------------- d. the fused lift through multiply and square
@pytest.mark.parametrize("square", [False, True], ids=["multiply", "square"])
@pytest.mark.parametrize("case", H.LIFT_CASES, ids=H.LIFT_IDS)
def test_multiply_on_planted_r_m_tilde(S, case, square):
    """operands whose columns carry every r_m_tilde target, in both operands and both members of the pairs (c, c + N/2) that
    the top-layer instances own, through each instance of the lift: exact k with the dot products split at 30 and at 31,
    with and without the forward transform's top layer, the run-time-k instance and the step-by-step kernels. Expected
    values from the oracle, whose lift steps tests/test_rns_host.py holds to the integers"""
    logn, name, t, k, inst, split, top = case
    n, count = 1 << logn, 3
    mods = H.lift_case_mods(logn, name, t)
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t)
    ref = O.RefContext(1, logn, mods, nsp=1, t=t)
    plan = ctx.debug_bfv_multiply_plan(k, 2, 2, square)
    assert (plan["lift_kernel"], plan["lift_top"]) == (inst, top), plan
    if inst <= O.BEHZ_EXACT_MAX_K:
        assert ctx.debug_behz_dot_split(k) == split
    rns = H.lift_ref(logn, name, t, k)
    a, b = H.lift_operand(rns, n, 2, count, 1), H.lift_operand(rns, n, 2, count, 2)
    out = filled(ctx, (count, 3, k, n))
    ev = S.Evaluator(ctx)
    if square:
        ev.square(ctx.upload(a), 2, k, count, out)
    else:
        ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, out)
    got = out.download((count, 3, k, n))
    ref.rns_tool(k)  # built once: the oracle calls below only read the context

    def oracle(i):
        exp = np.zeros((3, k, n), dtype=np.uint64)
        if square:
            assert L.ref_bfv_square(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(exp)) == 0
        else:
            assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(exp)) == 0
        return exp

    with ThreadPoolExecutor(count) as pool:
        exp = np.stack(list(pool.map(oracle, range(count))))
    if not np.array_equal(got, exp):
        at = tuple(int(v[0]) for v in np.nonzero(got != exp))
        raise AssertionError("%s %s: the product disagrees with the oracle at (item, polynomial, row, column) %s (%d words)"
                             % ("square" if square else "multiply", H.LIFT_IDS[H.LIFT_CASES.index(case)], at,
                                int((got != exp).sum())))
