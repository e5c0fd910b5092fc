"""The oracle's RNS tool held to the integers of tests/rns_ref.py, and what the planted operands cover (no GPU).

Three things: (1) every constant of the oracle's RnsTool equals the one rns_ref derives from the primes alone; (2) every
ref_* function that tests/test_gpu_rns.py takes expected values from equals the integers word for word on the planted
batches, at N = 8 and 2^8; (3) the plants do what they claim -- the deciding intermediate (r_m_tilde, alpha_sk, the rounded
last word, v_gamma, r) takes every target, in both lanes, both sides of every branch are taken, and the chains on which a
plant is impossible are exactly those the prime sizes predict. The builders below are the ones the GPU tests use."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import linear_layer_ref as R
import oracle_lib as O
import rns_ref as M
from support import rows

HERE = os.path.dirname(os.path.abspath(__file__))
L = O.lib()
CHAINS = R.CHAINS
N_KEY = 64  # key primes of the base-conversion contexts: levels up to 63
BCONV_LEVELS = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 63)  # either side of every bucket of dispatch_k_bucket, and both ends
SMALL_LEVELS = tuple(k for k in BCONV_LEVELS if k <= 9)  # the levels repeated on the larger rings
T_SMALL, T_59 = O.BFV_PLAN_T  # |B| = k and, on 61-bit primes, |B| = k + 1
DOWN_LEVELS = (2, 3, 4)
DSR_LEVELS = (1, 4, 63)
DSR_T = (2, 786433, T_59, (1 << 60) - 93)
# A plant needs one row whose prime exceeds the modulus its solved word lives under: 2^32 for r_m_tilde on a q-basis column,
# gamma (60 bits) for v_gamma. The smallest NTT primes of these rings have at most 19 bits: boundary words only there.
NOT_PLANTABLE = {("PMIN", "r_m_tilde"), ("PMIN", "vg")}


# ---------------------------------------------------------------- chains and references
@functools.lru_cache(maxsize=None)
def chain64(name, logn, count=N_KEY):
    """R.chain's three classes extended to `count` key primes (the last one special): 61-bit primes, the ring's smallest
    NTT primes, and 61 / 20 / 45 / 61 bits repeating; coprime to the auxiliary primes and to every plain modulus used"""
    n = 1 << logn
    if name == "P61":
        mods = O.ntt_primes_below(n, 1 << 61, count)
    elif name == "PMIN":
        mods = R.ntt_primes_from(n, count)
    else:
        assert name == "PMIX", name
        big, small, mid = (O.ntt_primes_below(n, 1 << b, c) for b, c in ((61, (count + 1) // 2), (20, count // 4 + 1),
                                                                         (45, count // 4 + 1)))
        mods = [(big[2 * (i // 4) + (i % 4 == 3)] if i % 4 in (0, 3) else small[i // 4] if i % 4 == 1 else mid[i // 4])
                for i in range(count)]
        assert [p.bit_length() for p in mods[:4]] == [61, 20, 45, 61][:len(mods[:4])]
    assert len(set(mods)) == count and not set(mods) & set(aux(n, count)) and not set(mods) & set(DSR_T)
    return tuple(mods)


def aux(n, n_key):
    return O.aux_primes(n, n_key + 3)


@functools.lru_cache(maxsize=None)
def rns(name, logn, k, t, count=N_KEY):
    return M.RnsRef(chain64(name, logn, count)[:k], t, aux(1 << logn, count))


@functools.lru_cache(maxsize=None)
def rns_down(name, logn, k):
    """level k of linear_layer_ref's five-prime chains (on PMIX the last prime has 20, 45 and 61 bits at k = 2, 3, 4)"""
    mods = R.chain(name, logn)
    return M.RnsRef(mods[:k], 2, aux(1 << logn, len(mods)))


@functools.lru_cache(maxsize=None)
def oracle_context(mods, logn, t):
    return O.RefContext(1, logn, list(mods), nsp=1, t=t)


def key_count(logn):
    return N_KEY if logn == 3 else max(SMALL_LEVELS) + 1


def levels(logn):
    return BCONV_LEVELS if logn == 3 else SMALL_LEVELS


# ---------------------------------------------------------------- operands (shared with the GPU tests)
def plant_items(n):
    return None if n == 8 else 3  # N = 8: as many items as put every target at every corner; the last block is partial


def bconv_operands(ref, n, seed):
    """{entry: (operand, spread index of the plant or None)}: boundary words in every row for fastbconv_m_tilde and
    fast_floor, r_m_tilde planted through the m_tilde word for sm_mrq, alpha_sk planted for fastbconv_sk"""
    rng = np.random.default_rng(seed)
    lead = (max(3, R.lead_for(n, 7, n == 8)),)
    out = {"fastbconv_m_tilde": (R.boundary_rows(ref.q, n, lead, R.boundary_words, rng), None),
           "fast_floor": (R.boundary_rows(ref.q + ref.Bsk, n, lead, R.boundary_words, rng), None)}
    idx, items = M.spread(n, len(M.R_M_TILDE_TARGETS), plant_items(n))
    x = R.boundary_rows(ref.Bsk + [M.MT], n, (items,), R.boundary_words, rng)
    out["sm_mrq"] = (ref.plant_r_m_tilde(x, None, *M.targets_at(idx, M.R_M_TILDE_TARGETS)), idx)
    idx, items = M.spread(n, len(ref.alpha_sk_targets()), plant_items(n))
    x = rows(rng, ref.Bsk, n, (items,))
    out["fastbconv_sk"] = (ref.plant_alpha_sk(x, *M.targets_at(idx, ref.alpha_sk_targets())), idx)
    return out


def down_operand(ref, n, seed):
    return ref.plant_last(n, np.random.default_rng(seed))


def dsr_operand(ref, n, seed, name):
    """(operand, spread index or None, first planted item): boundary words in every row, then (where a prime exceeds gamma)
    the v_gamma plants, then the two r = 0 items"""
    rng = np.random.default_rng(seed)
    parts = [R.boundary_rows(ref.q, n, (max(2, R.lead_for(n, 7, n == 8)),), R.boundary_words, rng)]
    idx = None
    try:
        row = ref.row_above(ref.gamma)
        idx, items = M.spread(n, len(ref.vg_targets()), plant_items(n))
        parts.append(ref.plant_vg(rows(rng, ref.q, n, (items,)), row, *M.targets_at(idx, ref.vg_targets())))
    except M.NotPlantable:
        assert (name, "vg") in NOT_PLANTABLE, name
    else:
        assert (name, "vg") not in NOT_PLANTABLE, name
    try:
        parts.append(ref.r_zero_columns(n))
    except M.NotPlantable:
        assert 2 * ref.t >= ref.prod_q  # (the level's modulus is too small for any small non-zero column to round to 0)
        parts.append(np.zeros((1, ref.k, n), dtype=np.uint64))
    return np.concatenate(parts), idx, len(parts[0])


def lift_columns(n):
    """the columns of a ring that the multiply operands plant: 32 at each end of either half, so that both members of a
    pair (c, c + n / 2) and the corners of both halves are planted"""
    half = np.concatenate([np.arange(32), np.arange(n // 2 - 32, n // 2)])
    return np.concatenate([half, half + n // 2])


def lift_operand(ref, n, size, count, seed):
    """a[count][size][k][n]: random residues, with r_m_tilde planted on lift_columns(n) of every polynomial (the targets
    shifted by one per polynomial)"""
    rng = np.random.default_rng(seed)
    x = rows(rng, ref.q, n, (count, size))
    cols = lift_columns(n)
    row = ref.row_above(M.MT)
    nt = len(M.R_M_TILDE_TARGETS)
    idx, _ = M.spread(len(cols), nt, count, pairs=True)
    for j in range(size):
        shifted = np.where(idx >= 0, (idx + j) % nt, -1)
        sub = np.ascontiguousarray(x[:, j][:, :, cols])
        x[:, j][:, :, cols] = ref.plant_r_m_tilde(sub, row, *M.targets_at(shifted, M.R_M_TILDE_TARGETS))
    return x


# (log n, prime class of oracle_lib.bfv_plan_contexts, t, level, lift instance, split, lift_top): the cheapest case of the
# grid per instance of the fused lift with at least two primes in the level, so that the solved word has a rest of the
# column to be solved against. Exact k with split 31 and the top layer is not on the grid: the top layer needs primes
# below 2^59, and on the grid those levels take split 30 (test_lift_cases_are_the_grid_s_cells).
LIFT_CASES = (
    (14, "50", T_SMALL, 2, 2, 30, 1),
    (12, "50", T_SMALL, 2, 2, 30, 0),
    (12, "61", T_SMALL, 4, 4, 31, 0),
    (12, "50", T_SMALL, 16, O.BEHZ_GENERIC, 31, 0),
    (12, "50", T_SMALL, 33, O.BEHZ_STEPWISE, 31, 0),
)
LIFT_IDS = ["exact30-top", "exact30", "exact31", "runtime-k", "stepwise"]


@functools.lru_cache(maxsize=None)
def plan_grid():
    return O.bfv_plan_contexts(json.load(open(os.path.join(HERE, "golden", "behz_instance_classes.json"))))


def lift_case_mods(logn, name, t):
    return next(mods for lg, nm, mods, tt in plan_grid() if (lg, nm, tt) == (logn, name, t))


def lift_ref(logn, name, t, k):
    mods = lift_case_mods(logn, name, t)
    return M.RnsRef(mods[:k], t, aux(1 << logn, len(mods)))


# ---------------------------------------------------------------- the oracle, item by item
def oracle_unit(fn, rt, x, out_rows):
    out = np.zeros((x.shape[0], out_rows, x.shape[2]), dtype=np.uint64)
    for i in range(x.shape[0]):
        fn(rt, O.ptr(np.ascontiguousarray(x[i])), O.ptr(out[i]))
    return out


def oracle_bconv(octx, ref, entry, x):
    rt = octx.rns_tool(ref.k)
    out_rows = {"fastbconv_m_tilde": ref.Bsk_size + 1, "sm_mrq": ref.Bsk_size, "fast_floor": ref.Bsk_size,
                "fastbconv_sk": ref.k}[entry]
    return oracle_unit(getattr(L, "ref_" + entry), rt, x, out_rows)


def lazy_forward_exact(mods, logn):
    """the reference's uncorrected forward transform (PARITY) stays below 2^64 on words below 2p: each of its log n layers
    adds at most 2p. Past that it wraps, the NTT form of the level-down is no longer the rounded quotient, and the
    reference's own words are PARITY's contract (the oracle decides alone); STRICT corrects every layer and is exact"""
    return all((2 * logn + 2) * int(p) <= 1 << 64 for p in mods)


def oracle_down(octx, k, x, ntt, strict=0):
    """divide_and_round_q_last on a copy, item by item: the first k - 1 rows"""
    rt = octx.rns_tool(k)
    out = x.copy()
    for i in range(len(out)):
        if ntt:
            L.ref_divide_and_round_q_last_ntt_inplace(rt, O.ptr(out[i]), octx.c.key_tables, strict)
        else:
            L.ref_divide_and_round_q_last_inplace(rt, O.ptr(out[i]))
    return np.ascontiguousarray(out[:, :k - 1])


def oracle_ntt_rows(octx, x):
    """the oracle's forward transform (every layer corrected: exact for every prime) of every row of x[items][k][n]"""
    out = x.copy()
    for i in range(out.shape[0]):
        for r in range(out.shape[1]):
            L.ref_ntt_forward(O.ptr(out[i, r]), octx.tables(r), 1)
    return out


def oracle_dsr(octx, k, x):
    out = np.zeros((x.shape[0], x.shape[2]), dtype=np.uint64)
    for i in range(len(x)):
        assert L.ref_decrypt_scale_and_round(C.byref(octx.c), k, O.ptr(np.ascontiguousarray(x[i])), O.ptr(out[i])) == 0
    return out


def _u64_rows(xn, ref, logn):
    """the integers' inverse transform of NTT-form rows"""
    return np.array([[[int(v) for v in ntt.inverse(row)] for ntt, row in zip(math_ntts(ref, logn), item)] for item in xn],
                    dtype=np.uint64)


def math_ntts(ref, logn):
    return [_math_ntt(logn, p) for p in ref.q]


@functools.lru_cache(maxsize=None)
def _math_ntt(logn, p):
    return O.MathNtt(logn, p)


# ---------------------------------------------------------------- coverage of a plant, by the integers alone
def assert_covers(deciding, index, targets, threshold, what):
    """the deciding intermediate equals its target on every planted column, every target is planted in both lanes, and the
    batch has columns on both sides of `x > threshold`"""
    tg, mask = M.targets_at(index, targets)
    assert (deciding[mask] == tg[mask]).all(), what
    assert M.both_lanes(index, len(targets)), what
    assert {int(v) for v in deciding[mask]} == {int(v) for v in targets}, what
    side = deciding[mask] > threshold
    assert side.any() and not side.all(), what
    for edge in (threshold, threshold + 1):
        assert edge in {int(v) for v in deciding[mask]}, (what, "the words on either side of the comparison")


# ---------------------------------------------------------------- 1. constants
def _mods(ptr, count):
    return [int(ptr[i].value) for i in range(count)]


def _words(ptr, count):
    return [int(ptr[i]) for i in range(count)]


def _same_converter(bc, conv, what):
    assert (bc.isize, bc.osize) == (len(conv.ibase), len(conv.obase)), what
    assert _mods(bc.ibase, bc.isize) == conv.ibase and _mods(bc.obase, bc.osize) == conv.obase, what
    assert _words(bc.inv_punct, bc.isize) == conv.inv_punct, what
    assert _words(bc.matrix, bc.isize * bc.osize) == [m for row in conv.matrix for m in row], what


def assert_same_constants(rt, ref):
    rt = rt.contents
    k, nb = ref.k, ref.Bsk_size
    assert (rt.q_size, rt.B_size, rt.Bsk_size) == (k, ref.B_size, nb)
    assert _mods(rt.q, k) == ref.q and _mods(rt.Bsk, nb) == ref.Bsk
    assert (int(rt.m_tilde.value), int(rt.m_sk.value), int(rt.gamma.value), int(rt.t.value)) == (M.MT, ref.m_sk, ref.gamma, ref.t)
    for name in ("q_to_Bsk", "q_to_m_tilde", "B_to_q", "B_to_m_sk"):
        _same_converter(getattr(rt, name), getattr(ref, name), name)
    assert _words(rt.prod_B_mod_q, k) == ref.prod_B_mod_q
    assert _words(rt.inv_prod_q_mod_Bsk, nb) == ref.inv_prod_q_mod_Bsk
    assert _words(rt.prod_q_mod_Bsk, nb) == ref.prod_q_mod_Bsk
    assert _words(rt.inv_m_tilde_mod_Bsk, nb) == ref.inv_m_tilde_mod_Bsk
    assert int(rt.inv_prod_B_mod_m_sk) == ref.inv_prod_B_mod_m_sk
    assert int(rt.inv_prod_q_mod_m_tilde) == ref.inv_prod_q_mod_m_tilde
    if k > 1:
        assert _words(rt.inv_q_last_mod_q, k - 1) == ref.inv_q_last_mod_q


@pytest.mark.parametrize("t", [T_SMALL, T_59], ids=["t_small", "t_59"])
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("logn", [3, 8])
def test_oracle_constants_are_the_integers(logn, name, t):
    octx = oracle_context(chain64(name, logn, key_count(logn)), logn, t)
    for k in levels(logn):
        assert_same_constants(octx.rns_tool(k), rns(name, logn, k, t, key_count(logn)))


def test_base_b_grows_at_the_bucket_sizes():
    """|B| = k + 1 occurs with k exactly a bucket size (the tb[KMAX + 1] arrays full), and |B| = k with the small t"""
    for k in BCONV_LEVELS:
        assert rns("P61", 3, k, T_59).B_size == k + 1 and rns("P61", 3, k, T_SMALL).B_size == k
        assert rns("PMIN", 3, k, T_59).B_size == k
    assert {4, 8, 16, 32} <= set(BCONV_LEVELS)


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("logn", [3, 8])
def test_oracle_constants_of_the_level_down_chains(logn, name):
    octx = oracle_context(tuple(R.chain(name, logn)), logn, 2)
    for k in DOWN_LEVELS:
        assert_same_constants(octx.rns_tool(k), rns_down(name, logn, k))


# ---------------------------------------------------------------- 2 and 3. functions and coverage
@pytest.mark.parametrize("t", [T_SMALL, T_59], ids=["t_small", "t_59"])
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("logn", [3, 8])
def test_oracle_base_conversions_are_the_integers(logn, name, t):
    n = 1 << logn
    octx = oracle_context(chain64(name, logn, key_count(logn)), logn, t)
    for k in levels(logn):
        ref = rns(name, logn, k, t, key_count(logn))
        ops = bconv_operands(ref, n, 1000 * logn + k)
        what = "%s N=%d k=%d" % (name, n, k)
        for entry, (x, idx) in ops.items():
            exp = getattr(ref, entry)(x)
            assert np.array_equal(oracle_bconv(octx, ref, entry, x), exp), (entry, what)
        x, idx = ops["sm_mrq"]
        assert_covers(ref.sm_mrq(x, deciding=True)[1], idx, M.R_M_TILDE_TARGETS, (1 << 31) - 1, "r_m_tilde " + what)
        x, idx = ops["fastbconv_sk"]
        assert_covers(ref.fastbconv_sk(x, deciding=True)[1], idx, ref.alpha_sk_targets(), ref.m_sk >> 1, "alpha_sk " + what)


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("logn", [3, 8])
def test_oracle_level_down_is_the_integers(logn, name):
    n = 1 << logn
    octx = oracle_context(tuple(R.chain(name, logn)), logn, 2)
    for k in DOWN_LEVELS:
        ref = rns_down(name, logn, k)
        x = down_operand(ref, n, 10 * logn + k)
        what = "%s N=%d k=%d" % (name, n, k)
        exp, last = ref.divide_and_round_q_last(x, deciding=True)
        assert np.array_equal(oracle_down(octx, k, x, False), exp), what
        xn = oracle_ntt_rows(octx, x)
        exp_ntt, last_ntt = ref.divide_and_round_q_last_ntt(xn, math_ntts(ref, logn), deciding=True)
        assert np.array_equal(oracle_down(octx, k, xn, True, strict=1), exp_ntt), what + " (NTT form, STRICT)"
        if lazy_forward_exact(ref.q, logn):
            assert np.array_equal(oracle_down(octx, k, xn, True), exp_ntt), what + " (NTT form, PARITY)"
        assert (_u64_rows(xn, ref, logn) == x).all()  # the transform of the planted rows, exactly
        assert (last == last_ntt).all()
        # coverage: every ordered pair (boundary word, last word) in every row above the last, and the sum last + half on
        # both sides of the wrap past q_last
        p, half = ref.q[-1], ref.q[-1] >> 1
        for r in range(k - 1):
            have = {(int(a), int(b)) for a, b in zip(x[:, r].ravel(), x[:, -1].ravel())}
            assert {(a, b) for a in R.boundary_words(ref.q[r]) for b in ref.last_words()} <= have, what
        for lane in (0, 1):  # every planted last word in both lanes
            assert set(ref.last_words()) <= {int(v) for v in x[:, -1, lane::2].ravel()}, what
        wrapped = x[:, -1].astype(object) + half >= p
        assert wrapped.any() and not wrapped.all()
        assert {0, p - 1, p - 2, half, half - 1} <= {int(v) for v in last.ravel()}, what


def test_the_rings_where_the_parity_level_down_is_exact():
    """N = 8 on every chain, every ring on the smallest primes; 61-bit rows wrap from N = 16 on"""
    for logn in (3, 8, 9, 13):
        for name in CHAINS:
            assert lazy_forward_exact(R.chain(name, logn)[:4], logn) == (logn == 3 or name == "PMIN"), (logn, name)


def test_level_down_meets_both_arms_of_the_prime_comparison():
    """on PMIX the last prime has 20, 45 and 61 bits in turn: Q.p < L.p is false for every row, true for one of two, true
    for two of three"""
    for logn in (3, 8):
        arms = [[rns_down("PMIX", logn, k).q[i] < rns_down("PMIX", logn, k).q[-1] for i in range(k - 1)] for k in DOWN_LEVELS]
        assert arms == [[False], [False, True], [False, True, True]]


@pytest.mark.parametrize("t", DSR_T, ids=["t=2", "t=786433", "t_59", "t=2^60-93"])
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("logn", [3, 8])
def test_oracle_decrypt_scale_and_round_is_the_integers(logn, name, t):
    n = 1 << logn
    count = N_KEY if logn == 3 else 5
    octx = oracle_context(chain64(name, logn, count), logn, t)
    for k in (kk for kk in DSR_LEVELS if kk < count):
        ref = rns(name, logn, k, t, count)
        x, idx, first = dsr_operand(ref, n, 100 * logn + k, name)
        what = "%s N=%d k=%d t=%d" % (name, n, k, t)
        exp, vg, r = ref.decrypt_scale_and_round(x, deciding=True)
        assert np.array_equal(oracle_dsr(octx, k, x), exp), what
        zeros = 2 if 2 * t < ref.prod_q else 1  # the zero item and, where the level admits one, the non-zero one with r = 0
        assert not r[-zeros:].any() and not exp[-zeros:].any() and x[-1].all() == (zeros == 2), what
        assert r[:first].any(), what  # and the other side of `r == 0`
        if idx is not None:
            planted = vg[first:first + idx.shape[0]]
            assert_covers(planted, idx, ref.vg_targets(), ref.gamma >> 1, "v_gamma " + what)


def test_the_chains_that_admit_no_plant_are_the_ones_without_a_large_prime():
    """a plant raises exactly where no prime of the level exceeds the modulus of the solved word; nothing is skipped"""
    declared = set()
    for name in CHAINS:
        for logn in (3, 8, 9):
            for k in (1, 4, key_count(logn) - 1):
                ref = rns(name, logn, k, T_SMALL, key_count(logn))
                x = rows(np.random.default_rng(k), ref.q, 8, (1,))
                for kind, bound, plant, targets in (("r_m_tilde", M.MT, ref.plant_r_m_tilde, M.R_M_TILDE_TARGETS),
                                                    ("vg", ref.gamma, ref.plant_vg, ref.vg_targets())):
                    admits = max(ref.q) > bound
                    assert admits == ((name, kind) not in NOT_PLANTABLE), (name, kind, k)
                    if not admits:
                        declared.add((name, kind))
                        with pytest.raises(M.NotPlantable):
                            ref.row_above(bound)
                        for target in targets:  # every target, on every row
                            for row in range(k):
                                with pytest.raises(M.NotPlantable):
                                    plant(x, row, target)
                        continue
                    row = ref.row_above(bound)
                    for target in targets:
                        y = plant(x, row, target)
                        got = ref.lift_r_m_tilde(y) if kind == "r_m_tilde" else ref.decrypt_scale_and_round(y, deciding=True)[1]
                        assert (got == target).all() and (y < np.array(ref.q, dtype=np.uint64)[None, :, None]).all()
                        assert np.array_equal(np.delete(y, row, axis=1), np.delete(x, row, axis=1))
    assert declared == NOT_PLANTABLE


# ---------------------------------------------------------------- the multiply operands
@pytest.mark.parametrize("case", LIFT_CASES, ids=LIFT_IDS)
def test_multiply_operands_carry_every_r_m_tilde_target(case):
    logn, name, t, k, *_ = case
    n = 1 << logn
    ref = lift_ref(logn, name, t, k)
    cols = lift_columns(n)
    nt = len(M.R_M_TILDE_TARGETS)
    idx, _ = M.spread(len(cols), nt, 3, pairs=True)
    assert (idx >= 0).sum() and ((idx[:, :64] >= 0) == (idx[:, 64:] >= 0)).all()  # both members of a pair, or neither
    for seed in (1, 2):  # the two operands
        a = lift_operand(ref, n, 2, 3, seed)
        assert (a < np.array(ref.q, dtype=np.uint64)[None, None, :, None]).all()
        for j in range(2):
            r = ref.lift_r_m_tilde(np.ascontiguousarray(a[:, j][:, :, cols]))
            tg, mask = M.targets_at(np.where(idx >= 0, (idx + j) % nt, -1), M.R_M_TILDE_TARGETS)
            assert (r[mask] == tg[mask]).all()
            for half in (slice(0, 64), slice(64, 128)):  # either member of the pairs carries every target, in both lanes
                for lane in (0, 1):
                    got = {int(v) for v in r[:, half][:, lane::2][mask[:, half][:, lane::2]]}
                    assert got == set(M.R_M_TILDE_TARGETS), (case, j, lane)


def test_lift_cases_are_the_grid_s_cells():
    """the plans the restatement derives for LIFT_CASES name the instances the cases are listed for, and over the rings
    2^12 and 2^14 of the grid no level runs an exact-k instance with the top layer on primes of 2^59 or more, which is
    where split 31 begins on the exact-k levels the grid has"""
    for logn, name, t, k, inst, split, top in LIFT_CASES:
        plan = O.bfv_multiply_plan(logn, lift_case_mods(logn, name, t), t, k, 2, 2)
        assert (plan["lift_kernel"], plan["lift_top"]) == (inst, top), (logn, name, k)
    import sealhip as S

    cells = set()
    for logn, name, mods, t in plan_grid():
        if logn in (12, 14):  # host-only contexts: the engine's own plan and split
            ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, device=-1)
            for k in range(1, O.BEHZ_EXACT_MAX_K + 1):
                plan = ctx.debug_bfv_multiply_plan(k)
                if plan["lift_kernel"] <= O.BEHZ_EXACT_MAX_K:
                    cells.add((ctx.debug_behz_dot_split(k), plan["lift_top"]))
                    if (logn, name, t, k) in {c[:4] for c in LIFT_CASES}:
                        assert (logn, name, t, k, k, ctx.debug_behz_dot_split(k), plan["lift_top"]) in LIFT_CASES
        for k in range(1, O.BEHZ_EXACT_MAX_K + 1):
            if O.bfv_multiply_plan(logn, mods, t, k, 2, 2)["lift_top"]:
                assert max(mods[:k]) < 1 << 59
    assert cells == {(30, 0), (30, 1), (31, 0)}, cells  # split 31 with the top layer has no level: no case for it
