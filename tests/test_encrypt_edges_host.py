"""tests/encrypt_edge_ref.py against the oracle, without a device: the exact reference equals the oracle's functions, the
planted words reach both sides of every branch they are planted for, and the planting keys give the target polynomial word
for word. tests/test_gpu_encrypt_edges.py relies on all three."""
import ctypes as C

import numpy as np
import pytest

import encrypt_edge_ref as E
import oracle_lib as O

L = O.lib()
PLAIN_MODULI, CHAINS, chains_for = E.PLAIN_MODULI, E.CHAINS, E.chains_for
LOGNS = (4, 11)


def context(name, logn, scheme=1, t=786433):
    bits, nsp = CHAINS[name]
    mods = O.coeff_modulus_create(1 << logn, bits)
    return O.RefContext(scheme, logn, mods, nsp=nsp, t=t if scheme == 1 else 0), mods


@pytest.mark.parametrize("t", PLAIN_MODULI)
def test_delta_m_equals_the_oracle_and_the_estimate_misses(t):
    """items 1 and 2: ref_delta_m = ref_multiply_add_plain_with_scaling_variant on zeros for the planted and 1000 random
    words, at k = 1 and k = k_first; the planted words hold one whose Barrett estimate is one short and one whose estimate
    is exact (a power of two divides 2^128, so its estimate is exact on every word)"""
    rng = np.random.default_rng(t % 1000)
    for name, logn in [(name, logn) for name in chains_for(t) for logn in LOGNS]:  # the chains and rings of the GPU test
        n = 1 << logn
        ref, mods = context(name, logn, t=t)
        for k in sorted({1, ref.k_first}):
            planted = E.planted_plain_words(mods[:k], t)
            words = planted + [int(v) for v in rng.integers(0, t, size=1000, dtype=np.uint64)]
            words += [0] * (-len(words) % n)
            for off in range(0, len(words), n):
                plain = np.array(words[off:off + n], dtype=np.uint64)
                c0 = np.zeros((k, n), dtype=np.uint64)
                L.ref_multiply_add_plain_with_scaling_variant(C.byref(ref.c), k, O.ptr(plain), 0, O.ptr(c0))
                for i, m in enumerate(plain):
                    assert E.ref_delta_m(m, mods[:k], t) == [int(v) for v in c0[:, i]], (name, k, int(m))
            short = exact = 0
            for m in planted:
                num = E.numerator(m, mods[:k], t)
                est = E.barrett_quotient_estimate(num, t)
                assert est in (num // t, num // t - 1), (name, k, m)
                short += est == num // t - 1
                exact += est == num // t
            if t & (t - 1) == 0:
                assert short == 0  # nothing to correct: the correction line cannot be reached with this t
            else:
                assert short >= 1 and exact >= 1, (name, k, short, exact)


def test_barrett_estimate_equals_its_closed_form():
    rng = np.random.default_rng(5)
    for t in PLAIN_MODULI + [3, (1 << 61) - 1]:
        for _ in range(200):
            m = int(rng.integers(0, t, dtype=np.uint64))
            num = m * int(rng.integers(0, t, dtype=np.uint64)) + (t + 1) // 2
            assert E.barrett_quotient_estimate(num, t) == num * ((1 << 128) // t) >> 128


def planted_columns(mods_R):
    """every planted last-row sum with every planted residue of the rows above it"""
    cols = []
    for x_last in E.planted_last_row(mods_R[-1]):
        for kind in range(E.ROW_KINDS):
            cols.append([E.planted_row(p, E.row_temp(x_last, mods_R, r))[kind] for r, p in enumerate(mods_R[:-1])] + [x_last])
    return cols


@pytest.mark.parametrize("name", list(CHAINS))
def test_divround_rows_equals_the_oracle_and_both_sides_are_reached(name):
    """item 3: at every level with an RNSTool, on the planted columns and on random ones; the planted last-row sums wrap and
    do not wrap q_last, and the planted residues give a borrow and a zero in every row's subtraction"""
    logn, n = 6, 1 << 6
    ref, mods = context(name, logn)
    rng = np.random.default_rng(len(name))
    for R in range(2, len(mods) + 1):
        cols = planted_columns(mods[:R])
        traces = []
        for col in cols:
            tr = {}
            E.divround_rows(col, mods[:R], tr)
            traces.append(tr)
        assert any(tr["wrapped"] for tr in traces) and not all(tr["wrapped"] for tr in traces)
        half = mods[R - 1] >> 1
        assert [tr["wrapped"] for tr in traces][::E.ROW_KINDS] == [
            x + half >= mods[R - 1] for x in E.planted_last_row(mods[R - 1])]
        for r in range(R - 1):
            assert any(tr["borrow"][r] for tr in traces) and any(tr["zero"][r] for tr in traces), (R, r)
            assert any(not tr["borrow"][r] and not tr["zero"][r] for tr in traces), (R, r)
        tool = L.ref_context_rns_tool(C.byref(ref.c), R)
        if not tool:
            assert name == "60"  # the oracle builds no RNSTool on 60-bit primes: the GPU test expects from the restatement
            continue
        cols += [[int(rng.integers(0, p, dtype=np.uint64)) for p in mods[:R]] for _ in range(-len(cols) % n or n)]
        for off in range(0, len(cols), n):
            x = E.to_u64([[col[r] for col in cols[off:off + n]] for r in range(R)])
            want = x.copy()
            L.ref_divide_and_round_q_last_inplace(tool, O.ptr(want))
            for i, col in enumerate(cols[off:off + n]):
                assert E.divround_rows(col, mods[:R]) == [int(v) for v in want[:R - 1, i]], (R, col)
            got = x.copy()
            E.divround_restated(got, mods, R, 0, ref.c)
            assert np.array_equal(got[:R - 1], want[:R - 1])


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", ["mixed", "55"])
def test_divround_restated_ntt_branch_equals_the_oracle(name, scheme):
    logn, n = 6, 1 << 6
    ref, mods = context(name, logn, scheme)
    rng = np.random.default_rng(3)
    for R in range(2, len(mods) + 1):
        x = E.to_u64(E.random_rows(rng, mods[:R], n))
        want = x.copy()
        L.ref_divide_and_round_q_last_ntt_inplace(ref.rns_tool(R), O.ptr(want), ref.c.key_tables, 0)
        E.divround_restated(x, mods, R, 1, ref.c)
        assert np.array_equal(x[:R - 1], want[:R - 1])


def test_sample_pairs_wrap_and_reach_zero():
    for p in (O.coeff_modulus_create(16, [30])[0], O.coeff_modulus_create(2048, [60])[0]):
        pairs = E.planted_sample_pairs(p)
        sums = [E.add_small(c, e, p) for c, e in pairs]
        assert all(0 <= c < p and abs(e) <= E.SAMPLE_BOUND for c, e in pairs)
        assert sums.count(0) >= 3 and p - 1 in sums  # two zero sums with e != 0, one wrap to zero from p - 1
        assert any(c + E.lift(e, p) >= p for c, e in pairs) and any(c + E.lift(e, p) < p for c, e in pairs)
        assert (p - 1, 1) in pairs and (0, -1) in pairs and (19, -19) in pairs and (p - 19, 19) in pairs


@pytest.mark.parametrize("logn", LOGNS)
@pytest.mark.parametrize("name", list(CHAINS))
def test_planting_keys_round_trip_on_the_oracle(name, logn):
    """items 4 and 5: encrypt_zero_asymmetric with pk_for_targets and u = (1, 0, .., 0) gives target + lift(e); encrypt_zero_
    symmetric with the ones key, and with sk_for_targets over a seed's expansion (as sampled, and transformed as in the seeded
    branch), gives -(target + lift(e)); the seeds picked have no zero word"""
    n = 1 << logn
    ref, mods = context(name, logn)
    rng = np.random.default_rng(logn + len(name))
    for rows in (len(mods), ref.k_first):
        target = E.random_rows(rng, mods[:rows], n, (2,))
        for r, p in enumerate(mods[:rows]):
            target[0, r, :2] = [0, p - 1]
        e = rng.integers(-19, 20, size=(2, n)).astype(np.int32)
        e[:, :2] = [[1, -1], [0, 19]]
        pk = E.pk_for_targets(ref, target)
        for sign in (1, -1):
            got = np.zeros((2, rows, n), dtype=np.uint64)
            L.ref_encrypt_zero_asymmetric_given(C.byref(ref.c), rows, O.ptr(pk), 0, O.ptr(E.delta_u(n, sign)), O.ptr(e),
                                                O.ptr(got))
            for j in range(2):
                for r, p in enumerate(mods[:rows]):
                    want = [(sign * int(c) + int(ev)) % p for c, ev in zip(target[j, r], e[j])]
                    assert [int(v) for v in got[j, r]] == want, (rows, sign, j, r)
        # symmetric: a = NTT(target) under the ones key
        a = E.ntt_rows(ref, target[0])
        got = np.zeros((2, rows, n), dtype=np.uint64)
        L.ref_encrypt_zero_symmetric_given(C.byref(ref.c), rows, O.ptr(E.ones_key(mods[:rows], n)), 0, O.ptr(a), O.ptr(e[0]),
                                           O.ptr(got))
        for r, p in enumerate(mods[:rows]):
            assert [int(v) for v in got[0, r]] == [-(int(c) + int(ev)) % p for c, ev in zip(target[0, r], e[0])]
            assert [int(v) for v in got[1, r]] == [int(c) for c in target[0, r]]
        # symmetric: a from a seed, the target through the secret key
        for transform in (False, True):
            seed = E.pick_seed(rng, mods[:rows], n, ref, transform)
            sample, a = E.seeded_a(ref, seed, mods[:rows], n, transform)
            assert sample.all() and a.all()
            sk = E.sk_for_targets(ref, target[1], a, mods)
            got = np.zeros((2, rows, n), dtype=np.uint64)
            L.ref_encrypt_zero_symmetric_given(C.byref(ref.c), rows, O.ptr(sk), 0, O.ptr(a), O.ptr(e[1]), O.ptr(got))
            for r, p in enumerate(mods[:rows]):
                assert [int(v) for v in got[0, r]] == [-(int(c) + int(ev)) % p for c, ev in zip(target[1, r], e[1])]


def test_planting_transform_is_exact_where_the_oracle_wraps():
    """ref_ntt_forward's uncorrected butterflies wrap 2^64 on 60-bit primes at 2^11 for some operands; ntt_row then gives the
    transform from its definition. Where the oracle's transform is exact the two are the same words."""
    rng = np.random.default_rng(60)
    ref, mods = context("60", 11)
    wrapped = 0
    for _ in range(40):
        row = E.random_rows(rng, mods[:1], 1 << 11)[0]
        wrapped += not E.round_trips(ref, row, 0)
        out = E.ntt_row(ref, row, 0)
        L.ref_ntt_inverse(O.ptr(out), C.byref(ref.c.key_tables[0]))
        assert [int(v) for v in out] == list(row)
    assert wrapped  # (else this test shows nothing)
    for name, logn in (("55", 11), ("mixed", 4), ("60", 4)):
        ref, mods = context(name, logn)
        for r, p in enumerate(mods):
            row = E.random_rows(rng, [p], 1 << logn)[0]
            assert E.round_trips(ref, row, r)
            assert [int(v) for v in E.ntt_row_raw(ref, row, r)] == list(O.MathNtt(logn, p).forward(row))


def test_a_zero_word_is_refused():
    ref, mods = context("55", 4)
    a = np.ones((3, 16), dtype=np.uint64)
    a[1, 5] = 0
    with pytest.raises(AssertionError, match="zero word"):
        E.sk_for_targets(ref, np.ones((3, 16), dtype=object), a, mods)


def test_planted_words_and_positions():
    mods = O.coeff_modulus_create(16, [30, 40])
    for t in PLAIN_MODULI[:-1]:
        words = E.planted_plain_words(mods, t)
        assert len(set(words)) == len(words) and all(0 <= w < t for w in words)
        rems = {E.numerator(m, mods, t) % t for m in words}
        assert {0, 1 % t, (t - 2) % t, t - 1} <= rems
        assert {0, 1 % t, t - 1, t // 2, (t + 1) // 2 % t} <= set(words)
    q = mods[0]
    # (q is odd: q - half = half + 1, the first sum that wraps)
    assert set(E.planted_last_row(q)) == {0, 1, (q >> 1) - 1, q >> 1, (q >> 1) + 1, (q >> 1) + 2, q - 1}
    assert E.planted_row(q, 0) == [q - 1, 0, 1, 0, q - 1] and E.planted_row(q, q - 1) == [q - 2, q - 1, 0, 0, q - 1]
    pos = E.planted_positions(16, np.random.default_rng(0))
    assert pos[:4] == [0, 1, 14, 15] and 2 <= pos[4] < 14
