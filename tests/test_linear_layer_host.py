"""The operand builders of tests/linear_layer_ref.py do what they say, and the oracle's coefficient-wise, Galois and
Evaluator-level linear functions agree with the Python-integer references on those operands: at 61-bit primes, at the
smallest NTT primes of the ring and on a mixed chain. No GPU: this pins the oracle itself at the boundary words, so that
tests/test_gpu_linear_layer.py can compare a kernel with either side and say which one disagreed."""
import ctypes as C

import numpy as np
import pytest

import linear_layer_ref as R
import oracle_lib as O

L = O.lib()
WORD_SETS = [(R.boundary_words, R.below_p), (R.wide_words, R.below_2_64), (R.words_63, R.below_2_63)]


def mods_of(name, logn):
    return R.chain(name, logn)[:4]


# ---------------------------------------------------------------- the word sets and the builders
@pytest.mark.parametrize("name", R.CHAINS)
@pytest.mark.parametrize("logn", [3, 9, 16])
def test_word_sets_are_inside_their_documented_ranges(name, logn):
    mods = R.chain(name, logn)
    assert len(set(mods)) == 5 and all(O.is_prime(p) and p % (2 << logn) == 1 and p < 1 << 61 for p in mods)
    for p in mods:
        b, w, w63 = R.boundary_words(p), R.wide_words(p), R.words_63(p)
        assert len(set(b)) == len(b) == 7 or p < 8  # (p = 17 is the smallest prime of any ring: all seven differ)
        assert all(0 <= x < p for x in b) and {0, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2} <= set(b)
        assert set(b) < set(w) and all(0 <= x < 1 << 64 for x in w) and {p, 2 * p, (1 << 64) - 1, (1 << 64) - p} <= set(w)
        assert all(0 <= x < 1 << 63 for x in w63) and w63[-1] == (1 << 63) - 1
        m = ((1 << 63) - 1) // p
        assert {0, p - 1, p, m * p - 1, m * p} <= set(w63) and (m + 1) * p > (1 << 63) - 1


@pytest.mark.parametrize("words,fill", WORD_SETS, ids=["boundary", "wide", "w63"])
@pytest.mark.parametrize("n", [8, 16, 256, 512])
def test_boundary_rows_put_every_word_in_every_row_and_both_lanes(n, words, fill):
    mods = R.chain("PMIX", 3)[:4] if n == 8 else R.chain("PMIX", n.bit_length() - 1)
    nw = len(words(mods[0]))
    for corners in (False, True):
        count = max(2, R.lead_for(n, nw, corners))
        x = R.boundary_rows(mods, n, (count,), words, np.random.default_rng(n), fill)
        assert x.shape == (count, len(mods), n) and x.dtype == np.uint64
        for r, p in enumerate(mods):
            W = set(words(p))
            rows = R.row_words(x, r)
            assert all(int(v) < fill(p) for v in rows.reshape(-1))
            assert W <= {int(v) for v in rows[:, 0::2].reshape(-1)}, (r, "even lane")
            assert W <= {int(v) for v in rows[:, 1::2].reshape(-1)}, (r, "odd lane")
            assert not W >= {int(v) for v in rows.reshape(-1)}, "random words are interleaved"
            for col in R.CORNERS:
                at = {int(v) for v in rows[:, col]}
                assert at <= W and (at == W or not corners), (r, col)


@pytest.mark.parametrize("wa,wb,fa", [(R.boundary_words, R.boundary_words, R.below_p), (R.wide_words, R.boundary_words, R.below_2_64)],
                         ids=["canonical", "wide"])
@pytest.mark.parametrize("n", [8, 256, 512, 8192])
def test_boundary_pairs_put_every_ordered_pair_in_every_row(n, wa, wb, fa):
    logn = n.bit_length() - 1
    mods = R.chain("PMIX", logn)
    a, b = R.boundary_pairs(mods, n, (3,), wa, wb, np.random.default_rng(n), fill_a=fa)
    assert a.shape == b.shape and a.shape[1:] == (3, len(mods), n) and a.shape[0] >= 2
    assert a.shape[0] == max(2, -(-len(wa(mods[0])) * len(wb(mods[0])) // n))
    lanes = set()
    for r, p in enumerate(mods):
        want = {(x, y) for x in wa(p) for y in wb(p)}
        for j in range(3):
            ra, rb = a[:, j, r, :].reshape(-1), b[:, j, r, :].reshape(-1)
            assert want <= {(int(x), int(y)) for x, y in zip(ra, rb)}, (r, j)
            assert all(int(x) < fa(p) for x in ra) and all(int(y) < p for y in rb)
        first = (int(wa(p)[0]), int(wb(p)[0]))
        lanes.add([(int(x), int(y)) for x, y in zip(a[:, 0, r, :].reshape(-1), b[:, 0, r, :].reshape(-1))].index(first) % 2)
    assert lanes == {0, 1}, "a pair changes lane from row to row"
    with pytest.raises(AssertionError):
        R.boundary_pairs(mods, 8, (), wa, wb, np.random.default_rng(0), count=1)


def test_plants_are_what_the_validity_checks_are_told():
    mods = R.chain("PMIX", 3)[:4]
    ct, valid, labels = R.plants(mods, 8, 3, extra=[(0, mods[1], True), (1, mods[2], False), (3, (1 << 64) - 1, False)])
    assert ct.shape == (3 * 4 * 4 * 2 + 3, 3, 4, 8) and len(labels) == len(valid) == ct.shape[0]
    assert [int(np.count_nonzero(item)) for item in ct] == [1] * ct.shape[0]
    assert np.array_equal(R.is_data_valid_for(ct, mods), valid) and valid.sum() == 3 * 4 * 4 + 1
    seen = {(j, r, c % 8) for j, r, c in (tuple(int(v[0]) for v in np.nonzero(item)) for item in ct[:-3])}
    assert seen == {(j, r, c) for j in range(3) for r in range(4) for c in (0, 1, 6, 7)}
    for size in (2, 3):
        ct, names = R.transparency_plants(4, 8, size)
        flags = R.is_transparent(ct)
        assert dict(zip(names, flags))["last word of polynomial 0"] and not dict(zip(names, flags))["first word of polynomial 1"]
        assert not dict(zip(names, flags))["last word of the last polynomial"] and flags[0] and flags[6]
        assert any(flags[i] != flags[i + 1] for i in range(len(flags) - 1))
    assert R.is_transparent(np.ones((2, 1, 4, 8), dtype=np.uint64)).all()


# ---------------------------------------------------------------- the oracle against the integers
def oracle_rows(fn, mods, *operands, tail=()):
    """fn(row pointers.., n, modulus, result) of the oracle over every row of operands [..][rows][n]"""
    out = np.empty_like(operands[0])
    n = out.shape[-1]
    flat = [o.reshape(-1, len(mods), n) for o in operands]
    res = out.reshape(-1, len(mods), n)
    for r, p in enumerate(mods):
        m = O.modulus(int(p))
        for i in range(res.shape[0]):
            rows = [np.ascontiguousarray(f[i, r]) for f in flat]
            tmp = np.empty(n, dtype=np.uint64)
            fn(*[O.ptr(x) for x in rows], n, *tail, C.byref(m), O.ptr(tmp))
            res[i, r] = tmp
    return out


@pytest.mark.parametrize("name", R.CHAINS)
@pytest.mark.parametrize("logn", [3, 9])
def test_oracle_coefficient_wise_functions_on_boundary_words(name, logn):
    n, mods = 1 << logn, mods_of(name, logn)
    rng = np.random.default_rng(logn)
    a, b = R.boundary_pairs(mods, n, (), R.boundary_words, R.boundary_words, rng)
    assert np.array_equal(oracle_rows(L.ref_add_poly_coeffmod, mods, a, b), R.add(a, b, mods))
    assert np.array_equal(oracle_rows(L.ref_sub_poly_coeffmod, mods, a, b), R.sub(a, b, mods))
    assert np.array_equal(oracle_rows(L.ref_sub_poly_coeffmod, mods, a, a), np.zeros_like(a))
    assert np.array_equal(oracle_rows(L.ref_negate_poly_coeffmod, mods, a), R.negate(a, mods))
    w, c = R.boundary_pairs(mods, n, (), R.wide_words, R.boundary_words, rng, fill_a=R.below_2_64)
    assert np.array_equal(oracle_rows(L.ref_dyadic_product_coeffmod, mods, w, c), R.dyadic_product(w, c, mods))
    u = R.boundary_rows(mods, n, (R.lead_for(n, 16, n == 8),), R.wide_words, rng, R.below_2_64)
    for s in scalars(mods, rng):
        got = oracle_rows(L.ref_multiply_poly_scalar_coeffmod, mods, u, tail=(s,))
        assert np.array_equal(got, R.scalar_product(u, s, mods)), s
    v = R.boundary_rows(mods, n, (R.lead_for(n, 10, n == 8),), R.words_63, rng, R.below_2_63)
    assert np.array_equal(oracle_rows(L.ref_modulo_poly_coeffs_63, mods, v), R.modulo(v, mods))


def scalars(mods, rng):
    return [0, 1, min(mods) - 1, max(mods) - 1, max(mods), (1 << 64) - 1, int(rng.integers(0, 1 << 63)) * 2 + 1]


def galois_elements(logn, rng):
    n = 1 << logn
    if logn <= 4:
        return list(range(1, 2 * n, 2))
    step = lambda s: int(L.ref_galois_elt_from_step(n, s, None))
    fixed = [3, 5, n - 1, n + 1, 2 * n - 3, 2 * n - 1, step(1), step(-1), step(n // 2 - 1)]
    return fixed + [int(g) * 2 + 1 for g in rng.integers(0, n, 4)]


@pytest.mark.parametrize("name", R.CHAINS)
@pytest.mark.parametrize("logn", [3, 4, 12])
def test_oracle_automorphisms_on_boundary_words(name, logn):
    n, mods = 1 << logn, mods_of(name, logn)
    rng = np.random.default_rng(logn)
    x = R.boundary_rows(mods, n, (max(2, R.lead_for(n, 7)),), R.boundary_words, rng)
    x = np.concatenate([x, np.zeros_like(x[:1])])  # a zero item: a negated zero stays zero
    for g in galois_elements(logn, rng):
        exp, exp_ntt = R.apply_galois(x, logn, g, mods), R.apply_galois_ntt(x, logn, g)
        got, got_ntt = np.empty_like(x), np.empty_like(x)
        for i in range(x.shape[0]):
            for r, p in enumerate(mods):
                m = O.modulus(p)
                L.ref_apply_galois(O.ptr(x[i, r]), logn, g, C.byref(m), O.ptr(got[i, r]))
                L.ref_apply_galois_ntt(O.ptr(x[i, r]), logn, g, O.ptr(got_ntt[i, r]))
        assert np.array_equal(got, exp), g
        assert np.array_equal(got_ntt, exp_ntt), g
        assert not exp[-1].any() and all(int(v) < p for r, p in enumerate(mods) for v in exp[:, r].reshape(-1)[:64])
        if logn <= 4:  # the vectorised references against the loop in Python integers
            for r, p in enumerate(mods):
                c, t = R.apply_galois_ints(x[0, r], logn, g, p)
                assert c == [int(v) for v in exp[0, r]] and t == [int(v) for v in exp_ntt[0, r]]


def test_automorphism_references_are_the_maps_they_claim():
    """on a polynomial whose NTT is known: the coefficient-form map is x -> x^g, the NTT-form map the same map on the
    evaluations at psi^(2 bitrev(i) + 1)"""
    logn, n = 4, 16
    p = R.chain("PMIN", logn)[1]
    ntt = O.MathNtt(logn, p)
    rng = np.random.default_rng(1)
    a = [int(v) for v in rng.integers(0, p, n)]
    for g in range(1, 2 * n, 2):
        moved = R.apply_galois(np.array([a], dtype=np.uint64), logn, g, [p])[0]
        lhs = ntt.forward([int(v) for v in moved])
        rhs = R.apply_galois_ntt(np.array([ntt.forward(a)], dtype=np.uint64), logn, g)[0]
        assert [int(v) for v in lhs] == [int(v) for v in rhs], g


@pytest.mark.parametrize("name", R.CHAINS)
@pytest.mark.parametrize("logn", [3, 9])
def test_oracle_evaluator_linear_functions_on_boundary_words(name, logn):
    n, kmods = 1 << logn, R.chain(name, logn)
    k, mods = 4, kmods[:4]
    ref = O.RefContext(2, logn, kmods, nsp=1, t=0)
    rng = np.random.default_rng(logn + 1)
    for sa in (1, 2, 3):
        for sb in (1, 2, 3):
            a, b = ct_operands(mods, n, sa, sb, rng)
            for fn, subtract in ((L.ref_evaluator_add, False), (L.ref_evaluator_sub, True)):
                got = np.zeros((a.shape[0], max(sa, sb), k, n), dtype=np.uint64)
                for i in range(a.shape[0]):
                    fn(C.byref(ref.c), k, O.ptr(a[i]), sa, O.ptr(b[i]), sb, O.ptr(got[i]))
                assert np.array_equal(got, R.ct_add(a, b, mods, subtract)), (sa, sb, subtract)
        got = np.zeros_like(a)
        for i in range(a.shape[0]):
            L.ref_evaluator_negate(C.byref(ref.c), k, O.ptr(a[i]), sa, O.ptr(got[i]))
        assert np.array_equal(got, R.ct_negate(a, mods)), sa
    ct, plain = R.boundary_pairs(mods, n, (), R.boundary_words, R.boundary_words, rng)
    ct = np.stack([ct, ct[::-1]], axis=1).copy()  # size 2: the plaintext row meets two different polynomials
    for pl in (plain, plain[:1]):
        got = ct.copy()
        for i in range(ct.shape[0]):
            L.ref_multiply_plain_ntt(C.byref(ref.c), k, O.ptr(got[i]), 2, O.ptr(np.ascontiguousarray(pl[i if len(pl) > 1 else 0])))
        assert np.array_equal(got, R.multiply_plain_ntt(ct, pl, mods)), len(pl)


def ct_operands(mods, n, sa, sb, rng):
    """a[count][sa][k][n], b[count][sb][k][n]: boundary pairs on the polynomials both have, boundary rows on the tail"""
    lo = min(sa, sb)
    a, b = R.boundary_pairs(mods, n, (lo,), R.boundary_words, R.boundary_words, rng)
    if sa != sb:
        tail = R.boundary_rows(mods, n, (a.shape[0], abs(sa - sb)), R.boundary_words, rng)
        if sa > sb:
            a = np.concatenate([a, tail], axis=1)
        else:
            b = np.concatenate([b, tail], axis=1)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def plain_moduli(mods):
    """2, the largest prime below the smallest ciphertext prime, 2^60 - 93 and a power of two"""
    t = min(mods) - 1
    while not O.is_prime(t):
        t -= 1
    return [2, t, (1 << 60) - 93, 1 << 32]


def plaintexts(t, n, rng):
    """[items][n]: the four coefficient values 0, threshold - 1, threshold, t - 1 as monomials (at the first, an inner and
    the last power) and as dense polynomials (the four cycled; random coefficients with the four planted)"""
    thr = (t + 1) // 2
    four = [0, thr - 1, thr, t - 1]
    out = []
    for v, at in zip(four, (0, 1, n // 2 + 1, n - 1)):
        m = np.zeros(n, dtype=np.uint64)
        m[at] = v
        out.append(m)
    out.append(np.array([four[(i + 1) % 4] for i in range(n)], dtype=np.uint64))
    dense = rng.integers(0, t, n, dtype=np.uint64)
    dense[[0, 1, n - 2, n - 1]] = four
    out.append(dense)
    return np.stack(out)


def plain_chain(bits, logn):
    """four ciphertext primes and a special prime, the largest below 2^bits"""
    return O.ntt_primes_below(1 << logn, 1 << bits, 5)


def oracle_multiply_plain(ref, k, ct, plain):
    got = ct.copy()
    for i in range(len(ct)):
        pl = np.ascontiguousarray(plain[i if len(plain) > 1 else 0])
        assert L.ref_multiply_plain(C.byref(ref.c), k, O.ptr(got[i]), ct.shape[1], O.ptr(pl)) == 0
    return got


# where the oracle's multiply_plain is the negacyclic product: 61-bit primes at N = 8, 59-bit primes at N = 2^9. The
# reference's forward transform keeps its lazy words unreduced, 2p more per layer: from N = 2^6 on they pass 2^64
# for a 61-bit prime, and multiply_plain is then a different function, in STRICT mode too (the plaintext's transform is
# never the corrected one). In PARITY that function is the contract; the integers check it where nothing wraps.
EXACT_PLAIN_CASES = [(3, 61), (9, 59)]


@pytest.mark.parametrize("logn,bits", EXACT_PLAIN_CASES)
def test_oracle_multiply_plain_on_boundary_coefficients(logn, bits):
    n, kmods = 1 << logn, plain_chain(bits, logn)
    k, mods = 4, kmods[:4]
    rng = np.random.default_rng(logn + 2)
    for t in plain_moduli(mods):
        if t >= min(mods):
            continue  # (2^60 - 93 on the 59-bit chain: refused, below)
        ref = O.RefContext(1, logn, kmods, nsp=1, t=t)
        plain = plaintexts(t, n, rng)
        assert {0, (t + 1) // 2 - 1, (t + 1) // 2, t - 1} <= {int(v) for v in plain.reshape(-1)} and int(plain.max()) < t
        ct = R.boundary_rows(mods, n, (len(plain), 2), R.boundary_words, rng)
        for pl in (plain, plain[-1:]):
            assert np.array_equal(oracle_multiply_plain(ref, k, ct, pl), R.multiply_plain(ct, pl, t, mods)), (t, len(pl))
    ref = O.RefContext(1, logn, R.chain("PMIX", logn), nsp=1, t=(1 << 60) - 93)
    assert L.ref_multiply_plain(C.byref(ref.c), k, O.ptr(ct[0].copy()), 2, O.ptr(plain[0])) == -1  # t above a prime


def test_negacyclic_reference_against_the_schoolbook_sum():
    rng = np.random.default_rng(3)
    a = [int(v) for v in rng.integers(0, 1 << 61, 8)]
    c = [int(v) - (1 << 59) for v in rng.integers(0, 1 << 60, 8)]
    school = [0] * 8
    for i in range(8):
        for j in range(8):
            school[(i + j) % 8] += a[i] * c[j] * (-1 if i + j >= 8 else 1)
    assert R.negacyclic(a, c) == school
    assert R.centred([0, 2, 3, 4], 5) == [0, 2, -2, -1] and R.centred([0, 1], 2) == [0, -1]
