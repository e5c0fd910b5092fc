"""The coefficient-wise, Galois and validity kernels of csrc/poly.hip on boundary words: every output word against the
Python-integer references of tests/linear_layer_ref.py and, where the oracle has the function, against the oracle as well
(tests/test_linear_layer_host.py holds the two to each other, so a failure here names the side that disagreed).

Operands come from the builders of linear_layer_ref: 0, 1, 2, (p -+ 1) / 2, p - 2, p - 1 in every row and both lanes, every
ordered pair of them for the binary operations, the words around p, 2p, 4p, 2^63 and 2^64 on the operands documented as any
64-bit word, and the words around the multiples of p below 2^63 for the 63-bit reduction. Chains: 61-bit primes (P61), the
smallest NTT primes of the ring (PMIN) and 61 / 20 / 45 / 61 bits (PMIX), where a row's prime is not monotone in the row
index. Rings: N = 8 (one block spans rows, polynomials and items), 2^8 and 2^9 (either side of "a block covers pairs of one
row"), 2^13 (many blocks per row); 2^12 and 2^16 for the automorphisms. Nothing rests on a tolerance: word for word."""
import ctypes as C

import numpy as np
import pytest

import linear_layer_ref as R
import oracle_lib as O
from support import S, session_memo, top
from test_linear_layer_host import (EXACT_PLAIN_CASES, ct_operands, galois_elements, oracle_multiply_plain, oracle_rows,
                                    plain_chain, plain_moduli, plaintexts, scalars)

pytestmark = pytest.mark.gpu

L = O.lib()
K = 4  # ciphertext primes of every chain


class Session:
    """a BFV context (the Bsk base exists only there) and the oracle's over one chain; every entry tested here is the same
    in both schemes except multiply_plain, which is BFV's"""

    def __init__(self, S, logn, mods, t=2):
        self.logn, self.n, self.kmods, self.t = logn, 1 << logn, [int(p) for p in mods], t
        self.ctx = S.Context(S.SCHEME_BFV, logn, self.kmods, 1, t)
        self.ev = S.Evaluator(self.ctx)
        self.ref = O.RefContext(1, logn, self.kmods, nsp=1, t=t)
        self.mods = self.kmods[:K]

    def row_mods(self, S, k, base):
        """the primes of the rows of one polynomial at level k of a base"""
        if base == S.BASE_Q:
            mods = self.kmods[:k]
        elif base == S.BASE_KEY:
            mods = self.kmods[:k] + self.kmods[K:]
        else:
            mods = [int(p) for p in self.ctx.debug_rns_constants(k, 0)]
        assert len(mods) == self.ctx.rows(k, base)
        return mods


_session = session_memo(Session)


def session(S, logn, name, t=2):
    return _session(S, logn, R.chain(name, logn) if isinstance(name, str) else name, t)


def same(got, exp, what, oracle=None):
    """got == exp word for word; the oracle, where there is one, is held to the integers first"""
    if oracle is not None:
        assert np.array_equal(oracle, exp), "%s: the ORACLE disagrees with the integers" % (what,)
    if not np.array_equal(got, exp):
        at = tuple(int(v[0]) for v in np.nonzero(got != exp))
        raise AssertionError("%s: the KERNEL disagrees with the integers at %s: got %d, expected %d (%d words differ)"
                             % (what, at, int(got[at]), int(exp[at]), int((got != exp).sum())))


# ---------------------------------------------------------------- 1. poly_op_kernel
def run_poly_ops(S, s, k, base, rng):
    ctx, n = s.ctx, s.n
    mods = s.row_mods(S, k, base)
    tag = "N=%d k=%d base=%d" % (n, k, base)

    def binary(fn, ofn, rfn, a, b, name):
        count = a.shape[0]
        exp = rfn(a, b, mods)
        da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(a.size)
        fn(da, db, count, k, out, base=base)
        same(out.download(a.shape), exp, "%s %s" % (name, tag), oracle_rows(ofn, mods, a, b))
        fn(da, db, count, k, da, base=base)  # the result aliases a
        same(da.download(a.shape), exp, "%s in place on a, %s" % (name, tag))
        da.upload(a)
        fn(da, db, count, k, db, base=base)  # the result aliases b
        same(db.download(a.shape), exp, "%s in place on b, %s" % (name, tag))
        if a is not w:  # both operands the same buffer (not the wide words: the second operand is a residue)
            fn(da, da, count, k, out, base=base)
            same(out.download(a.shape), rfn(a, a, mods), "%s of a with itself, %s" % (name, tag))
        before = out.download(a.shape)
        fn(da, db, 0, k, out, base=base)  # an empty batch is a no-op
        assert np.array_equal(out.download(a.shape), before)

    def unary(fn, ofn, rfn, a, name, tail=()):
        count = a.shape[0]
        exp = rfn(a, *tail, mods)
        da, out = ctx.upload(a), ctx.alloc(a.size)
        fn(da, count, k, *tail, out, base=base)
        same(out.download(a.shape), exp, "%s %s" % (name, tag), oracle_rows(ofn, mods, a, tail=tail))
        fn(da, count, k, *tail, da, base=base)
        same(da.download(a.shape), exp, "%s in place, %s" % (name, tag))

    a, b = R.boundary_pairs(mods, n, (), R.boundary_words, R.boundary_words, rng)
    w, c = R.boundary_pairs(mods, n, (), R.wide_words, R.boundary_words, rng, fill_a=R.below_2_64)
    binary(ctx.add_poly_coeffmod, L.ref_add_poly_coeffmod, R.add, a, b, "add")
    binary(ctx.sub_poly_coeffmod, L.ref_sub_poly_coeffmod, R.sub, a, b, "sub")
    binary(ctx.dyadic_product_coeffmod, L.ref_dyadic_product_coeffmod, R.dyadic_product, w, c, "dyadic product")
    x = R.boundary_rows(mods, n, (max(2, R.lead_for(n, 7, n == 8)),), R.boundary_words, rng)
    unary(ctx.negate_poly_coeffmod, L.ref_negate_poly_coeffmod, R.negate, x, "negate")
    v = R.boundary_rows(mods, n, (max(2, R.lead_for(n, 10, n == 8)),), R.words_63, rng, R.below_2_63)
    unary(ctx.modulo_poly_coeffs_63, L.ref_modulo_poly_coeffs_63, R.modulo, v, "modulo 63")
    u = R.boundary_rows(mods, n, (R.lead_for(n, 16, n == 8),), R.wide_words, rng, R.below_2_64)
    for sc in scalars(mods, rng):
        unary(ctx.multiply_poly_scalar_coeffmod, L.ref_multiply_poly_scalar_coeffmod, R.scalar_product, u,
              "scalar product by %d" % sc, tail=(sc,))


@pytest.mark.parametrize("name", R.CHAINS)
@pytest.mark.parametrize("logn", [3, 8, 9, 13])
def test_coefficient_wise_entries_on_boundary_words(S, logn, name):
    """add, sub, negate, dyadic product, scalar product and the 63-bit reduction on the ciphertext base at the top level and
    at k = 1, and on the key and Bsk bases at the top level; out of place, in place on either operand, on an empty batch"""
    s = session(S, logn, name)
    rng = np.random.default_rng(100 * logn + len(name))
    for k, base in ((K, S.BASE_Q), (1, S.BASE_Q), (K, S.BASE_KEY), (K, S.BASE_BSK)):
        run_poly_ops(S, s, k, base, rng)


# ---------------------------------------------------------------- 2. galois_kernel
@pytest.mark.parametrize("name", ["P61", "PMIX"])
@pytest.mark.parametrize("logn", [3, 4, 12, 16])
def test_automorphisms_on_boundary_words(S, logn, name):
    """both forms: every odd element at N = 8 and 16 (the identity included), the elements at the ends of the range, the
    rotation steps and four random ones at 2^12 and 2^16; a zero item stays zero wherever the sign flips"""
    s = session(S, logn, name)
    ctx, n = s.ctx, s.n
    k = 2 if logn == 16 else K
    mods = s.kmods[:k]
    rng = np.random.default_rng(logn)
    # (at N = 8 and 16 as many items as it takes to see every word in both lanes of every row)
    x = R.boundary_rows(mods, n, (1 if logn == 16 else max(2, R.lead_for(n, 7)),), R.boundary_words, rng)
    x = np.concatenate([x, np.zeros_like(x[:1])])
    count = x.shape[0]
    d, o = ctx.upload(x), ctx.alloc(x.size)
    elements = galois_elements(logn, rng)
    assert (1 in elements) == (logn <= 4) and 2 * n - 1 in elements
    assert ctx.galois_elt_from_step(1) in elements or logn <= 4
    for g in elements:
        exp, exp_ntt = R.apply_galois(x, logn, g, mods), R.apply_galois_ntt(x, logn, g)
        ora, ora_ntt = np.empty_like(x), np.empty_like(x)
        for i in range(count):
            for r, p in enumerate(mods):
                m = O.modulus(p)
                L.ref_apply_galois(O.ptr(x[i, r]), logn, g, C.byref(m), O.ptr(ora[i, r]))
                L.ref_apply_galois_ntt(O.ptr(x[i, r]), logn, g, O.ptr(ora_ntt[i, r]))
        o.upload(np.full(x.shape, 7, dtype=np.uint64))  # (every word of the result must be written)
        ctx.apply_galois(d, count, k, g, o)
        same(o.download(x.shape), exp, "apply_galois N=%d element %d" % (n, g), ora)
        o.upload(np.full(x.shape, 7, dtype=np.uint64))
        ctx.apply_galois_ntt(d, count, k, g, o)
        same(o.download(x.shape), exp_ntt, "apply_galois_ntt N=%d element %d" % (n, g), ora_ntt)
        assert not exp[-1].any()
    for bad in (0, 2, 2 * n, 2 * n + 1):
        with pytest.raises(ValueError):
            ctx.apply_galois(d, count, k, bad, o)
        with pytest.raises(ValueError):
            ctx.apply_galois_ntt(d, count, k, bad, o)
    with pytest.raises(ValueError):
        ctx.apply_galois(d, count, k, 3, d)


# ---------------------------------------------------------------- 3. ct_linear_kernel
@pytest.mark.parametrize("name", ["P61", "PMIX"])
@pytest.mark.parametrize("logn", [3, 9])
def test_evaluator_add_sub_negate_over_every_pair_of_sizes(S, logn, name):
    s = session(S, logn, name)
    ctx, ev, n, mods, k = s.ctx, s.ev, s.n, s.mods, K
    rng = np.random.default_rng(logn + 30)
    for sa in (1, 2, 3):
        for sb in (1, 2, 3):
            a, b = ct_operands(mods, n, sa, sb, rng)
            count, so = a.shape[0], max(sa, sb)
            da, db, do = ctx.upload(a), ctx.upload(b), ctx.alloc(count * so * k * n)
            for fn, ofn, subtract in ((ev.add, L.ref_evaluator_add, False), (ev.sub, L.ref_evaluator_sub, True)):
                what = "%s sizes (%d, %d) N=%d" % ("sub" if subtract else "add", sa, sb, n)
                exp = R.ct_add(a, b, mods, subtract)
                ora = np.zeros_like(exp)
                for i in range(count):
                    ofn(C.byref(s.ref.c), k, O.ptr(a[i]), sa, O.ptr(b[i]), sb, O.ptr(ora[i]))
                fn(da, sa, db, sb, k, count, do)
                same(do.download(exp.shape), exp, what, ora)
                if sa >= sb:  # in place on the first operand, as Evaluator::add_inplace
                    fn(da, sa, db, sb, k, count, da)
                    same(da.download(a.shape), exp, what + " in place")
                    da.upload(a)
                else:  # a raw buffer cannot grow
                    with pytest.raises(ValueError):
                        fn(da, sa, db, sb, k, count, da)
            with pytest.raises(ValueError):
                ev.add(da, 0, db, sb, k, count, do)
        exp = R.ct_negate(a, mods)
        ora = np.zeros_like(a)
        for i in range(count):
            L.ref_evaluator_negate(C.byref(s.ref.c), k, O.ptr(a[i]), sa, O.ptr(ora[i]))
        dn = ctx.alloc(a.size)
        ev.negate(da, sa, k, count, dn)
        same(dn.download(a.shape), exp, "negate size %d N=%d" % (sa, n), ora)
        ev.negate(da, sa, k, count, da)
        same(da.download(a.shape), exp, "negate in place size %d N=%d" % (sa, n))


@pytest.mark.parametrize("name", ["P61", "PMIX"])
@pytest.mark.parametrize("logn", [3, 9])
def test_evaluator_multiply_plain_ntt_add_many_and_resize(S, logn, name):
    s = session(S, logn, name)
    ctx, ev, n, mods, k = s.ctx, s.ev, s.n, s.mods, K
    rng = np.random.default_rng(logn + 31)
    one, plain = R.boundary_pairs(mods, n, (), R.boundary_words, R.boundary_words, rng)
    count = one.shape[0]
    for size in (1, 2, 3):
        ct = np.stack([np.roll(one, j, axis=0) for j in range(size)], axis=1).copy()  # the plaintext row meets other words per polynomial
        for stride, pl in ((k * n, plain), (0, plain[:1])):
            exp = R.multiply_plain_ntt(ct, pl, mods)
            ora = ct.copy()
            for i in range(count):
                L.ref_multiply_plain_ntt(C.byref(s.ref.c), k, O.ptr(ora[i]), size, O.ptr(np.ascontiguousarray(pl[i if stride else 0])))
            d = ctx.upload(ct)
            ev.multiply_plain_inplace(d, size, k, count, ctx.upload(pl), stride, ntt_form=True)
            same(d.download(ct.shape), exp, "multiply_plain_ntt size %d stride %d N=%d" % (size, stride, n), ora)
    # add_many: nine ciphertexts of all p - 1, every partial sum at 2p - 2 before its reduction
    full = top(mods, n, (2, 2))
    out = ctx.alloc(full.size)
    ev.add_many([ctx.upload(full) for _ in range(9)], 2, k, 2, out)
    exp = R._u64(np.array([[(9 * (p - 1)) % p] * n for p in mods], dtype=object))
    same(out.download(full.shape), np.broadcast_to(exp, full.shape), "add_many of nine times p - 1, N=%d" % n)
    # resize 2 -> 3: the new polynomial is zero, the old words are unchanged
    two = ct[:, :2].copy()
    dst = ctx.upload(np.full((count, 3, k, n), 7, dtype=np.uint64))
    ev.resize(ctx.upload(two), 2, 3, k, count, dst)
    got = dst.download((count, 3, k, n))
    assert np.array_equal(got[:, :2], two) and not got[:, 2].any()


# ---------------------------------------------------------------- 4. multiply_plain (BFV, coefficient form)
def run_multiply_plain(S, logn, kmods, t, exact):
    """the four coefficient values as monomials and in dense plaintexts, one plaintext per ciphertext and one for all;
    always against the oracle (PARITY: the reference word for word), against the integers where `exact`"""
    s = session(S, logn, kmods, t)
    ctx, ev, n, mods, k = s.ctx, s.ev, s.n, s.mods, K
    rng = np.random.default_rng(logn + 40)
    plain = plaintexts(t, n, rng)
    ct = R.boundary_rows(mods, n, (len(plain), 2), R.boundary_words, rng)
    for stride, pl in ((n, plain), (0, plain[-1:])):
        what = "multiply_plain t=%d stride %d N=%d" % (t, stride, n)
        ora = oracle_multiply_plain(s.ref, k, ct, pl)
        d = ctx.upload(ct)
        ev.multiply_plain_inplace(d, 2, k, len(ct), ctx.upload(pl), stride, ntt_form=False)
        got = d.download(ct.shape)
        if exact:
            same(got, R.multiply_plain(ct, pl, t, mods), what, ora)
        assert np.array_equal(got, ora), what + ": the kernel disagrees with the oracle"


@pytest.mark.parametrize("ti", range(4), ids=["t=2", "t=prime_below_q", "t=2^60-93", "t=2^32"])
@pytest.mark.parametrize("logn,bits", EXACT_PLAIN_CASES + [(9, 61)])
def test_multiply_plain_on_boundary_coefficients(S, logn, bits, ti):
    """Plaintext coefficients exactly at 0, threshold - 1, threshold and t - 1 against ciphertexts of boundary words. At N = 8
    the 61-bit chain and at N = 2^9 a 59-bit chain are where the reference's multiply_plain is the negacyclic product, and
    the integers decide. On the 61-bit chain at N = 2^9 its forward transform's lazy words pass 2^64 and the
    reference's own words are the contract of PARITY mode: the oracle decides alone."""
    kmods = plain_chain(bits, logn)
    t = plain_moduli(kmods[:K])[ti]
    if t >= min(kmods[:K]):  # 2^60 - 93 above the 59-bit primes: no fast plain lift, refused
        s = session(S, logn, kmods, t)
        d = s.ctx.upload(np.zeros((1, 2, K, s.n), dtype=np.uint64))
        with pytest.raises(S.LogicError):
            s.ev.multiply_plain_inplace(d, 2, K, 1, s.ctx.upload(np.zeros(s.n, dtype=np.uint64)), s.n, ntt_form=False)
        return
    run_multiply_plain(S, logn, kmods, t, exact=(logn, bits) in EXACT_PLAIN_CASES)


def test_multiply_plain_refuses_a_plain_modulus_above_a_prime(S):
    s = session(S, 3, "PMIX", (1 << 60) - 93)  # above the 20-bit and the 45-bit row
    d = s.ctx.upload(np.zeros((1, 2, K, 8), dtype=np.uint64))
    with pytest.raises(S.LogicError):
        s.ev.multiply_plain_inplace(d, 2, K, 1, s.ctx.upload(np.zeros(8, dtype=np.uint64)), 8, ntt_form=False)
    assert not d.download().any()


# ---------------------------------------------------------------- 5. out_of_range_kernel
@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("name", ["P61", "PMIX"])
@pytest.mark.parametrize("logn", [3, 9])
def test_is_data_valid_for_at_every_row_and_corner(S, logn, name, size):
    """p - 1 is valid and p is not, at both lanes of the first and of the last pair of every row of every polynomial, all
    items in one batch with the flags back per item; on PMIX a word that is valid under one row's prime and invalid under
    its neighbour's, which is what tests the row -> prime map"""
    s = session(S, logn, name)
    mods = s.mods
    extra = [(3, (1 << 64) - 1, False)]
    if name == "PMIX":
        extra += [(0, mods[1], True), (3, mods[1], True), (1, mods[2], False), (2, mods[0], False), (2, mods[1] - 1, True)]
    ct, valid, labels = R.plants(mods, s.n, size, extra)
    assert np.array_equal(R.is_data_valid_for(ct, mods), valid)
    got = s.ctx.is_data_valid_for(s.ctx.upload(ct), size, K, len(ct))
    wrong = [labels[i] + (": valid" if got[i] else ": invalid") for i in np.nonzero(got != valid)[0]]
    assert not wrong, wrong[:8]
    # the same batch in the other order: a flag belongs to its item, not to its place
    got = s.ctx.is_data_valid_for(s.ctx.upload(ct[::-1].copy()), size, K, len(ct))
    assert np.array_equal(got, valid[::-1])
    # level 1: one row per polynomial
    ct1, valid1, _ = R.plants(mods[:1], s.n, size)
    assert np.array_equal(s.ctx.is_data_valid_for(s.ctx.upload(ct1), size, 1, len(ct1)), valid1)


# ---------------------------------------------------------------- 6. nonzero_tail_kernel
@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("logn", [3, 13])
def test_is_transparent_single_words(S, logn, size):
    """one non-zero word at the first word of polynomial 1, at the last word of the last polynomial, and in polynomial 0
    only (still transparent); transparent and opaque items alternate within the batch"""
    s = session(S, logn, "PMIN")
    ct, labels = R.transparency_plants(K, s.n, size)
    exp = R.is_transparent(ct)
    assert exp.tolist() == [True, False, True, False, True, False, True, False]
    for k, batch in ((K, ct), (1, np.ascontiguousarray(ct[:, :, :1]))):
        ora = [bool(L.ref_is_transparent(C.byref(s.ref.c), k, O.ptr(np.ascontiguousarray(item)), size)) for item in batch]
        want = R.is_transparent(batch)
        assert ora == want.tolist()
        got = s.ctx.is_transparent(s.ctx.upload(batch), size, k, len(batch))
        assert got.tolist() == want.tolist(), [n for n, g, e in zip(labels, got, want) if g != e]
        got = s.ctx.is_transparent(s.ctx.upload(batch[::-1].copy()), size, k, len(batch))
        assert got.tolist() == want[::-1].tolist()
    ones = s.ctx.upload(np.ones((3, 1, K, s.n), dtype=np.uint64))
    assert s.ctx.is_transparent(ones, 1, K, 3).all()  # fewer than two polynomials
