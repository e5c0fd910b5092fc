"""Polynomial evaluation on CKKS ciphertexts on the device.
Linear combinations over terms at their own level and size (sealhip_evaluator_linear_combination_levels), word for word
against the composition that defines them: drop each term to its first k rows, pad it with zero polynomials to the sum's size,
then tests/poly_eval_ref.linear_combination (ref_multiply_poly_scalar_coeffmod / ref_add_poly_coeffmod). The planned
evaluation (sealhip_evaluator_evaluate_polynomial_ckks) word for word against the restatement tests/poly_eval_ckks_ref.py at
N = 2^12 with eight data primes alternating 39 and 41 bits, its launch counts, its refusals, and one end-to-end case that
decrypts.

Shapes: the smallest that reach every path. Six data primes give a first level of 5; the sums are formed at level 2 from terms
at levels 2, 3 and 5 and of sizes 2 and 3 mixed into a size-3 sum, so every term has a row stride and an item stride of its
own and polynomial 2 sees only some of them. lincomb_levels_kernel takes up to 16 terms and 4 sums per launch: 1 and 5 terms
are one group, 17 a full group and a group of one that adds the partial sum in; 1 sum is one tile, 5 a full tile and a tile of
one. At N = 2^8 a block of 256 pairs straddles two rows (and, at the row 2 k - 1 | 2 k, two polynomials: the per-lane
variant), and three items of 3 x 2 rows leave the last block half full; at N = 2^12 a block lies inside one row (the uniform
variant)."""
import math

import numpy as np
import pytest

import oracle_lib as O
import poly_eval_ckks_ref as PC
import poly_eval_ref as P
from support import BaseSession, S, compile_cpp, rows, run_exe, session_memo, weights


pytestmark = pytest.mark.gpu

BITS = [40, 41, 40, 41, 40, 41]  # five data primes and the special one: levels 1 .. 5
K_FIRST = 5
TILE, GROUP = 4, 16
LEVELS, SIZES = (2, 3, 5), (2, 3)


def _dropped(x, k, size):
    """[size_t][k_t][N] -> [size][k][N]: the first k rows, zero polynomials up to size"""
    out = np.zeros((size, k, x.shape[-1]), dtype=np.uint64)
    out[:x.shape[0]] = x[:, :k]
    return out


class Session(BaseSession):
    def __init__(self, S, logn, mode, count=3):
        super().__init__(S, S.SCHEME_CKKS, logn, BITS, 1, mode, 0, 100 * logn + mode)
        self.count = count
        self.pools = {}

    def term(self, level, size, i):
        """the i-th operand batch count x size x level x N, host and device, made once and never modified"""
        host, dev = self.pools.setdefault((level, size), ([], []))
        while len(host) <= i:
            host.append(rows(self.rng, self.mods[:level], self.n, (self.count, size)))
            dev.append(self.ctx.upload(host[-1]))
        return host[i], dev[i]

    def terms(self, levels, sizes):
        """distinct batches for the terms of one call: the i-th of its (level, size) pair"""
        seen = {}
        out = []
        for lv, sz in zip(levels, sizes):
            out.append(self.term(lv, sz, seen.setdefault((lv, sz), 0)))
            seen[(lv, sz)] += 1
        return out

    def shapes(self, n_terms):
        """levels cycle 2, 3, 5 and sizes 2, 3: every (level, size) pair appears from six terms on"""
        return [LEVELS[i % 3] for i in range(n_terms)], [SIZES[(i // 3 + i) % 2] for i in range(n_terms)]

    def call(self, k, size, levels, sizes, w, kc, entry="levels"):
        hosts, devs = zip(*self.terms(levels, sizes))
        n_sums = w.shape[0]
        dw = self.ctx.upload(np.ascontiguousarray(w))
        dk = self.ctx.upload(np.ascontiguousarray(kc)) if kc is not None else None
        out = self.ctx.alloc(n_sums * self.count * size * k * self.n)
        if entry == "levels":
            self.ev.linear_combination_levels(list(devs), levels, sizes, dw, k, self.count, out, size=size, n_sums=n_sums,
                                              constant=dk)
        else:
            self.ev.linear_combination(list(devs), dw, k, self.count, out, size=size, n_sums=n_sums, constant=dk)
        got = out.download((n_sums, self.count, size, k, self.n)).copy()
        for d in (dw, dk, out):
            if d is not None:
                d.free()
        return hosts, got

    def compare(self, k, size, levels, sizes, n_sums, const, tag, items=None):
        w = weights(self.rng, self.mods[:k], (n_sums, len(levels)))
        kc = weights(self.rng, self.mods[:k], (n_sums,)) if const else None
        hosts, got = self.call(k, size, levels, sizes, w, kc)
        for c in (range(self.count) if items is None else items):
            want = P.linear_combination(self.ref, k, [_dropped(h[c], k, size) for h in hosts], w, kc)
            assert np.array_equal(got[:, c], want), (tag, "item", c)
        return got

    def check_pools_unchanged(self):
        for host, dev in self.pools.values():
            for h, d in zip(host, dev):
                assert np.array_equal(d.download(h.shape), h), "an operand was modified"


_session = session_memo(Session)


def test_export_and_method(S):
    for name in ("linear_combination_levels", "polynomial_plan_ckks", "evaluate_polynomial_ckks"):
        assert hasattr(S.lib(), "sealhip_evaluator_" + name) and callable(getattr(S.Evaluator, name))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("logn", [8, 12])
def test_levels_words(S, logn, mode):
    """output level 2 under a first level of 5, terms at levels 2, 3 and 5, sizes 2 and 3 mixed into a size-3 sum; 1, 5 and 17
    terms; 1 sum and one more than the tile holds; with and without the constant; three items; both modes"""
    se = _session(S, logn, mode)
    for n_terms in (1, 5, 17):
        levels, sizes = se.shapes(n_terms)
        for n_sums in (1, TILE + 1):
            for const in (False, True):
                heavy = n_terms > 5 and n_sums > 1
                se.compare(2, 3, levels, sizes, n_sums, const, (logn, mode, n_terms, n_sums, const),
                           items=(2,) if heavy else None)
    se.check_pools_unchanged()


@pytest.mark.parametrize("logn", [8, 12])
def test_levels_other_output_levels_and_sizes(S, logn):
    """the last level (one row, every term above it), the first level (no term above it) and a size-2 sum of size-2 terms; a
    single size-2 term in a size-3 sum leaves polynomial 2 zero (or the constant-free zero) everywhere"""
    se = _session(S, logn, 0)
    se.compare(1, 3, [5, 2, 3, 1], [3, 2, 2, 3], 2, True, (logn, "k 1"))
    se.compare(K_FIRST, 3, [5, 5, 5], [2, 3, 2], 2, True, (logn, "k first"))
    se.compare(3, 2, [3, 5, 5, 3, 5], [2] * 5, TILE + 1, True, (logn, "size 2"))
    got = se.compare(2, 3, [5], [2], 2, True, (logn, "padded"))
    assert not got[:, :, 2].any() and got[:, :, 1].any()
    se.check_pools_unchanged()


@pytest.mark.parametrize("logn", [8, 12])
def test_equal_levels_and_sizes_give_the_existing_entrys_words(S, logn):
    se = _session(S, logn, 0)
    for k, size, n_terms, n_sums in ((5, 2, 5, 1), (5, 3, 17, TILE + 1), (3, 3, 5, 2)):
        w = weights(se.rng, se.mods[:k], (n_sums, n_terms))
        kc = weights(se.rng, se.mods[:k], (n_sums,))
        _, a = se.call(k, size, [k] * n_terms, [size] * n_terms, w, kc)
        _, b = se.call(k, size, [k] * n_terms, [size] * n_terms, w, kc, entry="plain")
        assert np.array_equal(a, b), (k, size, n_terms, n_sums)


def test_one_term_with_weight_one_is_mod_switch_to(S):
    """a CKKS mod_switch_to any lower level in one pass: the rows below k, nothing else"""
    se = _session(S, 12, 0)
    for k in (4, 1):
        w = np.ones((1, 1, k), dtype=np.uint64)
        hosts, got = se.call(k, 2, [5], [2], w, None)
        assert np.array_equal(got[0], hosts[0][:, :, :k])


def test_levels_transparency_flags(S):
    """one flag per output ciphertext in output order (sum-major): clear for the item whose polynomials 1.. are zero in every
    term and for the sum whose weights are all zero; a size-2 term's missing polynomial 2 counts as zero"""
    se = _session(S, 12, 0)
    ctx, ev, n, k, count, n_sums = se.ctx, se.ev, se.n, 2, 3, TILE + 1
    levels, sizes = se.shapes(17)
    pool = [rows(se.rng, se.mods[:lv], n, (count, sz)) for lv, sz in zip(levels, sizes)]
    for p in pool:
        p[1, 1:] = 0
    dev = [ctx.upload(p) for p in pool]
    w = weights(se.rng, se.mods[:k], (n_sums, 17))
    w[3] = 0
    dw, dk = ctx.upload(w), ctx.upload(weights(se.rng, se.mods[:k], (n_sums,)))
    out = ctx.alloc(n_sums * count * 3 * k * n)
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
        ev.linear_combination_levels(dev, levels, sizes, dw, k, count, out, size=3, n_sums=n_sums, constant=dk)
        got = flags.download().view(np.uint32)
        want = [s != 3 and c != 1 for s in range(n_sums) for c in range(count)]
        assert (got[:15] != 0).tolist() == want and got[15] == 5, got
        res = out.download((n_sums, count, 3, k, n))
        assert res[3, 0, 0].any() and not res[3, :, 1:].any() and not res[:, 1, 1:].any()
        ctx.transparency_sink(flags, 14)  # 15 flags do not fit
        with pytest.raises(ValueError, match="sink"):
            ev.linear_combination_levels(dev, levels, sizes, dw, k, count, out, size=3, n_sums=n_sums, constant=dk)
    finally:
        ctx.transparency_sink(None, 0)


def test_levels_graph_capture(S):
    """capturable after one warm-up call: two groups and two tiles, replayed on new inputs and new weights"""
    se = _session(S, 12, 0)
    ctx, ev, n, k, count, n_sums = se.ctx, se.ev, se.n, 2, 2, TILE + 1
    levels, sizes = se.shapes(17)
    fresh = lambda: [rows(se.rng, se.mods[:lv], n, (count, sz)) for lv, sz in zip(levels, sizes)]
    dev = [ctx.upload(p) for p in fresh()]
    dw = ctx.upload(weights(se.rng, se.mods[:k], (n_sums, 17)))
    dk = ctx.upload(weights(se.rng, se.mods[:k], (n_sums,)))
    out = ctx.alloc(n_sums * count * 3 * k * n)
    run = lambda: ev.linear_combination_levels(dev, levels, sizes, dw, k, count, out, size=3, n_sums=n_sums, constant=dk)
    run()
    g = ctx.capture(run)
    pool = fresh()
    w, kc = weights(se.rng, se.mods[:k], (n_sums, 17)), weights(se.rng, se.mods[:k], (n_sums,))
    for d, p in zip(dev, pool):
        d.upload(p)
    dw.upload(w)
    dk.upload(kc)
    g.launch()
    replayed = out.download((n_sums, count, 3, k, n)).copy()
    want = P.linear_combination(se.ref, k, [_dropped(p[1], k, 3) for p in pool], w, kc)
    assert np.array_equal(replayed[:, 1], want)
    out.upload(np.zeros(n_sums * count * 3 * k * n, dtype=np.uint64))
    run()
    assert np.array_equal(out.download((n_sums, count, 3, k, n)), replayed)


def test_levels_chunk_log_and_refusals_on_a_device(S):
    """the term list is logged as walked in groups of 16 ahead of the batch's one chunk (nothing comes from the arena, so the
    batch never splits); a BFV context and a term below the sum's level are refused on a device as on the host"""
    se = _session(S, 12, 0)
    levels, sizes = se.shapes(17)
    devs = [d for _, d in se.terms(levels, sizes)]
    dw = se.ctx.upload(weights(se.rng, se.mods[:2], (1, 17)))
    out = se.ctx.alloc(se.count * 3 * 2 * se.n)
    se.ctx.chunk_log()
    se.ev.linear_combination_levels(devs, levels, sizes, dw, 2, se.count, out, size=3)
    assert se.ctx.chunk_log() == [(17, GROUP), (se.count, se.count)]
    with pytest.raises(ValueError, match="level"):
        se.ev.linear_combination_levels(devs, levels, sizes, dw, 3, se.count, out, size=3)  # (term 0 is at level 2)
    with pytest.raises(ValueError, match="size"):
        se.ev.linear_combination_levels(devs, levels, sizes, dw, 2, se.count, out, size=2)  # (some terms have size 3)
    mods = O.coeff_modulus_create(1 << 12, [40, 40, 41])
    bfv = S.Context(S.SCHEME_BFV, 12, mods, 1, 65537, mode=S.MODE_STRICT)
    x = bfv.upload(np.zeros((1, 2, 2, 1 << 12), dtype=np.uint64))
    w = bfv.upload(np.ones((1, 1, 2), dtype=np.uint64))
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).linear_combination_levels([x], [2], [2], w, 2, 1, bfv.alloc(2 * 2 * (1 << 12)))


# ---------------------------------------------------------------- evaluate_polynomial_ckks
EBITS = [39, 41] * 4 + [42]  # eight data primes alternating 39 and 41 bits, one special prime
DELTA = 2.0 ** 40
_crng = np.random.default_rng(21)
SHAPES = {
    "d1": (list(_crng.uniform(-1, 1, 2)), 0),
    "d2": (list(_crng.uniform(-1, 1, 3)), 0),
    "d3": (list(_crng.uniform(-1, 1, 4)), 0),
    "d5 m2": (list(_crng.uniform(-1, 1, 6)), 2),
    "d7 auto": (list(_crng.uniform(-1, 1, 8)), 0),                                   # m = 3, g = 3
    "d8 m3": (list(_crng.uniform(-1, 1, 9)), 3),
    "d20 m4 zero chunk": ([0.0 if 8 <= e <= 11 else float(v) for e, v in enumerate(_crng.uniform(-1, 1, 21))], 4),
    "d3 coefficient 1e6": ([0.5, 1.0e6, -0.25, 1.0e6], 0),
    "d15": (list(_crng.uniform(-1, 1, 16)), 0),
}


class PolySession:
    """contexts on both sides, one seeded batch of two ciphertexts at the first level and a random key: the word-for-word
    comparison needs no valid key"""

    def __init__(self, S, mode):
        self.S, self.n, self.count = S, 1 << 12, 2
        self.mods = O.coeff_modulus_create(self.n, EBITS)
        self.k = len(self.mods) - 1
        self.ctx = S.Context(S.SCHEME_CKKS, 12, self.mods, 1, 0, mode=mode)
        self.ref = O.RefContext(S.SCHEME_CKKS, 12, self.mods, nsp=1, t=0, mode=mode)
        self.ev = S.Evaluator(self.ctx)
        rng = np.random.default_rng(77 + mode)
        self.key_host = rows(rng, self.mods, self.n, (self.k, 2))
        self.key = S.KSwitchKeys(self.ctx, self.key_host)
        self.ct = rows(rng, self.mods[:self.k], self.n, (self.count, 2))
        self.dct = self.ctx.upload(self.ct)

    def run(self, coeffs, basis, n_baby, scale_out=0.0, k=None, keys=True):
        k = self.k if k is None else k
        plan = self.ev.polynomial_plan_ckks(k, DELTA, coeffs, basis, n_baby, scale_out, tables=False)
        dct = self.dct if k == self.k else self.ctx.upload(np.ascontiguousarray(self.ct[:, :, :k]))
        out = self.ctx.alloc(self.count * 2 * plan["out_level"] * self.n)
        level, scale = self.ev.evaluate_polynomial_ckks(dct, coeffs, k, self.count, DELTA, out, [self.key] if keys else None,
                                                        basis, n_baby, scale_out)
        got = out.download((self.count, 2, plan["out_level"], self.n)).copy()
        out.free()
        return plan, level, scale, got


_POLY = {}


def _poly_session(S, mode):
    if mode not in _POLY:
        _POLY[mode] = PolySession(S, mode)
    return _POLY[mode]


@pytest.mark.parametrize("basis", [0, 1])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_polynomial_words(S, case, basis):
    """word for word against the restatement (item 1 of a batch of two), the returned level and scale against the plan's;
    d = 7 in STRICT mode and at a lower level with a scale of its own as well"""
    coeffs, n_baby = SHAPES[case]
    runs = [(0, None, 0.0)]
    if case == "d7 auto":
        runs += [(1, None, 0.0), (0, 7, 2.0 ** 38)]
    for mode, k, scale_out in runs:
        se = _poly_session(S, mode)
        k = se.k if k is None else k
        plan, level, scale, got = se.run(coeffs, basis, n_baby, scale_out, k)
        pl, want = PC.evaluate(se.ref, k, se.ct[1][:, :k], DELTA, coeffs, se.key_host, basis, n_baby, scale_out)
        assert (level, scale) == (plan["out_level"], plan["out_scale"]) == (pl["out_level"], pl["out_scale"])
        assert np.array_equal(got[1], want), (case, basis, mode, k)
        assert got[0].any() and not np.array_equal(got[0], got[1])
    se = _poly_session(S, 0)
    assert np.array_equal(se.dct.download(se.ct.shape), se.ct), "the operand was modified"


def _profile(ctx, fn):
    fn()  # (arena, pool and tables in place)
    ctx.profile_enable(True)
    fn()
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    return prof


@pytest.mark.parametrize("basis", [0, 1])
def test_polynomial_work_done_once(S, basis):
    """d = 20, n_baby = 4 (m = 4, g = 6; monomial: chunk 2 identically zero): ONE pass of levels-lincomb launches forms the five
    (Chebyshev: six) inner sums over E_1 .. E_3 read in place (two tiles), ONE rescale serves all of them, ONE tensor_dot and ONE key-switch inner product
    the outer sum; the only row copies are the drops of product operands one level apart and of the outer sum's operands
    above its level -- none for the inner sums"""
    se = _poly_session(S, 0)
    coeffs, n_baby = SHAPES["d20 m4 zero chunk"]
    pl = PC.plan(se.mods[:se.k], se.k, DELTA, coeffs, basis, n_baby)
    out = se.ctx.alloc(se.count * 2 * pl["out_level"] * se.n)
    prof = _profile(se.ctx, lambda: se.ev.evaluate_polynomial_ckks(se.dct, coeffs, se.k, se.count, DELTA, out, [se.key], basis,
                                                                   n_baby))
    print(prof)
    launches = lambda tag: prof.get(tag, {"launches": 0})["launches"]
    J, nb = pl["J"], pl["nb"]
    giants = len([j for j in pl["needed"] if j >= 2])
    # (zero coefficients make a zero chunk in the monomial basis; the T_m-adic expansion of the same list has none)
    assert J == ([1, 3, 4, 5] if basis == 0 else [1, 2, 3, 4, 5]) and nb == 4 and giants == 4
    assert pl["n_products"] == (nb - 1) + giants + 1
    inner = math.ceil((1 + len(J)) / TILE)
    cheb = nb - 1 if basis == 1 else 0  # one combination per Chebyshev step, ahead of its relinearization
    assert launches("lincomb_levels") == inner + 1 + cheb  # (+ 1: out = D + I_0 read in place)
    assert launches("rescale_post") == 1 and launches("lincomb") == 0 and launches("ct_linear") == 0
    assert launches("tensor_dot") == pl["n_products"] and launches("ks_mac") == pl["n_products"]
    drops = sum(pl["lev"][(e + 1) // 2] != pl["lev"][e // 2] for e in range(2, nb + 1))
    drops += sum(pl["glev"][(j + 1) // 2] != pl["glev"][j // 2] for j in pl["needed"] if j >= 2)
    drops += sum((pl["glev"][j] != pl["L_out"]) + (pl["L_I"] != pl["L_out"]) for j in J)
    # the row copies that the steps make inside (the key switch's copy of its target at this ring size, the rescale's copy of
    # the dropped row) are counted from the steps profiled on their own
    k, count, n = se.k, se.count, se.n
    wide, narrow = se.ctx.alloc(count * 3 * k * n), se.ctx.alloc(count * 2 * k * n)
    part = lambda fn: _profile(se.ctx, fn).get("copy_rows", {"launches": 0})["launches"]
    product = part(lambda: se.ev.dot_product_rescale([se.dct], [se.dct], k, count, narrow, [se.key]))
    outer = part(lambda: se.ev.dot_product_rescale([se.dct] * len(J), [se.dct] * len(J), k, count, narrow, [se.key]))
    se.ev.dot_product([se.dct], [se.dct], k, count, wide, None)
    relin = part(lambda: se.ev.relinearize_rescale(wide, k, count, [se.key], narrow))
    plain_dot = part(lambda: se.ev.dot_product([se.dct], [se.dct], k, count, wide, None))
    rescale = part(lambda: se.ev.rescale_to_next(se.dct, 2, k, count, narrow))
    steps = (nb - 1) * (plain_dot + relin if basis == 1 else product) + giants * product
    want = drops + steps + outer + rescale
    assert launches("copy_rows") == want, (launches("copy_rows"), drops, product, outer, relin, plain_dot, rescale)


def test_polynomial_refusals_on_a_device(S):
    """what needs a device to be refused: a key with fewer digits than the level needs; and the empty batch is S_OK"""
    se = _poly_session(S, 0)
    short = S.KSwitchKeys(se.ctx, np.ascontiguousarray(se.key_host[:se.k - 1]))
    out = se.ctx.alloc(se.count * 2 * se.k * se.n)
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        se.ev.evaluate_polynomial_ckks(se.dct, [1.0, 2.0, 3.0], se.k, se.count, DELTA, out, [short])
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        se.ev.evaluate_polynomial_ckks(se.dct, [1.0, 2.0, 3.0], se.k, se.count, DELTA, out, None)
    with pytest.raises(ValueError, match="end of modulus switching chain"):
        se.ev.evaluate_polynomial_ckks(se.dct, [1.0] * 64, 5, se.count, DELTA, out, [se.key])
    assert se.ev.evaluate_polynomial_ckks(se.dct, [1.0, 2.0], se.k, 0, DELTA, out, None) == (se.k - 1, DELTA)


def test_polynomial_transparency_flags(S):
    """one flag per output ciphertext from the read pass: clear for the item whose polynomial 1 is zero (degree one needs no
    key, and a random key would make every result opaque)"""
    se = _poly_session(S, 0)
    ctx, n, k, count = se.ctx, se.n, se.k, 3
    x = rows(np.random.default_rng(9), se.mods[:k], n, (count, 2))
    x[1, 1] = 0
    out = ctx.alloc(count * 2 * (k - 1) * n)
    flags = ctx.alloc(8)
    ctx.transparency_sink(flags, 16)
    try:
        flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
        se.ev.evaluate_polynomial_ckks(ctx.upload(x), [0.25, -0.5], k, count, DELTA, out, None)
        got = flags.download().view(np.uint32)
        assert (got[:3] != 0).tolist() == [True, False, True] and np.all(got[3:] == 5), got
    finally:
        ctx.transparency_sink(None, 0)


def _ring_eval(coeffs, basis, msg):
    n = len(msg)

    def mul(a, b):
        full = np.convolve(a, b)
        out = full[:n].copy()
        out[:n - 1] -= full[n:]
        return out

    one = np.zeros(n)
    one[0] = 1.0
    if basis == 0:
        acc, power = np.zeros(n), one
        for c in coeffs:
            acc, power = acc + c * power, mul(power, msg)
        return acc
    t_prev, t_cur = one, np.array(msg, dtype=float)
    acc = coeffs[0] * t_prev
    for c in coeffs[1:]:
        acc = acc + c * t_cur
        t_prev, t_cur = t_cur, 2.0 * mul(msg, t_cur) - t_prev
    return acc


@pytest.mark.parametrize("basis", [0, 1])
def test_polynomial_end_to_end(S, basis):
    """real keys: encrypt with the oracle's client, evaluate d = 7 on the device, decrypt on the device; within
    2^-20 sum |c_e| of the float evaluation in R[X]/(X^N + 1) (the CPU test's bound), and the restatement's words"""
    logn, n = 12, 1 << 12
    mods = O.coeff_modulus_create(n, EBITS)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ref = O.RefContext(2, logn, mods, nsp=1, t=0, mode=0)
    cl = O.Client(ref, seed=33)
    ev, k = S.Evaluator(ctx), cl.k
    rng = np.random.default_rng(33)
    coeffs = [float(v) for v in rng.uniform(-1, 1, 8)]
    norm = sum(abs(c) for c in coeffs)
    m = np.zeros(n)
    for i, v in {0: 0.3, 1: -0.25, 5: 0.2, 1700: 0.15}.items():
        m[i] = v
    ct = cl.encrypt_poly_ntt([int(round(v * DELTA)) for v in m])
    key_host = cl.relin_key()
    key = S.KSwitchKeys(ctx, key_host)
    plan = ev.polynomial_plan_ckks(k, DELTA, coeffs, basis, tables=False)
    lv = plan["out_level"]
    out = ctx.alloc(2 * lv * n)
    level, scale = ev.evaluate_polynomial_ckks(ctx.upload(ct[None]), coeffs, k, 1, DELTA, out, [key], basis)
    assert (level, scale) == (lv, DELTA)
    got = out.download((2, lv, n))
    dot = ctx.alloc(lv * n)
    ctx.dot_product_ct_sk(out, 2, lv, 1, ctx.upload(cl.sk_powers(1)), True, dot)
    centred, _ = cl.centered_from_ntt_rows(dot.download((lv, n)))
    err = np.max(np.abs(np.array([v / scale for v in centred]) - _ring_eval(coeffs, basis, m)))
    print("end to end basis %d: error %.3e, in units of sum |c_e| %.3e" % (basis, err, err / norm))
    assert err <= 2.0 ** -20 * norm
    assert np.array_equal(got, PC.evaluate(ref, k, ct, DELTA, coeffs, key_host, basis)[1])


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_poly_eval_ckks_check.cpp: the host-ciphertext and the DeviceCiphertext forms give the restatement's
    words on the same seeded inputs, at the plan's level and with the requested scale"""
    logn, n, k = 12, 1 << 12, 8
    mods = O.coeff_modulus_create(n, EBITS)
    exe = compile_cpp(tmp_path, "host_adapter_poly_eval_ckks_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    sm = O.SplitMix(0x4021)
    ct = sm.fill(2 * k, n, mods[:k] * 2).reshape(2, k, n)
    key = sm.fill(8 * 2 * 9, n, mods * 16).reshape(8, 2, 9, n)
    ref = O.RefContext(2, logn, mods, nsp=1, t=0, mode=0)
    coeffs = [0.5, -0.25, 0.125, 0.75, -0.5, 0.0625, 0.3125, -0.875]
    mono = PC.evaluate(ref, k, ct, DELTA, coeffs, key, 0)[1]
    cheb = PC.evaluate(ref, k, ct, DELTA, coeffs, key, 1, 0, 2.0 ** 38)[1]
    for side in ("host", "device"):
        for name, words in (("monomial", mono), ("chebyshev", cheb)):
            line = "%s %s digest %016x meta 1" % (side, name, O.fnv(words))
            assert line in stdout, (line, stdout)
