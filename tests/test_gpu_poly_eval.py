"""Polynomial evaluation on the device (sealhip_evaluator_linear_combination / _evaluate_polynomial)
against the oracle: linear combinations word for word against the composition ref_multiply_poly_scalar_coeffmod /
ref_add_poly_coeffmod (tests/poly_eval_ref.linear_combination), polynomial evaluation (BFV STRICT) against the restatement
poly_eval_ref.evaluate_polynomial.

Shapes: the smallest that reach every path. lincomb_kernel takes up to 16 terms per launch: 1, 2 and 5 terms are one group, 17
a full group and a group of one that adds the partial sum in, 33 three groups; and up to 4 sums per launch: 1 and 3 sums are
one tile, 9 two full tiles and a tile of one. Three items with an odd row count give a last block that is not full at
N = 2^8, where a block of 256 pairs also straddles two rows. For the polynomial, N = 2^12 takes the tiled transforms and the
copy + lift front inside dot_product, N = 2^14 the gathered forward transform and the deferred top layer of the inverse."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import poly_eval_ref as P
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe, session_memo, weights

pytestmark = pytest.mark.gpu

TILE, GROUP = 4, 16


class Session(BaseSession):
    """contexts on both sides and a random key: the word-for-word comparison needs no valid key"""

    def __init__(self, S, scheme, logn, bits, nsp, mode, t=0, seed=0):
        super().__init__(S, scheme, logn, bits, nsp, mode, t, seed + logn + len(bits))
        self.key_host = rows(self.rng, self.mods, self.n, (self.nd, 2))
        self.key = S.KSwitchKeys(self.ctx, self.key_host)
        self.pools = {}

    def pool(self, k, size, count, n_terms):
        """n_terms operand batches count x size x k x N, host and device, made once per shape and never modified"""
        key = (k, size, count)
        host, dev = self.pools.setdefault(key, ([], []))
        while len(host) < n_terms:
            host.append(rows(self.rng, self.mods[:k], self.n, (count, size)))
            dev.append(self.ctx.upload(host[-1]))
        return host[:n_terms], dev[:n_terms]

    def lincomb(self, k, size, count, idx, w, kc):
        """the call over the pool's batches idx, weights w [n_sums][len(idx)][k], constant kc [n_sums][k] or None"""
        host, dev = self.pool(k, size, count, 1 + max(idx))
        n_sums = w.shape[0]
        dw = self.ctx.upload(np.ascontiguousarray(w))
        dk = self.ctx.upload(np.ascontiguousarray(kc)) if kc is not None else None
        out = self.ctx.alloc(n_sums * count * size * k * self.n)
        self.ev.linear_combination([dev[i] for i in idx], dw, k, count, out, size=size, n_sums=n_sums, constant=dk)
        got = out.download((n_sums, count, size, k, self.n))
        for d in (dw, dk, out):
            if d is not None:
                d.free()
        return host, got

    def compare_lincomb(self, k, size, count, n_terms, n_sums, const, tag, items=None, idx=None, w=None):
        idx = list(range(n_terms)) if idx is None else idx
        w = weights(self.rng, self.mods[:k], (n_sums, len(idx))) if w is None else w
        kc = weights(self.rng, self.mods[:k], (n_sums,)) if const else None
        host, got = self.lincomb(k, size, count, idx, w, kc)
        for c in (range(count) if items is None else items):
            want = P.linear_combination(self.ref, k, [host[i][c] for i in idx], w, kc)
            assert np.array_equal(got[:, c], want), (tag, "item", c)
        return got

    def check_pools_unchanged(self):
        for host, dev in self.pools.values():
            for h, d in zip(host, dev):
                assert np.array_equal(d.download(h.shape), h), "an operand was modified"


_session = session_memo(Session)


# ---------------------------------------------------------------- linear_combination
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits", [(40, 40, 40, 40), (55, 55, 56, 55)])
def test_lincomb_ckks_words(S, bits, mode):
    """the first level and the last; sizes 2 and 3; one group, a full group plus one, three groups; one tile, two tiles plus
    one; with and without the constant (added at every coefficient of polynomial 0); three items"""
    se = _session(S, S.SCHEME_CKKS, 12, list(bits), 1, mode)
    for k in (3, 1):
        for size in (2, 3):
            for n_terms in (1, 2, 5, 17, 33):
                for n_sums in (1, 3, 9):
                    for const in (False, True):
                        heavy = n_terms > 5 or n_sums > 3
                        se.compare_lincomb(k, size, 3, n_terms, n_sums, const, ("ckks", bits, mode, k, size, n_terms, n_sums, const),
                                           items=(2,) if heavy else None)
    se.check_pools_unchanged()


@pytest.mark.parametrize("size", [2, 3])
def test_lincomb_bfv_words(S, size):
    """BFV STRICT: the constant goes to coefficient 0 of polynomial 0 alone"""
    se = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    for n_terms, n_sums in ((1, 1), (5, 3), (17, 9), (33, 1)):
        for const in (False, True):
            got = se.compare_lincomb(3, size, 3, n_terms, n_sums, const, ("bfv", size, n_terms, n_sums, const), items=(0, 2))
    se.check_pools_unchanged()
    # the constant alone: zero weights leave K at coefficient 0 of polynomial 0 and zeros everywhere else
    w = np.zeros((2, 3, 3), dtype=np.uint64)
    kc = weights(se.rng, se.mods[:3], (2,))
    _, got = se.lincomb(3, size, 3, [0, 1, 2], w, kc)
    want = np.zeros_like(got)
    want[:, :, 0, :, 0] = kc[:, None, :]
    assert np.array_equal(got, want)


def test_lincomb_bfv_parity_mode(S):
    """the entry serves both modes: a PARITY context gives the same words"""
    se = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, 0, t=65537)
    se.compare_lincomb(3, 2, 3, 5, 3, True, "bfv parity")


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_lincomb_small_ring_block_straddles_rows(S, scheme):
    """N = 2^8: a row is 128 coefficient pairs, so every block of 256 lanes covers two rows (two primes, two weights) and the
    last block of the odd row count 3 x 3 x 3 = 27 is half full"""
    if scheme == "bfv":
        se = _session(S, S.SCHEME_BFV, 8, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    else:
        se = _session(S, S.SCHEME_CKKS, 8, [40, 40, 40, 41], 1, 0)
    for n_terms, n_sums in ((2, 1), (17, 9)):
        se.compare_lincomb(3, 3, 3, n_terms, n_sums, True, (scheme, "2^8", n_terms, n_sums))
    se.compare_lincomb(1, 2, 1, 3, 2, True, (scheme, "2^8 one row"))
    se.check_pools_unchanged()


def test_lincomb_two_special_primes(S):
    se = _session(S, S.SCHEME_CKKS, 12, [40] * 5 + [41] * 2, 2, 0)
    for k in (5, 2):
        se.compare_lincomb(k, 2, 3, 17, 5, True, ("ckks nsp 2", k), items=(0, 2))


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_lincomb_repeated_pointers_and_zero_weights(S, scheme):
    """the same buffer in several terms; weights of zero (a whole term, a whole sum, single rows) contribute nothing"""
    if scheme == "bfv":
        se, k = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537), 3
    else:
        se, k = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 40], 1, 0), 3
    idx = [0, 1, 0, 2, 2]
    w = weights(se.rng, se.mods[:k], (3, len(idx)))
    w[:, 1] = 0      # a term nobody uses
    w[1] = 0         # a sum of nothing
    w[2, 3, 1] = 0   # one row of one weight
    got = se.compare_lincomb(k, 2, 2, len(idx), 3, False, (scheme, "repeats"), idx=idx, w=w)
    assert not got[1].any() and got[0].any()
    se.check_pools_unchanged()


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_lincomb_transparency_flags(S, scheme):
    """one flag per output ciphertext in output order (sum-major): set for ordinary inputs, clear for the item whose
    polynomials 1.. are zero in every term, and for the sum whose weights are all zero; the constant touches polynomial 0 only"""
    if scheme == "bfv":
        se, k = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537), 3
    else:
        se, k = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 40], 1, 0), 3
    ctx, ev, n, count, n_terms, n_sums = se.ctx, se.ev, se.n, 3, 17, 5
    pool = [rows(se.rng, se.mods[:k], n, (count, 2)) for _ in range(n_terms)]
    for p in pool:
        p[1, 1] = 0
    dev = [ctx.upload(p) for p in pool]
    w = weights(se.rng, se.mods[:k], (n_sums, n_terms))
    w[3] = 0
    dw, dk = ctx.upload(w), ctx.upload(weights(se.rng, se.mods[:k], (n_sums,)))
    out = ctx.alloc(n_sums * count * 2 * k * n)
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
        ev.linear_combination(dev, dw, k, count, out, n_sums=n_sums, constant=dk)
        got = flags.download().view(np.uint32)
        want = [s != 3 and c != 1 for s in range(n_sums) for c in range(count)]
        assert (got[:15] != 0).tolist() == want and got[15] == 5, got
        res = out.download((n_sums, count, 2, k, n))
        assert res[3, 0, 0].any() and not res[3, :, 1].any() and not res[:, 1, 1].any()
        ctx.transparency_sink(flags, 14)  # 15 flags do not fit
        with pytest.raises(ValueError, match="sink"):
            ev.linear_combination(dev, dw, k, count, out, n_sums=n_sums, constant=dk)
    finally:
        ctx.transparency_sink(None, 0)


def test_lincomb_graph_capture(S):
    """capturable after one warm-up call: three groups and three tiles, replayed on new inputs and new weights"""
    se = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 40], 1, 0)
    ctx, ev, n, k, count, n_terms, n_sums = se.ctx, se.ev, se.n, 3, 2, 33, 9
    dev = [ctx.upload(rows(se.rng, se.mods[:k], n, (count, 2))) for _ in range(n_terms)]
    dw = ctx.upload(weights(se.rng, se.mods[:k], (n_sums, n_terms)))
    dk = ctx.upload(weights(se.rng, se.mods[:k], (n_sums,)))
    out = ctx.alloc(n_sums * count * 2 * k * n)
    run = lambda: ev.linear_combination(dev, dw, k, count, out, n_sums=n_sums, constant=dk)
    run()
    g = ctx.capture(run)
    pool = [rows(se.rng, se.mods[:k], n, (count, 2)) for _ in range(n_terms)]
    w, kc = weights(se.rng, se.mods[:k], (n_sums, n_terms)), weights(se.rng, se.mods[:k], (n_sums,))
    for d, p in zip(dev, pool):
        d.upload(p)
    dw.upload(w)
    dk.upload(kc)
    g.launch()
    replayed = out.download((n_sums, count, 2, k, n)).copy()
    want = P.linear_combination(se.ref, k, [p[1] for p in pool], w, kc)
    assert np.array_equal(replayed[:, 1], want)
    out.upload(np.zeros(n_sums * count * 2 * k * n, dtype=np.uint64))
    run()
    assert np.array_equal(out.download((n_sums, count, 2, k, n)), replayed)


# ---------------------------------------------------------------- evaluate_polynomial
SHAPES = {
    "d1 no keys": ([123, 40000], 0, False),
    "d7 auto": ([5, 0, 65536, 7, 11, 32768, 32769, 99], 0, True),            # m = 3, g = 3, the last inner sum short
    "d8 m3": ([1, 2, 3, 4, 5, 6, 7, 8, 9], 3, True),                          # every inner sum full
    "d9 g1": ([9, 8, 7, 6, 5, 4, 3, 2, 1, 65000], 10, True),                  # one giant step: the plain power basis
    "d20 m4": (list(range(100, 121)), 4, True),                               # g = 6
    "trailing zeros": ([3, 1, 4, 1, 5, 0, 0, 0], 0, True),                    # d = 4 after trimming
    "zero inner sum": ([2, 7, 1, 0, 0, 0, 8, 2, 8], 3, True),                 # I_1 is identically zero: G_1 only feeds G_2
}


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("logn", [12, 14])
def test_polynomial_words(S, logn, name):
    bits, k, count = ([40, 40, 40, 41], 3, 2) if logn == 12 else ([40, 40, 41], 2, 1)
    se = _session(S, S.SCHEME_BFV, logn, bits, 1, S.MODE_STRICT, t=65537)
    coeffs, n_baby, keys = SHAPES[name]
    host, dev = se.pool(k, 2, count, 1)
    out = se.ctx.alloc(count * 2 * k * se.n)
    se.ev.evaluate_polynomial(dev[0], coeffs, k, count, out, [se.key] if keys else None, n_baby=n_baby)
    got = out.download((count, 2, k, se.n))
    out.free()
    c = count - 1  # (one item: the restatement is the slow side)
    want = P.evaluate_polynomial(se.ref, k, host[0][c], coeffs, se.key_host if keys else None, n_baby=n_baby)
    assert np.array_equal(got[c], want), (logn, name)
    if count > 1:
        assert not np.array_equal(got[0], got[1])
    se.check_pools_unchanged()


def test_degree_two_is_multiply_relinearize_and_linear_combination(S):
    """d = 2, n_baby = 3 (g = 1): B_2 from the device's multiply + relinearize, then the device's own linear_combination with
    the tables w(c_1), w(c_2), K(c_0) computed on the host"""
    se = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    ctx, ev, n, k, count, t = se.ctx, se.ev, se.n, 3, 2, 65537
    coeffs = [40000, 65536, 12345]
    host, dev = se.pool(k, 2, count, 1)
    out = ctx.alloc(count * 2 * k * n)
    ev.evaluate_polynomial(dev[0], coeffs, k, count, out, [se.key], n_baby=3)
    prod = ctx.alloc(count * 3 * k * n)
    ev.multiply(dev[0], 2, dev[0], 2, k, count, prod)
    ev.relinearize_inplace(prod, 3, k, count, [se.key])
    b2 = ctx.upload(np.ascontiguousarray(prod.download((count, 3, k, n))[:, :2]))
    w = np.array([[P.bfv_weight(coeffs[1], t, se.mods[:k]), P.bfv_weight(coeffs[2], t, se.mods[:k])]], dtype=np.uint64)
    kc = np.array([P.bfv_constant(se.ref, k, coeffs[0])], dtype=np.uint64)
    lin = ctx.alloc(count * 2 * k * n)
    ev.linear_combination([dev[0], b2], ctx.upload(w), k, count, lin, constant=ctx.upload(kc))
    assert np.array_equal(out.download(), lin.download())


def test_polynomial_refusals_that_need_a_device(S):
    """a key with fewer digits than the level; too small a sink; each leaves the output untouched"""
    se = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    ctx, ev, n, k = se.ctx, se.ev, se.n, 3
    short = S.KSwitchKeys(ctx, rows(se.rng, se.mods, n, (2, 2)))
    host, dev = se.pool(k, 2, 2, 1)
    sentinel = np.full(2 * 2 * k * n, 0x5A5A5A5A, dtype=np.uint64)
    out = ctx.upload(sentinel)
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        ev.evaluate_polynomial(dev[0], [1, 2, 3], k, 2, out, [short])
    flags = ctx.alloc(8)
    ctx.transparency_sink(flags, 1)
    try:
        with pytest.raises(ValueError, match="sink"):
            ev.evaluate_polynomial(dev[0], [1, 2, 3], k, 2, out, [se.key])
    finally:
        ctx.transparency_sink(None, 0)
    assert np.array_equal(out.download(), sentinel)


@pytest.mark.parametrize("name", ["d1 no keys", "d9 g1", "d8 m3", "zero inner sum"])
def test_polynomial_transparency_flags(S, name):
    """one flag per output ciphertext: clear for the item whose c_1 is zero (every power and sum of it is transparent), set for
    the others -- from lincomb_kernel when it stores out (g = 1), from the read pass otherwise"""
    se = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 3
    coeffs, n_baby, keys = SHAPES[name]
    x =rows(se.rng, se.mods[:k], n, (count, 2))
    x[1, 1] = 0
    dx, out = ctx.upload(x), ctx.alloc(count * 2 * k * n)
    flags = ctx.alloc(8)
    ctx.transparency_sink(flags, 16)
    try:
        flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
        ev.evaluate_polynomial(dx, coeffs, k, count, out, [se.key] if keys else None, n_baby=n_baby)
        got = flags.download().view(np.uint32)
        assert (got[:3] != 0).tolist() == [True, False, True] and np.all(got[3:] == 5), got
        res = out.download((count, 2, k, n))
        assert not res[1, 1].any() and res[0, 1].any()
    finally:
        ctx.transparency_sink(None, 0)


def _profile(ctx, fn):
    fn()  # (arena and tables in place)
    ctx.profile_enable(True)
    fn()
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    return prof


def test_polynomial_work_done_once(S):
    """d = 20, n_baby = 4 (m = 4, g = 6): three baby and four giant products, ONE pass of lincomb launches over the baby powers
    (two tiles of sums, one group of terms), ONE tensor_dot, three floors and one key-switch inner product for the outer sum --
    and nothing else: every launch tag of the call is accounted for by seven products and one five-term dot_product profiled on
    their own, the table kernel, the lincomb launches and the final add."""
    se = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 2
    coeffs, n_baby, _ = SHAPES["d20 m4"]
    host, dev = se.pool(k, 2, count, 10)
    out, out3 = ctx.alloc(count * 2 * k * n), ctx.alloc(count * 3 * k * n)
    call = _profile(ctx, lambda: ev.evaluate_polynomial(dev[0], coeffs, k, count, out, [se.key], n_baby=n_baby))

    def product():
        ev.multiply(dev[0], 2, dev[1], 2, k, count, out3)
        ev.relinearize_inplace(out3, 3, k, count, [se.key])

    prod = _profile(ctx, product)
    dot = _profile(ctx, lambda: ev.dot_product(dev[:5], dev[5:10], k, count, out, [se.key]))
    print(call, prod, dot)
    launches = lambda prof, tag: prof.get(tag, {"launches": 0})["launches"]
    n_products = 3 + 4
    extra = {"lincomb": math.ceil(6 / TILE), "poly_tables": 1, "copy_rows": n_products, "ct_linear": 1}
    for tag in set(call) | set(prod) | set(dot) | set(extra):
        want = n_products * launches(prod, tag) + launches(dot, tag) + extra.get(tag, 0)
        assert launches(call, tag) == want, (tag, launches(call, tag), want)
    assert launches(call, "tensor_dot") == 1 and launches(dot, "bfv_floor_sk") == 3 and launches(dot, "ks_mac") == 1
    assert launches(call, "bfv_floor_sk") == 3 * n_products + 3 and launches(call, "ks_mac") == n_products + 1


def test_polynomial_temporaries_go_back_to_the_pool(S):
    """both drivers hold their temporaries in a scoped scratch (csrc/pool_scratch.hpp): a call leaves the pool's bytes in use
    where they were, and once the pool is warm an identical call makes no allocator call (no new miss). BFV d = 20, m = 4
    (g = 6) at N = 2^12, k = 3, two items; CKKS d = 7 (m = 3, g = 3) on the CKKS file's session of the same ring degree. (The
    release when an exception unwinds has no clean trigger here, every refusal coming before the first block is taken: it is
    checked on the CPU over a stub pool, tests/pool_scratch_check.cpp.)"""
    import test_gpu_poly_eval_ckks as PK

    se = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    k, count = 3, 2
    coeffs, n_baby, _ = SHAPES["d20 m4"]
    host, dev = se.pool(k, 2, count, 1)
    out = se.ctx.alloc(count * 2 * k * se.n)
    bfv = lambda: se.ev.evaluate_polynomial(dev[0], coeffs, k, count, out, [se.key], n_baby=n_baby)
    ck = PK._poly_session(S, 0)
    ccoeffs, cbaby = PK.SHAPES["d7 auto"]
    plan = ck.ev.polynomial_plan_ckks(ck.k, PK.DELTA, ccoeffs, 0, cbaby, 0.0, tables=False)
    assert plan["g"] > 1
    cout = ck.ctx.alloc(ck.count * 2 * plan["out_level"] * ck.n)
    ckks = lambda: ck.ev.evaluate_polynomial_ckks(ck.dct, ccoeffs, ck.k, ck.count, PK.DELTA, cout, [ck.key], 0, cbaby, 0.0)
    for ctx, call in ((se.ctx, bfv), (ck.ctx, ckks)):
        call()  # (warm-up: arena, tables and the pool's blocks in place)
        before = ctx.pool_stats()
        call()
        after = ctx.pool_stats()
        call()
        again = ctx.pool_stats()
        print(before, after, again)
        assert before["bytes_in_use"] == after["bytes_in_use"] == again["bytes_in_use"], (before, after, again)
        assert before["misses"] == after["misses"] == again["misses"], (before, after, again)
        assert before["hits"] < after["hits"] < again["hits"], (before, after, again)  # (the blocks do come from the pool)
    out.free()
    cout.free()


def test_polynomial_end_to_end(S):
    """encrypt with the oracle's client, evaluate d = 7 on the device, decrypt on the device: p(m) mod (x^N + 1, t)"""
    logn, n, t = 12, 1 << 12, 65537
    mods = O.coeff_modulus_create(n, [40] * 5 + [41])
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT)
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    cl = O.Client(ref, seed=20)
    ev, k, count = S.Evaluator(ctx), cl.k, 2
    rng = np.random.default_rng(20)
    m = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    coeffs = [int(v) for v in rng.integers(1, t, size=8)]
    coeffs[2] = 0
    ct = np.stack([cl.encrypt_bfv(x) for x in m])
    key_host = cl.relin_key()
    key = S.KSwitchKeys(ctx, key_host)
    out = ctx.alloc(count * 2 * k * n)
    ev.evaluate_polynomial(ctx.upload(ct), coeffs, k, count, out, [key])
    dot, plain = ctx.alloc(count * k * n), ctx.alloc(count * n)
    ctx.dot_product_ct_sk(out, 2, k, count, ctx.upload(cl.sk_powers(1)), False, dot)
    ctx.decrypt_scale_and_round(k, dot, count, plain)
    got = plain.download((count, n))
    ntt = O.MathNtt(logn, t)  # (t = 1 mod 2N: p(m) slot by slot)
    for c in range(count):
        slots = ntt.forward(m[c])
        acc = np.zeros(n, dtype=object)
        for coef in reversed(coeffs):
            acc = (acc * slots + coef) % t
        want = np.array([int(v) for v in ntt.inverse(acc)], dtype=np.uint64)
        assert np.array_equal(got[c], want), c
    assert np.array_equal(out.download((count, 2, k, n))[1], P.evaluate_polynomial(ref, k, ct[1], coeffs, key_host))


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_cpp_adapter(S, tmp_path, scheme):
    """tests/host_adapter_poly_eval_check.cpp: the host-ciphertext and the DeviceCiphertext forms give the ABI's words on the
    same seeded inputs -- linear_combination with BFV scalars mod t and with CKKS doubles at one scale (the residues of
    encode(value, scale): ref_ckks_encode_value + ref_multiply_plain_ntt + add), and evaluate_polynomial"""
    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_poly_eval_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", scheme, *mods, timeout=120)
    sm = O.SplitMix(0x4020)
    terms = [sm.fill(2 * k, n, mods[:k] * 2).reshape(2, k, n) for _ in range(3)]
    key = sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n)
    L = O.lib()
    if scheme == "ckks":
        ref = O.RefContext(2, logn, mods, nsp=1, t=0, mode=0)
        values, scale = [1.5, -2.25, 0.0078125], float(1 << 30)
        acc = np.zeros((2, k, n), dtype=np.uint64)
        for x, v in zip(terms, values):
            plain = np.zeros((k, n), dtype=np.uint64)
            assert L.ref_ckks_encode_value(C.byref(ref.c), k, v, scale, O.ptr(plain)) == 0
            term = x.copy()
            L.ref_multiply_plain_ntt(C.byref(ref.c), k, O.ptr(term), 2, O.ptr(plain))
            nxt = np.zeros_like(acc)
            L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(acc), 2, O.ptr(term), 2, O.ptr(nxt))
            acc = nxt
        lines = ["%s lincomb digest %016x meta 1" % (side, O.fnv(acc)) for side in ("host", "device")]
    else:
        t = 65537
        ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
        scalars = [3, 65536, 40000]
        w = np.array([[P.bfv_weight(c, t, mods[:k]) for c in scalars]], dtype=np.uint64)
        lin = P.linear_combination(ref, k, terms, w)[0]
        coeffs = [7, 0, 65530, 5, 9]
        poly = P.evaluate_polynomial(ref, k, terms[0], coeffs, key)
        lines = ["%s lincomb digest %016x meta 1" % (side, O.fnv(lin)) for side in ("host", "device")]
        lines += ["%s poly digest %016x meta 1" % (side, O.fnv(poly)) for side in ("host", "device")]
    for line in lines:
        assert line in stdout, (line, stdout)


# ---------------------------------------------------------------- the smallest arena (a child process)
LOGN, N = 15, 1 << 15


def _child():
    """CKKS, N = 2^15, k = 3: 17 terms of four size-2 items are 17 x 6 MiB of operands and nine sums 54 MiB of output -- more
    than the 64 MiB arena could stage. lincomb_kernel reads the operands where they are: the chunk loop reserves nothing, the
    batch is one chunk, the term list is logged as walked in groups of 16, and the words are the oracle's."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    mods = O.coeff_modulus_create(N, [40, 40, 40, 41])
    ctx = S.Context(S.SCHEME_CKKS, LOGN, mods, 1, 0)
    ref = O.RefContext(2, LOGN, mods, nsp=1, t=0, mode=0)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(64)
    k, n_terms, n_sums, count = 3, 17, 9, 4
    pool = [rows(rng, mods[:k], N, (count, 2)) for _ in range(n_terms)]
    dev = [ctx.upload(p) for p in pool]
    w, kc = weights(rng, mods[:k], (n_sums, n_terms)), weights(rng, mods[:k], (n_sums,))
    out = ctx.alloc(n_sums * count * 2 * k * N)
    ctx.chunk_log()
    ev.linear_combination(dev, ctx.upload(w), k, count, out, n_sums=n_sums, constant=ctx.upload(kc))
    log = ctx.chunk_log()
    assert log == [(n_terms, GROUP), (count, count)], log  # the term split ahead of the item chunks
    got = out.download((n_sums, count, 2, k, N))
    for c in (0, count - 1):
        assert np.array_equal(got[:, c], P.linear_combination(ref, k, [p[c] for p in pool], w, kc)), c
    ctx.chunk_log()
    ev.linear_combination(dev[:GROUP], ctx.upload(np.ascontiguousarray(w[:, :GROUP])), k, count, out, n_sums=n_sums)
    assert ctx.chunk_log() == [(count, count)]  # (one group: no term split to report)
    print("LINCOMB_ARENA_OK")


def test_lincomb_needs_no_arena():
    run_arena_child(__file__, "LINCOMB_ARENA_OK", timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
