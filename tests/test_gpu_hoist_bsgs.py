"""Baby-step/giant-step matrix-vector products on the device (sealhip_evaluator_apply_galois_bsgs_plain /
_rotate_vector_bsgs_plain) against the CPU restatement of tests/hoist_bsgs_ref.py, word for word in the
context's mode.

Shapes: as tests/test_gpu_hoist_dot.py, the smallest that reach every path. N = 2^12 takes the tiled transforms, the explicit
mod-up and the moddown_pre / moddown_post back half -- here also at polynomial granularity, for the one-component mod-down;
the gathered mod-up, the CKKS fold and BFV's deferred top layer exist from N = 2^14, the fused mod-down store from 2^15. A
lane of the giant kernel holds four ciphertexts, so eleven give a short last group. Seventeen digits and rings below a
workgroup take the loop kernel; seventeen giants take two launches of the giant kernel and of the BASE update, the second
adding into what the first left."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import hoist_bsgs_ref as HB
import hoist_ref as H
import noise_ref as NR
import oracle_lib as O
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe

pytestmark = pytest.mark.gpu


def _baby(n):
    """a rotation, the identity, another rotation, the first again"""
    return [H.elt_from_step(n, 1), 1, H.elt_from_step(n, -3), H.elt_from_step(n, 1)]


def _giant(n):
    """a rotation, conjugation, the identity, the first again: a run of two non-identity giants, then a run of one"""
    return [H.elt_from_step(n, 4), 2 * n - 1, 1, H.elt_from_step(n, 4)]


class Session(BaseSession):
    """contexts on both sides and random keys: the word-for-word comparison needs no valid keys"""

    def __init__(self, S, scheme, logn, bits, nsp, mode, t=0, seed=0):
        super().__init__(S, scheme, logn, bits, nsp, mode, t, seed + logn + len(bits))
        self.keys = {}

    def key(self, g):
        if g == 1:
            return None, None
        if g not in self.keys:
            host = rows(self.rng, self.mods, self.n, (self.nd, 2))
            self.keys[g] = (host, self.S.KSwitchKeys(self.ctx, host))
        return self.keys[g]

    def compare(self, k, count, baby, giant, tag, items=None):
        n = self.n
        ct = rows(self.rng, self.mods[:k], n, (count, 2))
        plains = rows(self.rng, self.mods, n, (len(giant), len(baby)))
        d, dp = self.ctx.upload(ct), self.ctx.upload(plains)
        out = self.ctx.alloc(count * 2 * k * n)
        bk, gk = [self.key(g) for g in baby], [self.key(g) for g in giant]
        self.ev.apply_galois_bsgs_plain(d, k, count, baby, [kk[1] for kk in bk], giant, [kk[1] for kk in gk], dp, out)
        got = out.download((count, 2, k, n))
        assert np.array_equal(d.download(ct.shape), ct), (tag, "the input was modified")
        assert np.array_equal(dp.download(plains.shape), plains), (tag, "the plaintexts were modified")
        want = HB.bsgs(self.ref, k, ct, baby, [kk[0] for kk in bk], giant, [kk[0] for kk in gk], plains, items)
        for c in (range(count) if items is None else items):
            assert np.array_equal(got[c], want[c]), (tag, "item", c)
        for b in (d, dp, out):
            b.free()
        return ct, plains, got


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits", [[40, 40, 40, 40], [55, 55, 56, 55]])
def test_ckks_words(S, bits, mode):
    """the FP64 and the integer transform instances, PARITY and STRICT; the first level and one below; the identity and a
    repeat on each axis"""
    se = Session(S, S.SCHEME_CKKS, 12, bits, 1, mode)
    for k in (3, 2):
        se.compare(k, 3, _baby(se.n), _giant(se.n), ("ckks", bits, mode, k), items=(0, 2))


@pytest.mark.parametrize("mode", [0, 1])
def test_ckks_two_special_primes(S, mode):
    """five ciphertext primes in bundles of two: the last bundle is short; two special rows in the one-component mod-down"""
    se = Session(S, S.SCHEME_CKKS, 12, [40] * 5 + [41] * 2, 2, mode)
    for k in (5, 2):
        se.compare(k, 2, _baby(se.n)[:3], _giant(se.n)[1:], ("ckks nsp 2", mode, k), items=(1,))


@pytest.mark.parametrize("logn", [12, 14])
def test_bfv_strict_words(S, logn):
    """coefficient-form ciphertexts: d_j in coefficient form, base_j and BASE in NTT form until the end; 2^14 has the deferred
    top layer in both mod-downs"""
    se = Session(S, S.SCHEME_BFV, logn, [40, 40, 40, 41] if logn == 12 else [40, 40, 41], 1, S.MODE_STRICT, t=65537)
    k = 3 if logn == 12 else 2
    se.compare(k, 2, _baby(se.n)[:3], _giant(se.n)[1:], ("bfv", logn), items=(1,))


@pytest.mark.parametrize("logn,mode", [(14, 0), (15, 0), (15, 1)])
def test_single_pass_transform_paths(S, logn, mode):
    """gathered mod-up and the CKKS fold (2^14), its fused mod-down store (2^15), both at polynomial granularity too"""
    se = Session(S, S.SCHEME_CKKS, logn, [40, 40, 41], 1, mode)
    se.compare(2, 2, _baby(se.n)[:2], _giant(se.n)[1:3], ("single pass", logn, mode), items=(1,))


@pytest.mark.parametrize("k", [1, 5, 16, 17])
def test_digit_counts(S, k):
    """nsp = 1, so ND = k: the smallest instance, the fifth, the sixteenth, and the loop kernel at seventeen digits"""
    se = _digit_session(S)
    se.compare(k, 2, _baby(se.n)[:2], _giant(se.n)[1:3], ("digits", k), items=(1,))


_DIGITS = {}


def _digit_session(S):
    if "s" not in _DIGITS:
        _DIGITS["s"] = Session(S, S.SCHEME_CKKS, 12, [40] * 17 + [41], 1, S.MODE_PARITY)
    return _DIGITS["s"]


def test_ring_smaller_than_a_workgroup(S):
    """N = 2^6: a workgroup spans several rows, the per-lane loop kernel"""
    se = Session(S, S.SCHEME_CKKS, 6, [50] * 3 + [51], 1, S.MODE_PARITY)
    for k in (3, 1):
        se.compare(k, 3, _baby(se.n), _giant(se.n), ("ring 6", k))


def test_loop_kernel_second_launch_adds(S):
    """N = 2^7 and 17 distinct giants: the second launch of the per-lane loop kernel adds into ACC"""
    se = Session(S, S.SCHEME_CKKS, 7, [50] * 3 + [51], 1, S.MODE_PARITY)
    se.compare(3, 2, _baby(se.n)[:2], [2 * i + 3 for i in range(17)], "ring 7, 17 giants")


def test_more_giants_and_babies_than_one_launch(S):
    """17 giants (the identity 12th, one repeated): the second launch of the giant kernel and of the BASE update adds; 17
    babies: the second launch of section 16's kernels adds into workspace"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 41], 1, S.MODE_PARITY)
    many = [2 * i + 3 for i in range(17)]
    many[11] = 1
    many[14] = many[2]
    se.compare(2, 2, _baby(se.n)[:2], many, "17 giants", items=(1,))
    se.compare(2, 2, many, _giant(se.n)[1:3], "17 babies", items=(1,))


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_degenerate_shapes(S, scheme):
    """all babies 1 with non-identity giants (no acc_j: d_j = base_j[1], no one-component mod-down); all giants 1 (no giant
    decomposition); everything 1 (no key switch at all)"""
    if scheme == "ckks":
        se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    else:
        se = Session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 2
    se.compare(k, count, [1, 1], _giant(n), (scheme, "babies 1"))
    se.compare(k, count, _baby(n), [1, 1, 1], (scheme, "giants 1"))
    se.compare(k, count, [1, 1], [1, 1], (scheme, "all 1"))
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    d, dp = ctx.upload(ct), ctx.upload(rows(se.rng, se.mods, n, (2, 2)))
    out = ctx.alloc(count * 2 * k * n)

    def tags(baby, giant):
        bk, gk = [se.key(g)[1] for g in baby], [se.key(g)[1] for g in giant]
        ev.apply_galois_bsgs_plain(d, k, count, baby, bk, giant, gk, dp, out)
        ctx.profile_enable(True)
        ev.apply_galois_bsgs_plain(d, k, count, baby, bk, giant, gk, dp, out)
        prof = ctx.profile_fetch()
        ctx.profile_enable(False)
        return {t for t in prof if not t.startswith("ntt_")}

    assert tags([1, 1], [1, 1]) == {"hoist_dot_base", "hoist_giant_base"}
    g = _giant(n)[:2]
    babies_one = tags([1, 1], g)
    assert "hoist_dot_mac" not in babies_one and "hoist_giant_mac" in babies_one and "ks_modup" in babies_one, babies_one
    giants_one = tags(g, [1, 1])
    assert "hoist_dot_mac" in giants_one and "hoist_giant_mac" in giants_one, giants_one


@pytest.mark.parametrize("count", [11, 2])
def test_lane_groups(S, count):
    """four ciphertexts per lane of the giant kernel: 11 = 4 + 4 + 3, and a single short group of two"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 41], 1, S.MODE_PARITY)
    se.compare(2, count, _baby(se.n)[:2], _giant(se.n)[1:], ("lanes", count), items=(0, count - 2, count - 1))


def test_launch_counts(S):
    """4 babies x 4 giants, the identity on each axis: with D the transformed rows of one decomposition of the batch and M
    those of one full mod-down (read off apply_galois_many with one and with three elements: D + M and D + 3 M), the call
    transforms exactly D (the input's digits, once) + 3 D (the d_j of the three non-identity giants) + 3 M / 2 (three
    one-component mod-downs) + M (one full mod-down) rows, per transform kernel; the mod-up runs twice (the input, the batch
    of d_j), each new kernel once."""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 2
    baby = [1, 3, 5, 7]
    giant = [1, 9, 11, 13]
    bk, gk = [se.key(g)[1] for g in baby], [se.key(g)[1] for g in giant]
    d = ctx.upload(rows(se.rng, se.mods[:k], n, (count, 2)))
    dp = ctx.upload(rows(se.rng, se.mods, n, (4, 4)))
    out = ctx.alloc(3 * count * 2 * k * n)
    ev.apply_galois_bsgs_plain(d, k, count, baby, bk, giant, gk, dp, out)  # (tables resident)

    def profile(fn):
        ctx.profile_enable(True)
        fn()
        prof = ctx.profile_fetch()
        ctx.profile_enable(False)
        return prof

    def transforms(prof):
        return {tag: v["units"] for tag, v in prof.items() if tag.startswith("ntt_")}

    bsgs = profile(lambda: ev.apply_galois_bsgs_plain(d, k, count, baby, bk, giant, gk, dp, out))
    one = profile(lambda: ev.apply_galois_many(d, k, count, baby[1:2], bk[1:2], out))
    three = profile(lambda: ev.apply_galois_many(d, k, count, baby[1:], bk[1:], out))
    t_b, t_1, t_3 = transforms(bsgs), transforms(one), transforms(three)
    assert set(t_b) == set(t_1) == set(t_3), (bsgs, one, three)
    for tag in t_b:
        m = (t_3[tag] - t_1[tag]) / 2
        dd = t_1[tag] - m
        assert t_b[tag] == 4 * dd + 2.5 * m, (tag, bsgs, one, three)
    assert bsgs["ks_modup"]["launches"] == 2 * one["ks_modup"]["launches"], (bsgs, one)
    for tag in one:
        if tag.startswith("ks_moddown"):
            assert bsgs[tag]["launches"] == 2 * one[tag]["launches"], (tag, bsgs, one)  # one run of three halves, one full
    for tag in ("hoist_dot_mac", "hoist_dot_base", "hoist_giant_mac", "hoist_giant_base"):
        assert bsgs[tag]["launches"] == 1, bsgs
    assert "hoist_mac" not in bsgs and "ks_mac" not in bsgs and "hoist_galois" not in bsgs, bsgs


def test_refusals(S):
    """BFV in PARITY mode; a bad element, a short key and a NULL key for an element other than 1, on either axis; overlap of
    out with ct and with plain_ntt; an empty axis; a missing key by step. Each leaves input and output untouched."""
    logn, n = 12, 1 << 12
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    rng = np.random.default_rng(1)
    k, count = 3, 1
    key = rows(rng, mods, n, (3, 2))
    for scheme, mode, t in ((S.SCHEME_BFV, S.MODE_PARITY, 65537), (S.SCHEME_CKKS, S.MODE_PARITY, 0)):
        ctx = S.Context(scheme, logn, mods, 1, t, mode=mode)
        ev = S.Evaluator(ctx)
        dkey, short = S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, key[:2])
        ct = rows(rng, mods[:k], n, (count, 2))
        plains = rows(rng, mods, n, (2, 2))
        d, dp = ctx.upload(ct), ctx.upload(plains)
        out = ctx.alloc(count * 2 * k * n)
        sentinel = np.full(out.words, 7, dtype=np.uint64)
        out.upload(sentinel)
        good, gkeys = [3, 1], [dkey, None]

        def call(baby=good, bkeys=gkeys, giant=good, gk=gkeys, o=out, src=d):
            ev.apply_galois_bsgs_plain(src, k, count, baby, bkeys, giant, gk, dp, o)

        if scheme == S.SCHEME_BFV:
            with pytest.raises(ValueError, match="STRICT"):
                call()
            with pytest.raises(ValueError, match="STRICT"):
                ev.rotate_vector_bsgs_plain(d, k, count, [1, 0], [0, 1], {H.elt_from_step(n, 1): dkey}, dp, out)
        else:
            for axis in (0, 1):
                def on_axis(elts, keys):
                    return call(baby=elts, bkeys=keys) if axis == 0 else call(giant=elts, gk=keys)

                for bad in (4, 2 * n, 2 * n + 1, 0):
                    with pytest.raises(ValueError, match="Galois element is not valid"):
                        on_axis([3, bad], [dkey, dkey])
                with pytest.raises(ValueError, match="kswitch_keys is not valid"):
                    on_axis([3, 5], [dkey, short])
                with pytest.raises(TypeError):
                    on_axis([1, 5], [dkey, None])
                with pytest.raises(ValueError, match="empty sum"):
                    on_axis([], [])
                steps = ([0, 1], [0, 0]) if axis == 0 else ([0, 0], [0, 1])
                with pytest.raises(ValueError, match="Galois key not present"):
                    ev.rotate_vector_bsgs_plain(d, k, count, steps[0], steps[1], {3: dkey}, dp, out)
            with pytest.raises(ValueError, match="level k out of range"):
                ev.apply_galois_bsgs_plain(d, 4, count, good, gkeys, good, gkeys, dp, out)
            with pytest.raises(ValueError, match="overlap ct"):
                call(o=d)
            with pytest.raises(ValueError, match="overlap ct"):
                call(src=d.ptr + 8 * k * n, o=d)
            with pytest.raises(ValueError, match="overlap plain_ntt"):
                call(o=dp.ptr + 8 * 3 * 4 * n)
            ev.apply_galois_bsgs_plain(d, 2, count, [3, 5], [dkey, short], [5, 1], [short, None], dp, out)  # (two digits do below)
            out.upload(sentinel)
        assert np.array_equal(out.download(), sentinel) and np.array_equal(d.download(ct.shape), ct)
        assert np.array_equal(dp.download(plains.shape), plains)
    host = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0, device=-1)
    with pytest.raises(S.LogicError, match="host-only"):
        S.Evaluator(host).apply_galois_bsgs_plain(d, k, count, [1], [None], [1], [None], dp, out)


def test_transparency_flags(S):
    """one flag per output ciphertext (count of them): a ciphertext with c1 = 0 gives a transparent product and is detected,
    by the storing kernel of the mod-down and by the read pass of the all-identity call; a sink that is too small is refused"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 3
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    ct[1, 1] = 0
    d = ctx.upload(ct)
    e1, e2 = H.elt_from_step(n, 1), H.elt_from_step(n, -2)
    dkeys = [se.key(e1)[1], se.key(e2)[1]]
    dp = ctx.upload(rows(se.rng, se.mods, n, (2, 2)))
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        out = ctx.alloc(count * 2 * k * n)
        for baby, bkeys, giant, gkeys in (([e1, 1], [dkeys[0], None], [1, e2], [None, dkeys[1]]),
                                          ([1, 1], [None, None], [e1, e2], dkeys),
                                          ([1, 1], [None, None], [1, 1], [None, None])):
            flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
            ev.apply_galois_bsgs_plain(d, k, count, baby, bkeys, giant, gkeys, dp, out)
            got = flags.download().view(np.uint32)
            assert (got[:3] != 0).tolist() == [True, False, True] and np.all(got[3:] == 5), (baby, giant, got)
        ev.apply_galois_bsgs_plain(d, k, count, [e1, 1], [dkeys[0], None], [1, e2], [None, dkeys[1]], dp, out)
        with_sink = out.download().copy()
        ctx.transparency_sink(flags, 2)
        with pytest.raises(ValueError, match="sink"):
            ev.apply_galois_bsgs_plain(d, k, count, [e1, 1], [dkeys[0], None], [1, e2], [None, dkeys[1]], dp, out)
    finally:
        ctx.transparency_sink(None, 0)
    ev.apply_galois_bsgs_plain(d, k, count, [e1, 1], [dkeys[0], None], [1, e2], [None, dkeys[1]], dp, out)
    assert np.array_equal(out.download(), with_sink)


def test_graph_capture(S):
    """warm the Galois tables, capture one call, replay it twice on new inputs: the words of the restatement"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 2
    baby, giant = _baby(n)[:3], _giant(n)[1:]
    bk, gk = [se.key(g) for g in baby], [se.key(g) for g in giant]
    d = ctx.upload(rows(se.rng, se.mods[:k], n, (count, 2)))
    dp = ctx.upload(rows(se.rng, se.mods, n, (3, 3)))
    out = ctx.alloc(count * 2 * k * n)
    run = lambda: ev.apply_galois_bsgs_plain(d, k, count, baby, [kk[1] for kk in bk], giant, [kk[1] for kk in gk], dp, out)
    run()
    g = ctx.capture(run)
    for _ in range(2):
        ct = rows(se.rng, se.mods[:k], n, (count, 2))
        plains = rows(se.rng, se.mods, n, (3, 3))
        d.upload(ct)
        dp.upload(plains)
        g.launch()
        got = out.download((count, 2, k, n))
        want = HB.bsgs(se.ref, k, ct, baby, [kk[0] for kk in bk], giant, [kk[0] for kk in gk], plains)
        assert np.array_equal(got, want)


def test_matrix_vector_product_in_one_call(S):
    """BFV STRICT, N = 2^12, t = 65537, real keys: the 16 x 16 matrix-vector product of tests/test_gpu_hoist_dot.py (4 x 4
    diagonals, the vector replicated along the batching rows) through ONE rotate_vector_bsgs_plain. Every slot decrypts to
    M v mod t; the device's words are the restatement's; and the invariant noise budget is at least that of the existing
    composition (rotate_vector_dot_plain, then apply_galois and add per giant step) on the same inputs minus one bit -- an
    inequality checked on the CPU restatement first (tests/noise_ref.py), then on the device's budgets."""
    logn, n, t, dim, bs = 12, 1 << 12, 65537, 16, 4
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    n_key = len(mods)
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT)
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    cl = O.Client(ref, seed=12)
    ev = S.Evaluator(ctx)
    k = cl.k
    rng = np.random.default_rng(12)
    M = rng.integers(0, t, size=(dim, dim), dtype=np.uint64)
    v = rng.integers(0, t, size=dim, dtype=np.uint64)
    # (the slot labelling of tests/test_gpu_hoist_dot.py: a rotation by one step advances the index by one)
    half, e1 = n // 2, H.elt_from_step(n, 1)
    s0 = next(s for s in range(half) if pow(3, s, 2 * n) in (e1, 2 * n - e1))
    slot = ((np.arange(n) % half) * pow(s0, -1, half) % half) % dim

    def encode(values):
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, n)
        plain = ctx.alloc(values.shape[0] * n)
        ctx.batch_encode(ctx.upload(values), n, values.shape[0], plain)
        return plain

    ct_host = cl.encrypt_bfv(encode(v[slot]).download())
    ct = ctx.upload(ct_host)
    diag = np.empty((bs, bs, n), dtype=np.uint64)  # W[g][b] = diagonal 4g + b rotated right by 4g
    for g in range(bs):
        for b in range(bs):
            diag[g, b] = M[(slot - bs * g) % dim, (slot + b) % dim]
    plains = ctx.alloc(bs * bs * n_key * n)
    ev.transform_plain_to_ntt(encode(diag), n, n_key, bs * bs, plains)
    baby_steps, giant_steps = list(range(bs)), [bs * g for g in range(bs)]
    host_keys = {H.elt_from_step(n, st): cl.galois_key(H.elt_from_step(n, st)) for st in baby_steps + giant_steps if st}
    gk = {g: S.KSwitchKeys(ctx, key) for g, key in host_keys.items()}
    fused = ctx.alloc(2 * k * n)
    ev.rotate_vector_bsgs_plain(ct, k, 1, baby_steps, giant_steps, gk, plains, fused)
    # the existing composition on the same inputs
    inner = ctx.alloc(bs * 2 * k * n)
    ev.rotate_vector_dot_plain(ct, k, 1, baby_steps, gk, plains, bs, inner)
    inner_host = inner.download((bs, 2, k, n))
    composed = ctx.upload(inner_host[0])
    for g in range(1, bs):
        term = ctx.upload(inner_host[g])
        ev.apply_galois_inplace(term, k, 1, H.elt_from_step(n, bs * g), gk[H.elt_from_step(n, bs * g)])
        nxt = ctx.alloc(2 * k * n)
        ev.add(composed, 2, term, 2, k, 1, nxt)
        composed = nxt
    want = np.array([sum(int(M[i, j]) * int(v[j]) for j in range(dim)) % t for i in range(dim)], dtype=np.uint64)
    sk = ctx.upload(cl.sk_powers(1))
    for result in (fused, composed):
        plain, values = ctx.alloc(n), ctx.alloc(n)
        ctx.decrypt(result, 2, k, 1, sk, False, plain)
        ctx.batch_decode(plain, 1, values)
        assert np.array_equal(values.download(), want[slot])
    # the restatement: the device's words, and the inequality on the CPU first
    baby = [1 if st == 0 else H.elt_from_step(n, st) for st in baby_steps]
    giant = [1 if st == 0 else H.elt_from_step(n, st) for st in giant_steps]
    plains_host = plains.download((bs, bs, n_key, n))
    args = (ref, k, ct_host, baby, [host_keys.get(g) for g in baby], giant, [host_keys.get(g) for g in giant], plains_host)
    restated, restated_comp = HB.bsgs_one(*args), HB.composed_one(*args)
    assert np.array_equal(fused.download((2, k, n)), restated)

    def cpu_budget(c):
        dot = np.zeros((k, n), dtype=np.uint64)
        O.lib().ref_dot_product_ct_sk(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(c)), 2, 0, O.ptr(cl.sk_powers(1)), O.ptr(dot))
        return NR.ref_noise_budget(dot, mods[:k], t)

    cpu_f, cpu_c = cpu_budget(restated), cpu_budget(restated_comp)
    dev_f = int(ctx.invariant_noise_budget(fused, 2, k, 1, sk)[0])
    dev_c = int(ctx.invariant_noise_budget(composed, 2, k, 1, sk)[0])
    print("matvec noise budgets: restatement fused %d composed %d; device fused %d composed %d" % (cpu_f, cpu_c, dev_f, dev_c))
    assert cpu_f >= cpu_c - 1, (cpu_f, cpu_c)
    assert dev_f == cpu_f and dev_f >= dev_c - 1, (dev_f, dev_c, cpu_f)


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_cpp_adapter(S, tmp_path, scheme):
    """tests/host_adapter_bsgs_check.cpp: the host-ciphertext and the DeviceCiphertext / DevicePlaintext overloads, by elements
    and by steps (rotate_vector_bsgs_plain for CKKS, rotate_rows_bsgs_plain for BFV), give the ABI's words on the same seeded
    inputs, with the operand's level and form and, for CKKS, the product of the scales"""
    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_bsgs_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", scheme, *mods, timeout=120)
    sm = O.SplitMix(0x4017)
    ct = sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n)
    keys = [sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n) for _ in range(3)]
    plains = sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n)
    if scheme == "ckks":
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    else:
        ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, mode=S.MODE_STRICT)
    ev = S.Evaluator(ctx)
    elts = [H.elt_from_step(n, st) for st in (1, -2, 4)]
    dkeys = [S.KSwitchKeys(ctx, key) for key in keys]
    d, dp = ctx.upload(ct), ctx.upload(plains)
    by_elt = ctx.alloc(2 * k * n)
    ev.apply_galois_bsgs_plain(d, k, 1, [elts[0], 1], [dkeys[0], None], [1, elts[1], elts[2]], [None, dkeys[1], dkeys[2]], dp,
                               by_elt)
    by_step = ctx.alloc(2 * k * n)
    ev.rotate_vector_bsgs_plain(d, k, 1, [1, 0], [0, -2, 4], dict(zip(elts, dkeys)), dp, by_step)
    assert np.array_equal(by_elt.download(), by_step.download())
    for name, buf in (("apply_galois_bsgs_plain", by_elt), ("steps", by_step)):
        for side in ("host", "device"):
            line = "%s %s digest %016x meta 1" % (side, name, O.fnv(buf.download()))
            assert line in stdout, (line, stdout)


# ---------------------------------------------------------------- arena chunks (a child process with the smallest arena)
LOGN, N = 13, 1 << 13


def _child():
    """N = 2^13, 8 + 1 primes, k = 8, CKKS, rows of N words = 64 KiB. The arena rule of DESIGN.md section 17: per item once
    w_coeff + w_ext + ACC + temp = (8 + 72 + 18 + 16) rows = 7.125 MiB, and per giant base_j + acc_j + d_j + temp + d_j's
    coeff and digits = (16 + 18 + 8 + 8 + 8 + 72) rows = 8.125 MiB. Two giants: 23.375 MiB per item, 2 items in 64 MiB, so 5
    items go in chunks 2 + 2 + 1. Eight giants: 72.125 MiB for one item, so the giant list is split 7 + 1 (the second pass
    adds into ACC and BASE), and the chunk is a single item."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    mods = O.coeff_modulus_create(N, [50] * 8 + [60])
    ctx = S.Context(S.SCHEME_CKKS, LOGN, mods, 1, 0)
    ref = O.RefContext(2, LOGN, mods, nsp=1)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(64)
    k = 8
    budget = int(ARENA_MB) << 20
    row = N * 8
    base, per_giant = (k + k * (k + 1) + 2 * (k + 1) + 2 * k) * row, (2 * k + 2 * (k + 1) + 3 * k + k * (k + 1)) * row
    made = {}

    def key(g):
        if g != 1 and g not in made:
            host = rows(rng, mods, N, (8, 2))
            made[g] = (host, S.KSwitchKeys(ctx, host))
        return made.get(g, (None, None))

    def run(count, baby, giant, items):
        bk, gk = [key(g) for g in baby], [key(g) for g in giant]
        ct = rows(rng, mods[:k], N, (count, 2))
        plains = rows(rng, mods, N, (len(giant), len(baby)))
        d, dp = ctx.upload(ct), ctx.upload(plains)
        out = ctx.alloc(count * 2 * k * N)
        ctx.chunk_log()
        ev.apply_galois_bsgs_plain(d, k, count, baby, [kk[1] for kk in bk], giant, [kk[1] for kk in gk], dp, out)
        log = ctx.chunk_log()
        got = out.download((count, 2, k, N))
        want = HB.bsgs(ref, k, ct, baby, [kk[0] for kk in bk], giant, [kk[0] for kk in gk], plains, items)
        for c in items:
            assert np.array_equal(got[c], want[c]), (count, len(giant), c)
        return log

    per_chunk = budget // (base + 2 * per_giant)
    assert per_chunk == 2
    log = run(5, [3, 1], [5, 1], (1, 4))
    assert log == [(5, per_chunk)], log                   # ragged item chunks; the giant list whole
    giants = [5, 7, 1, 9, 11, 5, 13, 15]
    assert base + len(giants) * per_giant > budget
    per_pass = (budget - base) // per_giant
    assert per_pass == 7
    log = run(2, [3, 1], giants, (1,))
    assert log == [(len(giants), per_pass), (2, 1)], log  # the giant list split 7 + 1, one item per chunk
    print("HOIST_BSGS_CHUNKS_OK")


def test_chunked_items_and_split_giant_list():
    run_arena_child(__file__, "HOIST_BSGS_CHUNKS_OK", timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
