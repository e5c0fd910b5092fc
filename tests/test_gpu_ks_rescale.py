"""The key switch's mod-down merged with the CKKS rescale on the device (the sealhip_evaluator_*_rescale entries, DESIGN.md
section 19) against the CPU restatement of tests/ks_rescale_ref.py, word for word, no tolerance.

Shapes: the smallest that reach every path of the new finish. [60]*5+[61] at N = 2^10 has primes on which an uncorrected
forward transform could wrap (the finish asks for the exact one in both modes); [50]*7+[51]*3 has three special primes (four
dropped primes: the widest register instance), a short last bundle and the FP64 transforms; nine special primes take the
loop form of the conversion kernel; N = 2^6 is a ring smaller than a workgroup; N = 2^14 takes the single-pass transforms.
Seventeen ciphertexts reach the grouped inner-product kernel and more than one block per row; seventeen terms the second
launch group of the tensor sum."""
import os
import sys

import numpy as np
import pytest

import hoist_ref as H
import ks_rescale_ref as R
import oracle_lib as O
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe, session_memo, top

pytestmark = pytest.mark.gpu


# logn, prime bits, special primes, levels
SETS = {
    "n10_nsp1": (10, [60] * 5 + [61], 1, (5, 4, 3, 2)),
    "n8_nsp3": (8, [50] * 7 + [51] * 3, 3, (7, 4, 3, 2)),
    "n8_nsp9": (8, [50] * 10 + [51] * 9, 9, (10, 2)),
    "n6_nsp1": (6, [50] * 3 + [51], 1, (3, 2)),
    "n14_nsp1": (14, [55] * 3 + [56], 1, (3,)),
}


class Session(BaseSession):
    """contexts on both sides and random keys: the word-for-word comparison needs no valid keys. fill: rows or top."""

    def __init__(self, S, logn, bits, nsp, mode=0, seed=0, top=False):
        super().__init__(S, S.SCHEME_CKKS, logn, bits, nsp, mode, 0, seed + logn + len(bits))
        self.top = top
        self.keys = {}

    def rows(self, mods, lead):
        return top(mods, self.n, lead) if self.top else rows(self.rng, mods, self.n, lead)

    def key(self, g):
        """(host words, device handle) of the key of element g; "relin" names the relinearization key; 1 has none"""
        if g == 1:
            return None, None
        if g not in self.keys:
            host = self.rows(self.mods, (self.nd, 2))
            self.keys[g] = (host, self.S.KSwitchKeys(self.ctx, host))
        return self.keys[g]

    # ---- the four operations: device result against the restatement, inputs unchanged
    def relinearize(self, k, count, tag, items=None, pad=0):
        n = self.n
        ct = self.rows(self.mods[:k], (count, 3))
        stride = 3 * k * n + pad
        buf = np.full((count, stride), 11, dtype=np.uint64)
        buf[:, :3 * k * n] = ct.reshape(count, -1)
        d = self.ctx.upload(buf)
        out = self.ctx.alloc(count * 2 * (k - 1) * n)
        kh, kd = self.key("relin")
        self.ev.relinearize_rescale(d, k, count, [kd], out, item_stride=stride if pad else 0)
        got = out.download((count, 2, k - 1, n))
        assert np.array_equal(d.download(buf.shape), buf), (tag, "the input was modified")
        for c in (range(count) if items is None else items):
            assert np.array_equal(got[c], R.relinearize_rescale(self.ref, k, ct[c], kh)), (tag, "item", c)
        d.free()
        out.free()
        return ct, got

    def dot_product(self, k, count, n_terms, tag, items=None):
        n = self.n
        pool = [self.rows(self.mods[:k], (count, 2)) for _ in range(2 * n_terms)]
        dev = [self.ctx.upload(p) for p in pool]
        out = self.ctx.alloc(count * 2 * (k - 1) * n)
        kh, kd = self.key("relin")
        self.ev.dot_product_rescale(dev[:n_terms], dev[n_terms:], k, count, out, [kd])
        got = out.download((count, 2, k - 1, n))
        for d, p in zip(dev, pool):
            assert np.array_equal(d.download(p.shape), p), (tag, "an operand was modified")
            d.free()
        out.free()
        for c in (range(count) if items is None else items):
            want = R.dot_product_rescale(self.ref, k, [p[c] for p in pool[:n_terms]], [p[c] for p in pool[n_terms:]], kh)
            assert np.array_equal(got[c], want), (tag, "item", c)
        return pool, got

    def dot_plain(self, k, count, elts, n_sums, tag):
        n = self.n
        ct = self.rows(self.mods[:k], (count, 2))
        plains = self.rows(self.mods, (n_sums, len(elts)))
        d, dp = self.ctx.upload(ct), self.ctx.upload(plains)
        out = self.ctx.alloc(n_sums * count * 2 * (k - 1) * n)
        keys = [self.key(g) for g in elts]
        self.ev.apply_galois_dot_plain_rescale(d, k, count, elts, [kk[1] for kk in keys], dp, n_sums, out)
        got = out.download((n_sums, count, 2, k - 1, n))
        assert np.array_equal(d.download(ct.shape), ct) and np.array_equal(dp.download(plains.shape), plains), tag
        want = R.dot_plain_rescale(self.ref, k, ct, elts, [kk[0] for kk in keys], plains)
        assert np.array_equal(got, want), tag
        for b in (d, dp, out):
            b.free()
        return ct, plains, got

    def bsgs(self, k, count, baby, giant, tag):
        n = self.n
        ct = self.rows(self.mods[:k], (count, 2))
        plains = self.rows(self.mods, (len(giant), len(baby)))
        d, dp = self.ctx.upload(ct), self.ctx.upload(plains)
        out = self.ctx.alloc(count * 2 * (k - 1) * n)
        bk, gk = [self.key(g) for g in baby], [self.key(g) for g in giant]
        self.ev.apply_galois_bsgs_plain_rescale(d, k, count, baby, [kk[1] for kk in bk], giant, [kk[1] for kk in gk], dp, out)
        got = out.download((count, 2, k - 1, n))
        assert np.array_equal(d.download(ct.shape), ct) and np.array_equal(dp.download(plains.shape), plains), tag
        want = R.bsgs_plain_rescale(self.ref, k, ct, baby, [kk[0] for kk in bk], giant, [kk[0] for kk in gk], plains)
        assert np.array_equal(got, want), tag
        for b in (d, dp, out):
            b.free()
        return ct, plains, got


_made = session_memo(Session)


def _session(S, name, mode=0):
    logn, bits, nsp, _ = SETS[name]
    return _made(S, logn, bits, nsp, mode)


def _few(se, count):
    """the items compared: all of them on the small rings, the first and the last two above"""
    return None if se.n <= 256 else sorted({0, count - 2, count - 1})


@pytest.mark.parametrize("name", list(SETS))
def test_relinearize_rescale(S, name):
    """three ciphertexts and seventeen at every level; once with ciphertexts further apart than their size"""
    se = _session(S, name)
    levels = SETS[name][3]
    for k in levels:
        se.relinearize(k, 3, (name, k, 3))
        se.relinearize(k, 17, (name, k, 17), items=_few(se, 17))
    se.relinearize(levels[0], 3, (name, "strided"), pad=5 * se.n + 3)


@pytest.mark.parametrize("name", list(SETS))
def test_dot_product_rescale(S, name):
    """one term (multiply + relinearize + rescale), three, and seventeen: the second launch group adds into the first"""
    se = _session(S, name)
    for k in SETS[name][3]:
        for n_terms in (1, 3, 17):
            se.dot_product(k, 2, n_terms, (name, k, n_terms), items=None if se.n <= 1024 else (1,))


@pytest.mark.parametrize("name", list(SETS))
def test_dot_plain_rescale(S, name):
    """two sums over [g, 1, g']; and identity elements only: no key-switch term, the plain rescale of base"""
    se = _session(S, name)
    n = se.n
    elts = [H.elt_from_step(n, 1), 1, H.elt_from_step(n, -3)]
    for k in SETS[name][3]:
        se.dot_plain(k, 2, elts, 2, (name, k))
    se.dot_plain(SETS[name][3][0], 2, [1, 1], 2, (name, "identity"))


@pytest.mark.parametrize("name", list(SETS))
def test_bsgs_plain_rescale(S, name):
    """2 x 2 steps with step 0 on both axes; the all-identity call is the plain rescale of BASE"""
    se = _session(S, name)
    n = se.n
    baby, giant = [1, H.elt_from_step(n, 1)], [H.elt_from_step(n, 2), 1]
    for k in SETS[name][3]:
        se.bsgs(k, 2, baby, giant, (name, k))
    se.bsgs(SETS[name][3][0], 2, [1, 1], [1, 1], (name, "identity"))


@pytest.mark.parametrize("nsp", [1, 2])
def test_extreme_operands(S, nsp):
    """61-bit primes only and every ciphertext, key and plaintext word p - 1: the largest residues every sum can see"""
    se = Session(S, 6, [61] * 6, nsp, top=True)
    n = se.n
    for k in (se.k_first, 2):
        se.relinearize(k, 2, ("top", nsp, k))
        se.dot_product(k, 2, 3, ("top", nsp, k))
        se.dot_plain(k, 2, [H.elt_from_step(n, 1), 1, 3], 2, ("top", nsp, k))
        se.bsgs(k, 2, [1, 3], [5, 1], ("top", nsp, k))


def test_strict_context(S):
    """a STRICT context beside PARITY: the finish is the same function of base and acc; acc is the mode's"""
    se = _session(S, "n10_nsp1", mode=S.MODE_STRICT)
    n = se.n
    for k in (5, 2):
        se.relinearize(k, 3, ("strict", k))
        se.dot_product(k, 2, 3, ("strict", k))
        se.dot_plain(k, 2, [H.elt_from_step(n, 1), 1, 3], 2, ("strict", k))
        se.bsgs(k, 2, [1, 3], [5, 1], ("strict", k))


def test_transparency_flags(S):
    """one flag per output ciphertext, in output order, written by the storing kernel (and by the read pass of the
    all-identity calls): a ciphertext whose c_1 and c_2 are zero gives a transparent result; a sink that is too small is
    refused"""
    se = _session(S, "n8_nsp3")
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 4, 3
    kd = se.key("relin")[1]
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        def check(expect, tag):
            got = flags.download().view(np.uint32)
            assert (got[:len(expect)] != 0).tolist() == expect and np.all(got[len(expect):] == 5), (tag, got)

        def arm():
            flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))

        ct3 = rows(se.rng, se.mods[:k], n, (count, 3))
        ct3[1, 1:] = 0
        d3 = ctx.upload(ct3)
        out = ctx.alloc(2 * count * 2 * (k - 1) * n)
        arm()
        ev.relinearize_rescale(d3, k, count, [kd], out)
        check([True, False, True], "relinearize")
        ct = rows(se.rng, se.mods[:k], n, (count, 2))
        ct[1, 1] = 0
        d = ctx.upload(ct)
        g = H.elt_from_step(n, 1)
        gk = se.key(g)[1]
        dp = ctx.upload(rows(se.rng, se.mods, n, (2, 2)))
        for elts, keys in (([g, 1], [gk, None]), ([1, 1], [None, None])):
            arm()
            ev.apply_galois_dot_plain_rescale(d, k, count, elts, keys, dp, 2, out)
            check([True, False, True] * 2, ("dot_plain", elts))
            arm()
            ev.apply_galois_bsgs_plain_rescale(d, k, count, elts, keys, elts[::-1], keys[::-1], dp, out)
            check([True, False, True], ("bsgs", elts))
        ctx.transparency_sink(flags, 2)
        with pytest.raises(ValueError, match="sink is smaller"):
            ev.relinearize_rescale(d3, k, count, [kd], out)
    finally:
        ctx.transparency_sink(None, 0)


def test_graph_capture(S):
    """relinearize_rescale captured after a warm-up call and replayed on new inputs"""
    se = _session(S, "n10_nsp1")
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 4, 2
    kh, kd = se.key("relin")
    d = ctx.upload(rows(se.rng, se.mods[:k], n, (count, 3)))
    out = ctx.alloc(count * 2 * (k - 1) * n)
    run = lambda: ev.relinearize_rescale(d, k, count, [kd], out)
    run()
    g = ctx.capture(run)
    for _ in range(2):
        ct = rows(se.rng, se.mods[:k], n, (count, 3))
        d.upload(ct)
        g.launch()
        got = out.download((count, 2, k - 1, n)).copy()
        out.upload(np.zeros(count * 2 * (k - 1) * n, dtype=np.uint64))
        run()
        assert np.array_equal(out.download((count, 2, k - 1, n)), got)
        for c in range(count):
            assert np.array_equal(got[c], R.relinearize_rescale(se.ref, k, ct[c], kh)), c


def test_refusals(S):
    """with a device: a key with fewer digits than the level, overlap of out with an input, the last level, a level above the
    first; each leaves input and output untouched. (The checks that need no key run in tests/test_ks_rescale_host.py.)"""
    se = _session(S, "n8_nsp3")
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 7, 2
    kd = se.key("relin")[1]
    short = S.KSwitchKeys(ctx, rows(se.rng, se.mods, n, (2, 2)))
    ct3 = rows(se.rng, se.mods[:k], n, (count, 3))
    d = ctx.upload(ct3)
    out = ctx.alloc(count * 2 * (k - 1) * n)
    sentinel = np.full(out.words, 7, dtype=np.uint64)
    out.upload(sentinel)
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        ev.relinearize_rescale(d, k, count, [short], out)
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        ev.dot_product_rescale([d], [d], k, count, out, [short])
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        ev.relinearize_rescale(d, k, count, [], out)
    with pytest.raises(ValueError, match="overlap"):
        ev.relinearize_rescale(d, k, count, [kd], d.ptr + 8 * (count * 3 * k * n - 1))
    with pytest.raises(ValueError, match="overlap"):
        ev.dot_product_rescale([d], [out], k, count, out, [kd])
    with pytest.raises(ValueError, match="end of modulus switching chain"):
        ev.relinearize_rescale(d, 1, count, [kd], out)
    with pytest.raises(ValueError, match="level k out of range"):
        ev.relinearize_rescale(d, 8, count, [kd], out)
    ev.relinearize_rescale(d, 6, count, [short], out)  # (two digits do at level 6)
    out.upload(sentinel)
    assert np.array_equal(out.download(), sentinel) and np.array_equal(d.download(ct3.shape), ct3)


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_ks_rescale_check.cpp in device mode: the host-ciphertext and the DeviceCiphertext forms of every
    adapter method give the ABI's words on the same seeded inputs, one level down, with the scale divided by q_{k-1}"""
    logn, n, k = 8, 1 << 8, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_ks_rescale_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    sm = O.SplitMix(0x4019)
    a, b = (sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n) for _ in range(2))
    ct3 = sm.fill(3 * k, n, mods[:k] * 3).reshape(1, 3, k, n)
    nd = k
    relin = S.KSwitchKeys(ctx, sm.fill(nd * 2 * len(mods), n, mods * (2 * nd)).reshape(nd, 2, len(mods), n))
    g1, g2 = H.elt_from_step(n, 1), H.elt_from_step(n, 2)
    gk = {g: S.KSwitchKeys(ctx, sm.fill(nd * 2 * len(mods), n, mods * (2 * nd)).reshape(nd, 2, len(mods), n)) for g in (g1, g2)}
    plains = sm.fill(4 * len(mods), n, mods * 4).reshape(2, 2, len(mods), n)
    da, db, d3, dp = ctx.upload(a), ctx.upload(b), ctx.upload(ct3), ctx.upload(plains)
    words = 2 * (k - 1) * n
    out = ctx.alloc(2 * words)
    results = {}
    ev.relinearize_rescale(d3, k, 1, [relin], out)
    results["relinearize"] = out.download()[:words].copy()
    ev.dot_product_rescale([da], [db], k, 1, out, [relin])
    results["dot_product"] = out.download()[:words].copy()
    ev.apply_galois_dot_plain_rescale(da, k, 1, [g1, 1], [gk[g1], None], dp, 2, out)
    results["dot_plain"] = out.download().copy()
    ev.apply_galois_bsgs_plain_rescale(da, k, 1, [g1, 1], [gk[g1], None], [1, g2], [None, gk[g2]], dp, out)
    results["bsgs"] = out.download()[:words].copy()
    for name, words_ in results.items():
        for side in ("host", "device"):
            line = "%s %s digest %016x meta 1" % (side, name, O.fnv(words_))
            assert line in stdout, (line, stdout)


# ---------------------------------------------------------------- arena chunks (a child process with the smallest arena)
LOGN, N = 13, 1 << 13


def _child():
    """N = 2^13, 8 + 1 primes, k = 8, CKKS, rows of N words = 64 KiB: the merged-rescale forms of the weighted sums under the
    arena rule of DESIGN.md section 19. base_s and BASE live at the front of the arena; the temporaries are 2 (k - 1) rows.

    dot_plain: per item once the digits, (8 + 72) rows = 5 MiB; per sum products + temporaries + base_s = (18 + 14 + 16) rows
    = 3 MiB. Two sums: 11 MiB per item, 5 items in 64 MiB, so 7 items go 5 + 2. Twenty sums: 65 MiB for one item, so the
    sum list is split 19 + 1 and the chunk is a single item.
    bsgs: per item once digits + ACC + temporaries + BASE = (8 + 72 + 18 + 14 + 16) rows = 8 MiB, per giant 8.125 MiB (as
    without rescale). Two giants: 24.25 MiB per item, 2 items per chunk, so 3 items go 2 + 1. Seven giants: 64.875 MiB for
    one item, so the giant list is split 6 + 1.
    Identity elements only: no key-switch term, and the finish is rescale_to_next of base_s / BASE -- a nested chunk loop
    over 2 m polynomials of (1 + 7) rows under a floor raised over them, for which every item carries 16 more rows. Two
    sums or giants: 4 MiB per item, 16 items per chunk, so 17 items need a second chunk; the nested loops log their pairs."""
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
    digits, prod, temp, base2 = (k + k * (k + 1)) * row, 2 * (k + 1) * row, 2 * (k - 1) * row, 2 * k * row
    nested = budget // ((1 + k - 1) * row)  # polynomials per chunk of the plain rescale
    made = {}

    def key(g):
        if g != 1 and g not in made:
            host = rows(rng, mods, N, (8, 2))
            made[g] = (host, S.KSwitchKeys(ctx, host))
        return made.get(g, (None, None))

    def dot_plain(count, elts, n_sums, items, sums):
        keys = [key(g) for g in elts]
        ct = rows(rng, mods[:k], N, (count, 2))
        plains = rows(rng, mods, N, (n_sums, len(elts)))
        d, dp = ctx.upload(ct), ctx.upload(plains)
        out = ctx.alloc(n_sums * count * 2 * (k - 1) * N)
        ctx.chunk_log()
        ev.apply_galois_dot_plain_rescale(d, k, count, elts, [kk[1] for kk in keys], dp, n_sums, out)
        log = ctx.chunk_log()
        got = out.download((n_sums, count, 2, k - 1, N))
        want = R.dot_plain_rescale(ref, k, ct[list(items)], elts, [kk[0] for kk in keys], plains[list(sums)])
        for j, s in enumerate(sums):
            for i, c in enumerate(items):
                assert np.array_equal(got[s, c], want[j, i]), ("dot_plain", elts, n_sums, s, c)
        for b in (d, dp, out):
            b.free()
        return log

    def bsgs(count, baby, giant, items):
        bk, gk = [key(g) for g in baby], [key(g) for g in giant]
        ct = rows(rng, mods[:k], N, (count, 2))
        plains = rows(rng, mods, N, (len(giant), len(baby)))
        d, dp = ctx.upload(ct), ctx.upload(plains)
        out = ctx.alloc(count * 2 * (k - 1) * N)
        ctx.chunk_log()
        ev.apply_galois_bsgs_plain_rescale(d, k, count, baby, [kk[1] for kk in bk], giant, [kk[1] for kk in gk], dp, out)
        log = ctx.chunk_log()
        got = out.download((count, 2, k - 1, N))
        want = R.bsgs_plain_rescale(ref, k, ct[list(items)], baby, [kk[0] for kk in bk], giant, [kk[0] for kk in gk], plains)
        for i, c in enumerate(items):
            assert np.array_equal(got[c], want[i]), ("bsgs", baby, giant, c)
        for b in (d, dp, out):
            b.free()
        return log

    # ---- apply_galois_dot_plain_rescale
    once, per_sum = digits, prod + temp + base2
    per_chunk = budget // (once + 2 * per_sum)
    assert per_chunk == 5
    log = dot_plain(7, [3, 1, 5], 2, (0, 6), (0, 1))
    assert log == [(7, per_chunk)], log                   # a second, ragged item chunk; the sum list whole
    n_sums = 20
    assert once + n_sums * per_sum > budget
    per_pass = (budget - once) // per_sum
    assert per_pass == n_sums - 1
    log = dot_plain(2, [3], n_sums, (0, 1), (0, n_sums - 1))
    assert log == [(n_sums, per_pass), (2, 1)], log       # the sum list split 19 + 1, one item per chunk
    per_chunk = budget // (2 * (base2 + base2))
    assert per_chunk == 16 and 2 * per_chunk <= nested
    log = dot_plain(17, [1, 1], 2, (0, 16), (0, 1))
    # one plain rescale per sum and chunk (a chunk is not the whole batch), each over the 2 m polynomials of its m items
    assert log == [(17, per_chunk)] + [(32, 32)] * 2 + [(2, 2)] * 2, log

    # ---- apply_galois_bsgs_plain_rescale
    once, per_giant = digits + prod + temp + base2, (2 * k + 2 * (k + 1) + 3 * k + k * (k + 1)) * row
    per_chunk = budget // (once + 2 * per_giant)
    assert per_chunk == 2
    log = bsgs(3, [3, 1], [5, 1], (0, 2))
    assert log == [(3, per_chunk)], log                   # a second, ragged item chunk; the giant list whole
    giants = [5, 7, 1, 9, 11, 5, 13]
    assert once + len(giants) * per_giant > budget
    per_pass = (budget - once) // per_giant
    assert per_pass == len(giants) - 1
    log = bsgs(2, [3, 1], giants, (0, 1))
    assert log == [(len(giants), per_pass), (2, 1)], log  # the giant list split 6 + 1, one item per chunk
    per_chunk = budget // (base2 + base2 + 2 * base2)
    assert per_chunk == 16
    log = bsgs(17, [1, 1], [1, 1], (0, 16))
    assert log == [(17, per_chunk), (32, 32), (2, 2)], log  # one plain rescale of BASE per chunk
    print("KS_RESCALE_CHUNKS_OK")


def test_chunked_items_and_split_lists():
    """apply_galois_dot_plain_rescale and apply_galois_bsgs_plain_rescale under the smallest arena: ragged item chunks, a
    sum / giant list one longer than what fits next to one item, and the identity-only calls, whose plain rescale nests a
    chunk loop under the raised floor. Chunk logs against the rule; first and last item (and sum) against the restatement."""
    run_arena_child(__file__, "KS_RESCALE_CHUNKS_OK", timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
