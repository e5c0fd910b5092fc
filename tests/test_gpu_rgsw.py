"""RGSW ciphertexts on the device (sealhip_generate_rgsw, sealhip_rgsw_*, sealhip_evaluator_external_product / _cmux /
_select) against the restatement of tests/rgsw_ref.py and against the composition from the entries
that existed before (rgsw_export, two switch_key_partial, an add, switch_key_finish with two partials), word for word.

Shapes: the smallest that reach every path. Rings of 2^3 and 2^4 (less than a workgroup per row: the loop kernel at every
batch), 2^8 and 2^9 (the first rings with the items family) and 2^12 (several workgroups per row); batches of 1, 15, 16, 17
and 33 (the items threshold and a ragged last group); the first level and level 1; one, two and three special primes with a
short last digit; nine digits (2 nd = 18: no instance); seven digits at levels 7 and 6 (2 nd = 14 and 12, the two instances
no other chain reaches); six 61-bit primes (2 nd = 10 terms do not fit 128 bits: the sum is
reduced between its halves, in both kernels); the 61/20/45/61 chain; CKKS in both modes and BFV in STRICT. Word comparisons
need no valid keys: the RGSW block is two random keys. The semantic runs use keys the library generated.
COMPARED lists every (chain, log N, level, batch) that `compare` is given; tests/test_rgsw_host.py evaluates the selector's rule
over it and asserts, without a device, that the runs reach every instance of the items family and the loop kernel for each of
its reasons."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import rgsw_ref as G
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe, session_memo, top
from test_rgsw_host import select_ext_mac, sum_is_split

pytestmark = pytest.mark.gpu
SENTINEL = 0x5E5E5E5E5E5E5E5E
CASES_16 = {"bfv": (1, [30, 35, 40, 45, 50], 1, 65537), "ckks": (2, [40] * 5 + [41] * 2, 2, 0)}
# name: (scheme, bit sizes, nsp, t, mode)   mode 1 = STRICT, 0 = PARITY
CHAINS = {
    "ckks nsp1": (2, [40, 40, 40, 41], 1, 0, 1),
    "ckks parity": (2, [40, 40, 40, 41], 1, 0, 0),
    "bfv nsp2": (1, [30, 35, 40, 45, 50, 55, 60], 2, 65537, 1),  # five ciphertext primes: digits of 2, 2 and 1
    "ckks nsp3": (2, [40] * 4 + [41] * 3, 3, 0, 1),               # four: digits of 3 and 1
    "nd9": (2, [30] * 9 + [31], 1, 0, 1),                        # 2 nd = 18: the loop kernel at every batch
    "nd7": (2, [40] * 7 + [41], 1, 0, 1),                        # 2 nd = 14, and 12 one level down
    "61": (2, [61] * 6, 1, 0, 1),                                # nd = 5: ten terms of 61-bit primes, the split sum
    "bfv 61": (1, [61] * 6, 1, 65537, 1),
    "mixed": (2, [61, 20, 45, 61], 1, 0, 1),
}


def first_level(chain):
    return len(CHAINS[chain][1]) - CHAINS[chain][2]


THRESHOLD_CHAINS = ("ckks nsp1", "ckks parity", "bfv nsp2", "ckks nsp3", "mixed")
SEVEN_DIGITS = (("nd7", 8, 7, 17), ("nd7", 8, 6, 17), ("nd7", 8, 7, 1))  # ND2 = 14, ND2 = 12, the loop kernel below 16 items
# every (chain, log N, level, batch) a test below hands to Session.compare (which refuses anything else)
COMPARED = set(SEVEN_DIGITS)
for _chain in ("ckks nsp1", "bfv nsp2", "ckks nsp3"):
    for _logn in (3, 4):
        COMPARED |= {(_chain, _logn, first_level(_chain), 1), (_chain, _logn, first_level(_chain), 17), (_chain, _logn, 1, 3)}
for _chain in THRESHOLD_CHAINS:
    for _logn in (8, 9):
        COMPARED |= {(_chain, _logn, first_level(_chain), _count) for _count in (1, 15, 16, 17, 33)} | {(_chain, _logn, 1, 17)}
for _chain in ("ckks nsp1", "bfv nsp2"):
    COMPARED |= {(_chain, 12, first_level(_chain), 1), (_chain, 12, first_level(_chain), 33), (_chain, 12, 1, 16)}
COMPARED |= {("nd9", 8, 9, 1), ("nd9", 8, 9, 17), ("nd9", 8, 8, 17)}
for _chain in ("61", "bfv 61"):
    COMPARED |= {(_chain, 8, 5, 1), (_chain, 8, 5, 17), (_chain, 8, 4, 17)}
COMPARED |= {(_chain, 8, first_level(_chain), 17) for _chain in ("ckks nsp1", "bfv nsp2", "mixed")}


class Session(BaseSession):
    """contexts on both sides and an RGSW block of two random keys (host arrays, device handles and the object)"""

    def __init__(self, S, chain, logn, seed=0):
        scheme, bits, nsp, t, mode = CHAINS[chain]
        super().__init__(S, scheme, logn, bits, nsp, mode, t, 290 + seed + logn)
        self.chain, self.kf = chain, self.k_first
        self.keys = tuple(rows(self.rng, self.mods, self.n, (self.nd, 2)) for _ in range(2))
        self.dkeys = tuple(S.KSwitchKeys(self.ctx, key) for key in self.keys)
        self.g = self.ctx.rgsw_create(*self.dkeys)

    def plan(self, k, count):
        """the device's plan for the batch, held to the rule restated in tests/test_rgsw_host.py"""
        got = self.ctx.debug_ext_mac_plan(k, count)
        nd = -(-k // self.nsp)
        want = select_ext_mac(self.logn, nd, k + self.nsp, count)
        assert (got["family"], got["nd2"], got["group"]) == want[:3], (self.chain, k, count, got, want)
        assert got["split"] == sum_is_split(nd, max(self.mods[:k] + self.mods[self.kf:])), (self.chain, k, count, got)
        return got

    def run(self, fn, inputs, count, k, flags_for=None):
        """fn(device inputs..., out) with sentinels behind out; the inputs must come back as they were; returns the words
        and, with flags_for, the transparency flags of the `flags_for` outputs"""
        words = count * 2 * k * self.n
        out = self.ctx.alloc(words + 4)
        out.upload(np.full(words + 4, SENTINEL, dtype=np.uint64))
        dev = [None if x is None else self.ctx.upload(x) for x in inputs]
        seen = None
        if flags_for is not None:
            flags = self.ctx.alloc((flags_for + 3) // 2 + 1)
            flags.upload(np.full(flags.words, 0x0000000500000005, dtype=np.uint64))
            self.ctx.transparency_sink(flags, flags_for)
        try:
            fn(*dev, out)
        finally:
            if flags_for is not None:
                self.ctx.transparency_sink(None, 0)
        got = out.download()
        assert np.all(got[words:] == SENTINEL), "words behind out were written"
        for x, d in zip(inputs, dev):
            assert x is None or np.array_equal(d.download(x.shape), x), "an input was modified"
        if flags_for is not None:
            seen = flags.download().view(np.uint32)
            assert np.all(seen[flags_for:] == 5), "flags behind the batch were written"
            seen = seen[:flags_for] != 0
        return got[:words].reshape(count, 2, k, self.n), seen

    def external_product(self, ct, k, base=None, flags=False):
        count = ct.shape[0]
        return self.run(lambda c, b, o: self.ev.external_product(c, k, count, self.g, o, base=b), (ct, base), count, k,
                        count if flags else None)

    def composition(self, ct, k, base=None):
        """the entries that existed before: two partials, their word-wise sum, the finish into a copy of base"""
        count, ctx = ct.shape[0], self.ctx
        nd = -(-k // self.nsp)
        pw = count * 2 * (k + self.nsp) * self.n
        parts = []
        for comp in range(2):
            p = ctx.alloc(pw)
            ctx.switch_key_partial(k, ctx.upload(np.ascontiguousarray(ct[:, comp])), count, self.dkeys[comp], 0, nd, p)
            parts.append(p.download())
        acc = ctx.upload(np.zeros((count, 2, k, self.n), dtype=np.uint64) if base is None else base)
        ctx.switch_key_finish(k, acc, ctx.upload(parts[0] + parts[1]), count, 2)
        return acc.download((count, 2, k, self.n))

    def compare(self, k, count, with_base=True, ct=None, tag=""):
        assert (self.chain, self.logn, k, count) in COMPARED, "a comparison the host test's table does not list"
        self.plan(k, count)
        if ct is None:
            ct = rows(self.rng, self.mods[:k], self.n, (count, 2))
        base = rows(self.rng, self.mods[:k], self.n, (count, 2)) if with_base else None
        got, _ = self.external_product(ct, k, base)
        where = (self.chain, "N", self.n, "k", k, "count", count, "base", with_base, tag)
        assert np.array_equal(got, self.composition(ct, k, base)), where + ("device composition",)
        for c in sorted({0, count // 2, count - 1}):  # (the restatement on the first, a middle and the last item)
            want = G.external_product(self.ref, k, ct[c], self.keys, None if base is None else base[c])
            assert np.array_equal(got[c], want), where + ("restatement, item", c)
        return got


session = session_memo(Session)


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("case", [(2, 4, [30, 35, 40, 45, 50], 1), (1, 4, [30, 35, 40, 45, 50, 55, 60], 2),
                                  (2, 12, [40, 40, 45, 50, 50, 60, 60], 2), (1, 8, [36, 36, 37, 40, 60, 60, 60], 3)],
                         ids=lambda c: "s%d-logn%d-k%d-nsp%d" % (c[0], c[1], len(c[2]), c[3]))
def test_generate_rgsw_word_for_word(S, case):
    """every word equals what sealhip_generate_switching_keys gives for sk_from = {NTT(m), NTT(m) (.) sk} with the same samples,
    and what generate_one_kswitch_key restated from oracle entries gives (tests/test_gpu_keygen.py's Setup.expected); the full
    level and level 1; rgsw_create(rgsw_export(x)) is x"""
    from test_gpu_keygen import Setup, wire

    scheme, logn, bits, nsp = case
    st = Setup(S, scheme, logn, bits, nsp)
    W, ctx, n = wire(), st.ctx, st.n
    n_msg = 2
    ms = np.stack([np.random.default_rng(logn).integers(-1, 2, size=n), G.monomial(n, 3, -1)]).astype(np.int32)
    m_ntt = [G.small_to_ntt(st.ref, m) for m in ms]
    s_from = np.stack([half for x in m_ntt for half in (x, G.times_secret(st.ref, x, st.cl.sk))])
    seeds, noise = st.samples(2 * n_msg)  # (n x 2 x d x ..: half h of message i is sample 2 i + h)
    dm, dn = ctx.upload_i32(ms), ctx.upload_i32(noise)
    full = [st.expected(s_from[i], seeds[i], noise[i]) for i in range(2 * n_msg)]
    for level in (st.k, 1):
        kept = (level + nsp - 1) // nsp
        exp = [key.copy() for key in full]
        if level < st.k:
            for key in exp:
                key[:, :, level:st.k] = 0
                key[kept:] = 0
        made = ctx.generate_rgsw(st.sk, dm, n_msg, level, seeds, dn)
        keys = ctx.generate_switching_keys(st.sk, ctx.upload(s_from), 2 * n_msg, level, seeds, dn)
        assert np.array_equal(dm.download().view(np.int32), ms.reshape(-1)) and np.array_equal(dn.download().view(np.int32), noise.reshape(-1))
        for i, g in enumerate(made):
            halves = ctx.rgsw_export(g)
            stream = S.save_kswitch_keys(ctx, list(halves))
            assert stream == S.save_kswitch_keys(ctx, keys[2 * i:2 * i + 2]), (case, level, i, "generate_switching_keys")
            assert stream == st.stream(W, exp[2 * i:2 * i + 2]), (case, level, i, "oracle")
            again = ctx.rgsw_create(*halves)
            assert S.save_kswitch_keys(ctx, list(ctx.rgsw_export(again))) == stream, (case, level, i, "create(export)")
    assert ctx.generate_rgsw(st.sk, None, 0, st.k, seeds[:0], None) == []


# ---------------------------------------------------------------- the external product
@pytest.mark.parametrize("chain", ["ckks nsp1", "bfv nsp2", "ckks nsp3"])
@pytest.mark.parametrize("logn", [3, 4])
def test_external_product_small_rings(S, chain, logn):
    """less than one workgroup per row: the loop kernel at every batch; both levels, with and without a base"""
    s = session(S, chain, logn)
    for count in (1, 17):
        assert s.plan(s.kf, count)["family"] == "loop"
        s.compare(s.kf, count)
    s.compare(1, 3, with_base=False)


@pytest.mark.parametrize("chain", THRESHOLD_CHAINS)
@pytest.mark.parametrize("logn", [8, 9])
def test_external_product_items_threshold(S, chain, logn):
    """either side of 16 items and the group edges, on the first rings with one workgroup (2^8) and two (2^9) per row"""
    s = session(S, chain, logn)
    for count in (1, 15, 16, 17, 33):
        assert s.plan(s.kf, count)["family"] == ("items" if count >= 16 else "loop")
        s.compare(s.kf, count, with_base=count != 16)
    s.compare(1, 17)


@pytest.mark.parametrize("chain", ["ckks nsp1", "bfv nsp2"])
def test_external_product_log12(S, chain):
    s = session(S, chain, 12)
    s.compare(s.kf, 1)
    s.compare(s.kf, 33)
    s.compare(1, 16, with_base=False)


def test_external_product_nine_digits(S):
    """2 nd = 18 has no instance: the loop kernel also at 17 items"""
    s = session(S, "nd9", 8)
    for count in (1, 17):
        plan = s.plan(s.kf, count)
        assert plan["family"] == "loop" and not plan["split"]
        s.compare(s.kf, count)
    assert s.plan(8, 17)["family"] == "items" and s.plan(8, 17)["nd2"] == 16  # (one level down the family's last instance)
    s.compare(8, 17)


def test_external_product_seven_digits(S):
    """seven ciphertext primes and one special prime: ext_mac_items_kernel<14> at the first level and <12> one below, the two
    instances between the five-digit chains and nd9's level 8; one item at the first level takes the loop kernel with the
    same fourteen terms"""
    for chain, logn, k, count in SEVEN_DIGITS:
        s = session(S, chain, logn)
        plan = s.plan(k, count)
        assert (plan["family"], plan["nd2"]) == (("items", 2 * k) if count >= 16 else ("loop", 0)) and not plan["split"]
        s.compare(k, count)


@pytest.mark.parametrize("chain", ["61", "bfv 61"])
def test_external_product_split_sum(S, chain):
    """five digits of 61-bit primes: ten terms do not fit 128 bits (bounds::ext_mac_sum_fits), the launcher says so and both
    kernels reduce between the halves; at level 4 (eight terms) the sum is whole again. Worst words: every target p - 1."""
    s = session(S, chain, 8)
    for count in (1, 17):
        plan = s.plan(s.kf, count)
        assert plan["split"] and plan["family"] == ("items" if count >= 16 else "loop")
        s.compare(s.kf, count)
        s.compare(s.kf, count, ct=top(s.mods[:s.kf], s.n, (count, 2)), tag="all p - 1")
    assert not s.plan(4, 17)["split"]
    s.compare(4, 17, ct=top(s.mods[:4], s.n, (17, 2)), tag="all p - 1")


@pytest.mark.parametrize("chain", ["ckks nsp1", "bfv nsp2", "mixed"])
def test_external_product_extreme_targets_and_flags(S, chain):
    """targets of all p - 1 and all 0; all 0 without a base gives all-zero results, which the flags report as transparent;
    one item with a non-zero base alone is not"""
    s = session(S, chain, 8)
    k, count = s.kf, 17
    s.compare(k, count, ct=top(s.mods[:k], s.n, (count, 2)), tag="all p - 1")
    zero = np.zeros((count, 2, k, s.n), dtype=np.uint64)
    got, flags = s.external_product(zero, k, None, flags=True)
    assert not got.any() and not flags.any()
    base = zero.copy()
    base[5] = rows(s.rng, s.mods[:k], s.n, (2,))
    got, flags = s.external_product(zero, k, base, flags=True)
    assert np.array_equal(got, base) and flags.tolist() == [i == 5 for i in range(count)]
    got, flags = s.external_product(rows(s.rng, s.mods[:k], s.n, (count, 2)), k, None, flags=True)
    assert flags.all()


# ---------------------------------------------------------------- CMux
def planted_pair(s, k, count):
    """two random batches with 0, 1 and p - 1 planted so that all nine pairs of them -- every borrow side of ct1 - ct0 --
    occur at an even and at an odd coefficient (both lanes of a 16-byte access) of every row"""
    a, b = (rows(s.rng, s.mods[:k], s.n, (count, 2)) for _ in range(2))
    for r in range(k):
        vals = (0, 1, s.mods[r] - 1)
        for i in range(min(18, s.n)):
            a[..., r, i], b[..., r, i] = vals[(i % 9) // 3], vals[(i % 9) % 3]
    return a, b


@pytest.mark.parametrize("chain,logn", [("ckks nsp1", 3), ("bfv nsp2", 4), ("ckks nsp1", 8), ("bfv nsp2", 8), ("ckks parity", 9),
                                        ("61", 8), ("ckks nsp3", 12)])
def test_cmux_words(S, chain, logn):
    """the words of external_product(sub(ct1, ct0), base = ct0), on the device and in the restatement"""
    s = session(S, chain, logn)
    for k, count in ((s.kf, 17), (s.kf, 2), (1, 3)):
        ct0, ct1 = planted_pair(s, k, count)
        got, flags = s.run(lambda a, b, o: s.ev.cmux(a, b, k, count, s.g, o), (ct0, ct1), count, k, flags_for=count)
        assert flags.all()
        diff = s.ctx.alloc(ct0.size)
        s.ev.sub(s.ctx.upload(ct1), 2, s.ctx.upload(ct0), 2, k, count, diff)
        host_diff = G.sub(s.mods, k, ct1, ct0)
        assert np.array_equal(diff.download(ct0.shape), host_diff)
        want, _ = s.external_product(host_diff, k, ct0)
        assert np.array_equal(got, want), (chain, logn, k, count, "device")
        for c in (0, count - 1):
            assert np.array_equal(got[c], G.cmux(s.ref, s.mods, k, ct0[c], ct1[c], s.keys)), (chain, logn, k, count, c)


# ---------------------------------------------------------------- select
class Tree:
    """a session with three more RGSW blocks of random keys: a tree's bits"""

    def __init__(self, S, chain, logn, levels, seed=7):
        self.s = s = Session(S, chain, logn, seed=seed)
        self.bit_keys = [s.keys] + [tuple(rows(s.rng, s.mods, s.n, (s.nd, 2)) for _ in range(2)) for _ in range(levels - 1)]
        self.handles = [tuple(S.KSwitchKeys(s.ctx, key) for key in pair) for pair in self.bit_keys[1:]]
        self.bits = [s.g] + [s.ctx.rgsw_create(*pair) for pair in self.handles]

    def select(self, cts, k, l, flags=False):
        s, count = self.s, cts.shape[0]
        return s.run(lambda c, o: s.ev.select(c, k, count, self.bits[:l], o), (cts,), count, k, count if flags else None)


@pytest.mark.parametrize("chain,logn", [("ckks nsp1", 4), ("bfv nsp2", 8), ("ckks nsp3", 9)])
def test_select_words(S, chain, logn):
    """l = 0, 1 and 3 with two items, against the restatement's tree; the flags come from the last level (or the copy)"""
    t = Tree(S, chain, logn, 3)
    s = t.s
    for k in (s.kf, 1):
        for l in (0, 1, 3):
            cts = rows(s.rng, s.mods[:k], s.n, (2, 1 << l, 2))
            cts[1, :, 1] = 0
            cts[1, :] = cts[1, 0]  # item 1: equal leaves with c_1 = 0: every difference is zero and the result transparent
            got, flags = t.select(cts, k, l, flags=True)
            assert flags.tolist() == [True, False], (chain, k, l)
            for c in range(2):
                assert np.array_equal(got[c], G.select(s.ref, s.mods, k, cts[c], t.bit_keys[:l])), (chain, logn, k, l, c)


WALK = dict(chain="ckks nsp1", logn=10, k=2, l=5, count=30)


def _child():
    """N = 2^10, k = 2: ciphertexts of 32 KiB; l = 5 parks 16 + 8 + 16 of them per item, 1.25 MiB, so half of the 64 MiB arena
    takes 25 items and 30 items need a second, ragged chunk. The words must be those of thirty calls of one item, which are
    not chunked; the first and the last item are also held to the restatement; the second chunk's flags land behind the
    first's (item 29's leaves are one ciphertext with c_1 = 0, item 28's are not).
    Refusal: N = 2^12, k = 3, l = 9: the first level of one item parks 640 ciphertexts of 192 KiB, 120 MiB."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    t = Tree(S, WALK["chain"], WALK["logn"], WALK["l"])
    s, k, l, count = t.s, WALK["k"], WALK["l"], WALK["count"]
    ct_bytes = 2 * k * s.n * 8
    cap = (int(ARENA_MB) << 20) // 2 - 3 * 256
    items = cap // (((1 << (l - 1)) * 2 + (1 << (l - 2))) * ct_bytes)
    assert items == 25
    cts = rows(s.rng, s.mods[:k], s.n, (count, 1 << l, 2))
    cts[29, :, 1] = 0
    cts[29, :] = cts[29, 0]  # (equal leaves with c_1 = 0: a transparent result)
    s.ctx.chunk_log()
    got, flags = t.select(cts, k, l, flags=True)
    log = s.ctx.chunk_log()
    assert log[-1] == (count, items), log[-4:]
    assert flags.tolist() == [True] * 29 + [False]
    for c in range(count):
        one, _ = t.select(cts[c:c + 1], k, l)
        assert s.ctx.chunk_log()[-1] == (1, 1)
        assert np.array_equal(got[c], one[0]), c
    for c in (0, count - 1):
        assert np.array_equal(got[c], G.select(s.ref, s.mods, k, cts[c], t.bit_keys[:l])), c

    big = Tree(S, "ckks nsp1", 12, 9)
    n = big.s.n
    item = 640 * 2 * 3 * n * 8
    with pytest.raises(MemoryError, match="first level of one item .%d bytes. does not fit half of the workspace arena .%d bytes." % (item, cap)):
        big.s.ev.select(big.s.ctx.alloc(512 * 2 * 3 * n), 3, 1, big.bits, big.s.ctx.alloc(2 * 3 * n))
    print("RGSW_SELECT_CHUNKS_OK")


def test_select_chunked_items_and_refusal(S):
    run_arena_child(__file__, "RGSW_SELECT_CHUNKS_OK", timeout=300)


# ---------------------------------------------------------------- semantic runs through the device Decryptor
class Real:
    """contexts on both sides, an oracle client for the secret and the encryptions, RGSW objects made on the device"""

    def __init__(self, S, scheme, logn, bits, nsp, t, seed):
        self.n = 1 << logn
        self.mods = O.coeff_modulus_create(self.n, bits)
        self.ref = O.RefContext(scheme, logn, self.mods, nsp=nsp, t=t, mode=1)
        self.cl = O.Client(self.ref, seed=seed)
        self.ctx = S.Context(scheme, logn, self.mods, nsp, t, mode=S.MODE_STRICT)
        self.ev = S.Evaluator(self.ctx)
        self.k = self.cl.k
        self.d = (self.k + nsp - 1) // nsp
        self.sk = self.ctx.upload(self.cl.sk)
        self.rng = np.random.default_rng(seed)

    def rgsw(self, ms):
        ms = np.ascontiguousarray(ms, dtype=np.int32)
        seeds = self.rng.integers(0, 2**64, size=(len(ms), 2, self.d, 8), dtype=np.uint64, endpoint=False)
        noise = self.rng.integers(-19, 20, size=(len(ms), 2, self.d, self.n), dtype=np.int32)
        return self.ctx.generate_rgsw(self.sk, self.ctx.upload_i32(ms), len(ms), self.k, seeds, self.ctx.upload_i32(noise))

    def bits(self, index, l):
        return self.rgsw([G.monomial(self.n, 0) * ((index >> b) & 1) for b in range(l)])


def test_semantic_bfv(S):
    """BFV, STRICT, t = 65537, log N = 12: select over 8 encrypted rows with the RGSW bits of index 5 decrypts to row 5, and the
    external product by RGSW(X^3) to the rotated plaintext, exactly"""
    t, n = 65537, 4096
    r = Real(S, 1, 12, [40, 40, 41, 50], 1, t, seed=12)
    ctx, k = r.ctx, r.k
    plains = r.rng.integers(0, t, size=(8, n), dtype=np.uint64)
    cts = ctx.upload(np.stack([r.cl.encrypt_bfv(p) for p in plains]))
    out, plain = ctx.alloc(2 * k * n), ctx.alloc(n)
    r.ev.select(cts, k, 1, r.bits(5, 3), out)
    ctx.decrypt(out, 2, k, 1, r.sk, False, plain)
    assert np.array_equal(plain.download(), plains[5])
    (g,) = r.rgsw([G.monomial(n, 3)])
    r.ev.external_product(cts, k, 1, g, out)
    ctx.decrypt(out, 2, k, 1, r.sk, False, plain)
    want = np.concatenate([(t - plains[0][n - 3:]) % t, plains[0][:n - 3]])
    assert np.array_equal(plain.download(), want)


def test_semantic_ckks(S):
    """CKKS at the moduli of CASES_16, scale 2^40: the same two runs within G.CKKS_REL_BOUND of the largest message coefficient"""
    scheme, bits, nsp, _ = CASES_16["ckks"]
    n = 16
    r = Real(S, scheme, 4, bits, nsp, 0, seed=5)
    ctx, k, cl = r.ctx, r.k, r.cl
    msgs = [[int(round(float(v) * 2.0 ** 40)) for v in r.rng.uniform(-1, 1, size=n)] for _ in range(8)]
    biggest = max(abs(v) for m in msgs for v in m)
    cts = ctx.upload(np.stack([cl.encrypt_poly_ntt(m) for m in msgs]))
    out, plain = ctx.alloc(2 * k * n), ctx.alloc(k * n)

    def rel_error(want):
        ctx.decrypt(out, 2, k, 1, r.sk, True, plain)
        phase, _ = cl.centered_from_ntt_rows(plain.download((k, n)))
        return max(abs(a - b) for a, b in zip(phase, want)) / biggest

    r.ev.select(cts, k, 1, r.bits(5, 3), out)
    rel = rel_error(msgs[5])
    print("ckks device select(l = 3): relative error 2^%.1f" % (np.log2(rel) if rel else -np.inf))
    assert rel <= G.CKKS_REL_BOUND, rel
    (g,) = r.rgsw([G.monomial(n, 3)])
    r.ev.external_product(cts, k, 1, g, out)
    rel = rel_error([-v for v in msgs[0][n - 3:]] + msgs[0][:n - 3])
    print("ckks device external product by X^3: relative error 2^%.1f" % (np.log2(rel) if rel else -np.inf))
    assert rel <= G.CKKS_REL_BOUND, rel


def test_pir_end_to_end(S):
    """BFV STRICT, log N = 4: the query Delta X^idx expanded into 16 with the normalisation, summed against a 4 x 16 table of
    batch-encoded plaintexts, the four sums folded by a CMux tree under two RGSW bits of the row index: db[row][idx], exactly"""
    import expand_ref as X

    scheme, bits, nsp, t = CASES_16["bfv"]
    N, n_rows = 16, 4
    r = Real(S, scheme, 4, bits, nsp, t, seed=3)
    ctx, k, cl = r.ctx, r.k, r.cl
    gk = {g: S.KSwitchKeys(ctx, cl.galois_key(g)) for g in X.galois_elts(4, N)}
    db = r.rng.integers(0, t, size=(n_rows, N, N), dtype=np.uint64)  # db[s][i]: the N slot values of entry i of row s
    encoded = ctx.alloc(n_rows * N * N)
    ctx.batch_encode(ctx.upload(db), N, n_rows * N, encoded)
    plain_ntt = ctx.alloc(n_rows * N * k * N)
    r.ev.transform_plain_to_ntt(encoded, N, k, n_rows * N, plain_ntt)
    for idx, row in ((0, 0), (5, 2), (15, 3), (9, 1)):
        query = np.zeros(N, dtype=np.uint64)
        query[idx] = 1
        expanded = ctx.alloc(N * 2 * k * N)
        r.ev.expand(ctx.upload(cl.encrypt_bfv(query)), k, 1, N, gk, expanded, normalize=True)
        r.ev.transform_to_ntt_inplace(expanded, 2, k, N)
        sums = ctx.alloc(n_rows * 2 * k * N)
        r.ev.dot_plain(expanded, plain_ntt, k, 1, N, n_rows, sums)
        r.ev.transform_from_ntt_inplace(sums, 2, k, n_rows)
        picked, plain, values = ctx.alloc(2 * k * N), ctx.alloc(N), ctx.alloc(N)
        r.ev.select(sums, k, 1, r.bits(row, 2), picked)
        ctx.decrypt(picked, 2, k, 1, r.sk, False, plain)
        ctx.batch_decode(plain, 1, values)
        assert np.array_equal(values.download(), db[row, idx]), (idx, row)


# ---------------------------------------------------------------- refusals and edges
def test_refusals_and_the_empty_batch(S):
    """the checks that need handles: an RGSW with too few digits or made for a lower level, halves that differ, overlap and
    alignment on a device context, PARITY BFV, the sink's capacity; the empty batch writes nothing"""
    logn, n, k = 8, 256, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    rng = np.random.default_rng(2)
    key = rows(rng, mods, n, (3, 2))
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    full, short = S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, key[:2])
    with pytest.raises(ValueError, match="same digit count and level"):
        ctx.rgsw_create(full, short)
    g, g_short = ctx.rgsw_create(full, full), ctx.rgsw_create(short, short)
    ct_h = rows(rng, mods[:k], n, (4, 2))
    ct, ct1 = ctx.upload(ct_h), ctx.upload(ct_h)
    out = ctx.alloc(2 * 2 * k * n)
    sentinel = np.full(out.words, 7, dtype=np.uint64)
    out.upload(sentinel)
    calls = {"external_product": lambda g, o, c=2: ev.external_product(ct, k, c, g, o),
             "cmux": lambda g, o, c=2: ev.cmux(ct, ct1, k, c, g, o),
             "select": lambda g, o, c=2: ev.select(ct, k, c, [g], o)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="rgsw is not valid for encryption parameters"):
            call(g_short, out)
        with pytest.raises(ValueError, match="rgsw is not valid for encryption parameters"):
            call(g_short, out, 0)  # (the handle is checked before the empty batch returns)
        with pytest.raises(ValueError, match="overlap"):
            call(g, ct.ptr + 16)
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(g, out.ptr + 8)
        call(g, out, 0)  # the empty batch
        assert np.array_equal(out.download(), sentinel), name
    ev.external_product(ct, 2, 2, g_short, out)  # (two digits are enough one level below)
    with pytest.raises(ValueError, match="overlap"):
        ev.external_product(ct, k, 2, g, out, base=out.ptr + 16)
    # an RGSW generated for level 1 serves level 1 only
    cl = O.Client(O.RefContext(2, logn, mods, nsp=1), seed=1)
    sk = ctx.upload(cl.sk)
    seeds = rng.integers(0, 2**64, size=(1, 2, 3, 8), dtype=np.uint64, endpoint=False)
    noise = ctx.upload_i32(rng.integers(-19, 20, size=(1, 2, 3, n), dtype=np.int32))
    (low,) = ctx.generate_rgsw(sk, ctx.upload_i32(G.monomial(n, 1).astype(np.int32)), 1, 1, seeds, noise)
    with pytest.raises(ValueError, match="rgsw is not valid for encryption parameters"):
        ev.external_product(ct, 2, 2, low, out)
    ev.external_product(ct, 1, 2, low, out)
    with pytest.raises(ValueError, match="level k out of range"):
        ctx.generate_rgsw(sk, ctx.upload_i32(G.monomial(n, 1).astype(np.int32)), 1, 4, seeds, noise)
    ctx.transparency_sink(ctx.alloc(2), 1)
    try:
        for call in calls.values():
            with pytest.raises(ValueError, match="sink"):
                call(g, out)
    finally:
        ctx.transparency_sink(None, 0)
    # BFV in PARITY mode: the object can be built, the evaluator entries refuse
    parity = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, mode=S.MODE_PARITY)
    pkey = S.KSwitchKeys(parity, key)
    pg = parity.rgsw_create(pkey, pkey)
    pct, pout = parity.upload(ct_h), parity.alloc(out.words)
    pev = S.Evaluator(parity)
    for call in (lambda: pev.external_product(pct, k, 2, pg, pout), lambda: pev.cmux(pct, pct, k, 2, pg, pout),
                 lambda: pev.select(pct, k, 2, [pg], pout)):
        with pytest.raises(ValueError, match="STRICT"):
            call()


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_rgsw_check.cpp: RgswCiphertext, KeyGenerator::rgsw and Evaluator::external_product / cmux / select
    on resident and on host operands give the ABI's words on the same seeded inputs, with the operands' metadata; the ABI's
    refusals arrive as std::invalid_argument with the wording the Python path sees"""
    from test_gpu_keygen import splitmix

    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_rgsw_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    sm = O.SplitMix(0x29A5)
    cts = np.stack([sm.fill(2 * k, n, mods[:k] * 2).reshape(2, k, n) for _ in range(4)])
    keys = [sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n) for _ in range(2)]
    sk = sm.fill(4, n, mods)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    kb, ka = (S.KSwitchKeys(ctx, key) for key in keys)
    g, g2 = ctx.rgsw_create(kb, ka), ctx.rgsw_create(ka, kb)
    d = ctx.upload(cts)
    ct_words = 2 * k * n
    d0, d1 = d.ptr, d.ptr + ct_words * 8
    out = ctx.alloc(ct_words)
    want = {}
    ev.external_product(d0, k, 1, g, out, base=d1)
    want["device external_product"] = want["host external_product"] = want["device external_product recreated"] = out.download()
    ev.external_product(d0, k, 1, g, out)
    want["device external_product no base"] = out.download()
    ev.cmux(d0, d1, k, 1, g, out)
    want["device cmux"] = want["host cmux"] = out.download()
    ev.select(d, k, 1, [g, g2], out)
    want["device select"] = want["host select"] = out.download()
    want["device select l0"] = cts[2]
    st = [0xCAFE29]
    seeds, noise = np.zeros((1, 2, 3, 8), dtype=np.uint64), np.zeros((1, 2, 3, n), dtype=np.int32)
    for h in range(2):
        for j in range(3):
            seeds[0, h, j] = [splitmix(st) for _ in range(8)]
            noise[0, h, j] = [splitmix(st) % 83 - 41 for _ in range(n)]
    m = np.zeros((1, n), dtype=np.int32)
    m[0, 0], m[0, 3] = 1, -1
    (made,) = ctx.generate_rgsw(ctx.upload(sk), ctx.upload_i32(m), 1, k, seeds, ctx.upload_i32(noise))
    ev.external_product(d0, k, 1, made, out)
    want["device external_product generated"] = out.download()
    for name, words in want.items():
        line = "%s digest %016x meta 1" % (name, O.fnv(words))
        assert line in stdout, (line, stdout)
    assert "refusals ok" in stdout, stdout


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
