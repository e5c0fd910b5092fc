"""Blind rotation on the device (sealhip_evaluator_multiply_monomial, sealhip_lwe_mod_switch,
sealhip_generate_blind_rotation_keys, sealhip_evaluator_blind_rotate) against the restatement of
tests/blind_rotate_ref.py and against the compositions from the entries that existed before, word for word.

Shapes: rings of 2^3 (all 16 exponents, so 0, 1, N - 1, N, N + 1 and 2N - 1 occur) and 2^4 (less than a workgroup per row),
2^8 and 2^9 (one and two workgroups per row) and 2^12; batches of 1, 2 and 17 with a different exponent per item; levels 3, 2
and 1; 61-bit primes and the 61/20/45/61 chain; CKKS in both modes and BFV in STRICT. Word comparisons need no valid keys: an
RGSW block is two random keys. The semantic runs use keys the library generated.

The file's name sorts behind every other device test on purpose. tests/test_gpu_dot_ct.py::test_refusals_that_need_a_device
hands dot_product a batch of two over operands of one ciphertext and expects the sink's refusal, which the entry reaches only
when the words behind its operands do not happen to be `out`: where the device allocator places three blocks depends on what
was allocated and freed before. Run ahead of it (as test_gpu_blind_rotate.py would be), this file's allocations change that
placement and the overlap check answers first. Behind the others it changes nothing they see."""
import os
import sys

import numpy as np
import pytest

import blind_rotate_ref as B
import oracle_lib as O
import rgsw_ref as G
from support import ARENA_MB, BaseSession, S, child_main, rows, run_arena_child, session_memo, top

pytestmark = pytest.mark.gpu
SENTINEL = 0x5E5E5E5E5E5E5E5E
# name: (scheme, bit sizes, nsp, t, mode)   mode 1 = STRICT, 0 = PARITY
CHAINS = {
    "ckks": (2, [40, 40, 40, 41], 1, 0, 1),
    "ckks parity": (2, [40, 40, 40, 41], 1, 0, 0),
    "bfv": (1, [30, 35, 40, 45], 1, 65537, 1),
    "61": (2, [61] * 4, 1, 0, 1),
    "bfv 61": (1, [61] * 4, 1, 65537, 1),
    "mixed": (2, [61, 20, 45, 61], 1, 0, 1),
    "bfv mixed": (1, [61, 20, 45, 61], 1, 65537, 1),
}


class Session(BaseSession):
    """contexts on both sides and three RGSW blocks of two random keys each (host arrays and the objects)"""

    def __init__(self, S, chain, logn):
        scheme, bits, nsp, t, mode = CHAINS[chain]
        super().__init__(S, scheme, logn, bits, nsp, mode, t, 300 + logn)
        self.chain, self.kf, self.ntt = chain, self.k_first, scheme == 2
        self.keys = [tuple(rows(self.rng, self.mods, self.n, (self.nd, 2)) for _ in range(2)) for _ in range(3)]
        self.handles = [tuple(S.KSwitchKeys(self.ctx, key) for key in pair) for pair in self.keys]
        self.gs = [self.ctx.rgsw_create(*pair) for pair in self.handles]

    def run(self, fn, inputs, count, k, flags_for=None):
        """fn(device inputs..., out) with sentinels behind out; the inputs must come back as they were (uint32 arrays are
        handed in as such); returns the words and, with flags_for, the transparency flags"""
        words = count * 2 * k * self.n
        out = self.ctx.alloc(words + 4)
        out.upload(np.full(words + 4, SENTINEL, dtype=np.uint64))
        dev = [self.ctx.upload_u32(x) if x.dtype == np.uint32 else self.ctx.upload(x) for x in inputs]
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
            back = d.download().view(x.dtype)[:x.size].reshape(x.shape)
            assert np.array_equal(back, x), "an input was modified"
        seen = None
        if flags_for is not None:
            seen = flags.download().view(np.uint32)
            assert np.all(seen[flags_for:] == 5), "flags behind the batch were written"
            seen = seen[:flags_for] != 0
        return got[:words].reshape(count, 2, k, self.n), seen

    def monomial(self, ct, k, count, exps, minus_one, stride=1):
        """ct: (n_ct, 2, k, N) with n_ct 1 or count; exps: uint32, exponent i at i * stride"""
        return self.run(lambda c, e, o: self.ev.multiply_monomial(c, k, count, e, o, n_ct=ct.shape[0], exps_stride=stride,
                                                                  minus_one=minus_one), (ct, exps), count, k)[0]

    def plain_ntt(self, k, e, minus_one):
        """NTT(X^e) (- 1) over the level's rows from the oracle's transform of the one-hot row: (k, N)"""
        out = np.zeros((k, self.n), dtype=np.uint64)
        e %= 2 * self.n
        for r in range(k):
            p = self.mods[r]
            out[r, e % self.n] = 1 if e < self.n else p - 1
            O.lib().ref_ntt_forward(O.ptr(out[r]), self.ref.tables(r), B.STRICT)
            if minus_one:
                out[r] = (out[r] + np.uint64(p - 1)) % np.uint64(p)
        return out

    def check_monomial(self, ct, k, count, exps, minus_one, tag=""):
        """the device's words against the integers and, in NTT form, against multiply_plain_ntt with NTT(X^e [- 1])"""
        where = (self.chain, "N", self.n, "k", k, "count", count, "minus_one", minus_one, tag)
        got = self.monomial(ct, k, count, exps, minus_one)
        items = range(count) if self.n <= 512 else sorted({0, count // 2, count - 1})
        for i in items:
            want = B.multiply_monomial(self.ref, k, ct[i if ct.shape[0] > 1 else 0], int(exps[i]), self.ntt, minus_one)
            assert np.array_equal(got[i], want), where + ("integers, item", i, "e", int(exps[i]))
        if self.ntt:
            work = self.ctx.upload(np.ascontiguousarray(np.broadcast_to(ct, (count, 2, k, self.n))))
            plain = self.ctx.upload(np.stack([self.plain_ntt(k, int(e), minus_one) for e in exps]))
            self.ev.multiply_plain_inplace(work, 2, k, count, plain, plain_stride=k * self.n, ntt_form=True)
            assert np.array_equal(got, work.download(got.shape)), where + ("multiply_plain_ntt",)
        return got

    def rotate(self, tv, k, count, exps, n_steps, flags=False):
        gs = [self.gs[t % 3] for t in range(n_steps)]
        return self.run(lambda c, e, o: self.ev.blind_rotate(c, k, count, e, gs, o, n_tv=tv.shape[0]), (tv, exps), count, k,
                        count if flags else None)

    def composition(self, tv, k, count, exps, n_steps):
        """the definition step by step on the device: multiply_monomial with minus_one, then external_product(target, base = acc)"""
        ctx, ev = self.ctx, self.ev
        words = count * 2 * k * self.n
        e = ctx.upload_u32(exps)
        acc, target, nxt = ctx.alloc(words), ctx.alloc(words), ctx.alloc(words)
        ev.multiply_monomial(ctx.upload(tv), k, count, e, acc, n_ct=tv.shape[0], exps_stride=1 + n_steps)
        for t in range(1, n_steps + 1):
            ev.multiply_monomial(acc, k, count, e.ptr + 4 * t, target, exps_stride=1 + n_steps, minus_one=True)
            ev.external_product(target, k, count, self.gs[(t - 1) % 3], nxt, base=acc)
            acc, nxt = nxt, acc
        return acc.download((count, 2, k, self.n))

    def check_rotate(self, k, count, n_steps, shared, restate):
        where = (self.chain, "N", self.n, "k", k, "count", count, "steps", n_steps, "shared", shared)
        tv = rows(self.rng, self.mods[:k], self.n, (1 if shared else count, 2))
        exps = self.rng.integers(0, 2 * self.n, size=(count, 1 + n_steps)).astype(np.uint32)
        exps[0, 0] = 2 * self.n - 1
        exps[-1, -1] = self.n
        got, flags = self.rotate(tv, k, count, exps, n_steps, flags=True)
        assert flags.all(), where
        assert np.array_equal(got, self.composition(tv, k, count, exps, n_steps)), where + ("device composition",)
        for c in sorted({0, count - 1}) if restate else ():
            want = B.blind_rotate(self.ref, k, tv[0 if shared else c], exps[c], [self.keys[t % 3] for t in range(n_steps)], self.ntt)
            assert np.array_equal(got[c], want), where + ("restatement, item", c)


session = session_memo(Session)


def planted(s, k, count, e):
    """random words with 1 and p - 1 planted in both lanes of the pair at the wrap position of X^e, and of the pair before"""
    ct = rows(s.rng, s.mods[:k], s.n, (count, 2))
    at = (e % s.n) & ~1
    for r in range(k):
        ct[..., r, at], ct[..., r, at + 1] = 1, s.mods[r] - 1
        ct[..., r, at - 2], ct[..., r, at - 1] = s.mods[r] - 1, 1
    return ct


# ---------------------------------------------------------------- the monomial product
@pytest.mark.parametrize("chain", ["ckks", "ckks parity", "bfv", "61", "bfv 61", "mixed", "bfv mixed"])
def test_multiply_monomial_every_exponent_of_the_smallest_ring(S, chain):
    """log N = 3: a batch of 16 items takes the exponents 0 .. 15 in one call, a batch of 17 the odd ones twice over the
    wrap; with and without the subtraction; levels 3, 2 and 1"""
    s = session(S, chain, 3)
    for k in (3, 2, 1):
        ct = rows(s.rng, s.mods[:k], s.n, (16, 2))
        for minus_one in (False, True):
            s.check_monomial(ct, k, 16, np.arange(16, dtype=np.uint32), minus_one)
    ct = rows(s.rng, s.mods[:s.kf], s.n, (17, 2))
    s.check_monomial(ct, s.kf, 17, ((np.arange(17) * 7 + 3) % 16).astype(np.uint32), True)


@pytest.mark.parametrize("chain,logn", [("ckks", 4), ("bfv", 4), ("ckks", 8), ("bfv", 8), ("ckks parity", 9), ("bfv mixed", 9),
                                        ("mixed", 8), ("61", 9), ("bfv 61", 8), ("ckks", 12), ("bfv", 12)])
def test_multiply_monomial_words(S, chain, logn):
    """batches of 1, 2 and 17 with a different exponent per item (0, 1, N - 1, N, N + 1 and 2N - 1 among them); operands of
    all 0, all p - 1, and 1 planted in both lanes of the pair at the wrap; a shared operand; exponents at a stride and
    above 2N"""
    s = session(S, chain, logn)
    n = s.n
    edge = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    for k, count in ((s.kf, 17), (2, 2), (1, 1)):
        exps = np.array((edge + [int(v) for v in s.rng.integers(0, 2 * n, size=17)])[:count], dtype=np.uint32)
        if count == 1:
            exps[0] = n + 5
        for minus_one in (False, True):
            s.check_monomial(rows(s.rng, s.mods[:k], n, (count, 2)), k, count, exps, minus_one)
        s.check_monomial(top(s.mods[:k], n, (count, 2)), k, count, exps, True, tag="all p - 1")
        got = s.check_monomial(np.zeros((count, 2, k, n), dtype=np.uint64), k, count, exps, False, tag="all 0")
        assert not got.any()
        s.check_monomial(rows(s.rng, s.mods[:k], n, (1, 2)), k, count, exps, True, tag="shared")
    for e in (n - 1, n + 3, 6):
        ct = planted(s, s.kf, 2, e)
        s.check_monomial(ct, s.kf, 2, np.array([e, e + 1], dtype=np.uint32), True, tag="planted")
    # a stride of three words, and exponents the kernel reduces modulo 2N
    k, count = s.kf, 2
    ct = rows(s.rng, s.mods[:k], n, (count, 2))
    spread = np.array([5, 99, 99, 2 * n + 7, 99, 99], dtype=np.uint32)
    got = s.monomial(ct, k, count, spread, False, stride=3)
    assert np.array_equal(got, s.monomial(ct, k, count, np.array([5, 7], dtype=np.uint32), False))
    assert np.array_equal(s.monomial(ct, k, count, np.array([4 * n + 1, 0xFFFFFFFF], dtype=np.uint32), True),
                          s.monomial(ct, k, count, np.array([1, 2 * n - 1], dtype=np.uint32), True))


def test_multiply_monomial_flags(S):
    """the read pass: an all-zero c_1 is transparent; X^0 - 1 makes every result zero"""
    s = session(S, "ckks", 8)
    k, count = s.kf, 3
    ct = rows(s.rng, s.mods[:k], s.n, (count, 2))
    ct[1, 1] = 0
    exps = np.array([3, 4, 0], dtype=np.uint32)
    for minus_one, want in ((False, [True, False, True]), (True, [True, False, False])):
        _, flags = s.run(lambda c, e, o: s.ev.multiply_monomial(c, k, count, e, o, minus_one=minus_one), (ct, exps), count, k, count)
        assert flags.tolist() == want


# ---------------------------------------------------------------- the modulus switch
@pytest.mark.parametrize("chain,logn", [("ckks", 3), ("bfv", 4), ("61", 8), ("bfv mixed", 8), ("ckks", 12)])
def test_lwe_mod_switch_words(S, chain, logn):
    """against ms() on random words and on words planted on both sides of rounding boundaries (the wrap to 0 among them),
    binary and ternary layouts, b_offset of 0 and N / t; sentinels behind the rows; the inputs come back as they were"""
    s = session(S, chain, logn)
    n, q = s.n, s.mods[0]
    bounds = [-(-((v + 1) * q - q // 2) // (2 * n)) for v in range(2 * n)]
    bounds = [x for x in bounds if x < q]
    n_samples = 3
    a = s.rng.integers(0, q, size=(n_samples, n), dtype=np.uint64)
    b = s.rng.integers(0, q, size=n_samples, dtype=np.uint64)
    picks = [bounds[-1], bounds[-1] - 1, bounds[0], bounds[0] - 1, 0, q - 1] + [bounds[int(i)] - d for i in
                                                                               s.rng.integers(0, len(bounds), size=n) for d in (0, 1)]
    a[0] = picks[:n]
    a[1, :min(n, len(picks) - n)] = picks[n:2 * n]
    b[0], b[1] = bounds[-1], bounds[-1] - 1
    da, db = s.ctx.upload(a), s.ctx.upload(b)
    for ternary in (False, True):
        for b_offset in (0, n // 8):
            row = 1 + n * (2 if ternary else 1)
            total = n_samples * row
            out = s.ctx.upload_u32(np.full(total + 3, 0x5E5E5E5E, dtype=np.uint32))
            s.ctx.lwe_mod_switch(da, db, n_samples, ternary, b_offset, out)
            got = out.download().view(np.uint32)
            assert np.all(got[total:total + 3] == 0x5E5E5E5E), "words behind exps were written"
            want = B.exps_rows(a.tolist(), b.tolist(), q, n, ternary, b_offset)
            assert np.array_equal(got[:total].reshape(n_samples, row), want), (chain, logn, ternary, b_offset)
            assert want[0, 0] == (-b_offset) % (2 * n) and want[1, 0] == (1 - b_offset) % (2 * n)  # (the wrap, and below it)
    assert np.array_equal(da.download(a.shape), a) and np.array_equal(db.download(), b)
    s.ctx.lwe_mod_switch(da, db, 0, False, 0, out)  # the empty batch


# ---------------------------------------------------------------- the key generator
@pytest.mark.parametrize("ternary", [False, True], ids=["binary", "ternary"])
@pytest.mark.parametrize("scheme,logn,bits,nsp", [(2, 4, [30, 35, 40, 45, 50], 1), (1, 8, [36, 36, 37, 40, 60, 60], 2)])
def test_generate_blind_rotation_keys_word_for_word(S, scheme, logn, bits, nsp, ternary):
    """every word is generate_rgsw's for the indicator messages with the same samples; the full level and level 1"""
    from test_gpu_keygen import Setup

    st = Setup(S, scheme, logn, bits, nsp)
    ctx, n = st.ctx, st.n
    n_lwe = 5
    secret = np.array([1, -1 if ternary else 0, 0, 1, -1 if ternary else 1, 0], dtype=np.int32)  # (padded to an even count)
    bits_ = B.indicators(secret[:n_lwe], ternary)
    ms = np.zeros((len(bits_), n), dtype=np.int32)
    ms[:, 0] = bits_
    seeds, noise = st.samples(2 * len(bits_))
    dn, ds = ctx.upload_i32(noise), ctx.upload_i32(secret)
    for level in (st.k, 1):
        made = ctx.generate_blind_rotation_keys(st.sk, ds, n_lwe, ternary, level, seeds, dn)
        want = ctx.generate_rgsw(st.sk, ctx.upload_i32(ms), len(bits_), level, seeds, dn)
        assert len(made) == len(want) == n_lwe * (2 if ternary else 1)
        for i, (g, w) in enumerate(zip(made, want)):
            assert S.save_kswitch_keys(ctx, list(ctx.rgsw_export(g))) == S.save_kswitch_keys(ctx, list(ctx.rgsw_export(w))), (level, i)
    assert np.array_equal(ds.download().view(np.int32), secret)
    assert ctx.generate_blind_rotation_keys(st.sk, None, 0, ternary, st.k, seeds[:0], None) == []


# ---------------------------------------------------------------- the rotation, word for word
@pytest.mark.parametrize("chain", ["ckks", "ckks parity", "bfv"])
@pytest.mark.parametrize("logn", [3, 4])
def test_blind_rotate_small_rings(S, chain, logn):
    """n_steps = 0, 1, 2 and 2N; batches of 1 and 17; the first level and level 1; a shared and a per-item test vector"""
    s = session(S, chain, logn)
    for n_steps in (0, 1, 2, 2 * s.n):
        for k, count, shared in ((s.kf, 17, True), (s.kf, 1, False), (1, 17, False), (1, 1, True)):
            s.check_rotate(k, count, n_steps, shared, restate=True)


@pytest.mark.parametrize("chain", ["ckks", "ckks parity", "bfv"])
def test_blind_rotate_log8(S, chain):
    s = session(S, chain, 8)
    for n_steps in (0, 1, 2):
        s.check_rotate(s.kf, 17, n_steps, True, restate=True)
        s.check_rotate(1, 1, n_steps, False, restate=True)
    s.check_rotate(s.kf, 17, 2 * s.n, False, restate=False)  # (512 steps: against the device composition)
    s.check_rotate(1, 1, 2 * s.n, True, restate=True)


def test_blind_rotate_flags(S):
    """the flags come from the last step's mod-down, or from the read pass when there is no step"""
    s = session(S, "ckks", 8)
    k, count = s.kf, 3
    tv = rows(s.rng, s.mods[:k], s.n, (count, 2))
    tv[1] = 0
    exps = s.rng.integers(0, 2 * s.n, size=(count, 3)).astype(np.uint32)
    for n_steps in (0, 2):
        got, flags = s.rotate(tv, k, count, np.ascontiguousarray(exps[:, :1 + n_steps]), n_steps, flags=True)
        assert flags.tolist() == [True, False, True] and not got[1].any()


WALK = {"chain": "ckks", "logn": 12, "count": 64, "steps": 2}


def _child():
    """N = 2^12, k = 3, one special prime: an item's arena is 2 x 3 rows in the other form, 2 x 3 digits of 4 rows, two
    products of 4 rows and two temporaries of 3, and the target of 2 x 3: 50 rows of 32 KiB, so the 64 MiB arena takes 40 items
    and 64 items need a second, ragged chunk. The words must be those of 64 calls of one item, which are not chunked."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    s = Session(S, WALK["chain"], WALK["logn"])
    k, count, n_steps = s.kf, WALK["count"], WALK["steps"]
    items = (int(ARENA_MB) << 20) // (50 * s.n * 8)
    assert items == 40
    tv = rows(s.rng, s.mods[:k], s.n, (count, 2))
    tv[63, 1] = 0
    exps = s.rng.integers(0, 2 * s.n, size=(count, 1 + n_steps)).astype(np.uint32)
    exps[63, 1:] = 0  # (X^0 - 1 = 0: the last item of the second chunk stays transparent)
    s.ctx.chunk_log()
    got, flags = s.rotate(tv, k, count, exps, n_steps, flags=True)
    assert s.ctx.chunk_log()[-1] == (count, items), s.ctx.chunk_log()[-4:]
    assert flags.tolist() == [True] * 63 + [False]
    for c in range(count):
        one, _ = s.rotate(tv[c:c + 1], k, 1, exps[c:c + 1], n_steps)
        assert s.ctx.chunk_log()[-1] == (1, 1)
        assert np.array_equal(got[c], one[0]), c
    print("BLIND_ROTATE_CHUNKS_OK")


def test_blind_rotate_chunked_items(S):
    run_arena_child(__file__, "BLIND_ROTATE_CHUNKS_OK", timeout=300)


# ---------------------------------------------------------------- semantic runs
class Real:
    """contexts on both sides, an oracle client for the encryptions and the decryption, blind-rotation keys made on the device"""

    def __init__(self, S, scheme, logn, bits, nsp, t, seed):
        self.n = 1 << logn
        self.mods = O.coeff_modulus_create(self.n, bits)
        self.ref = O.RefContext(scheme, logn, self.mods, nsp=nsp, t=t, mode=1)
        self.cl = O.Client(self.ref, seed=seed)
        self.ctx = S.Context(scheme, logn, self.mods, nsp, t, mode=S.MODE_STRICT)
        self.ev = S.Evaluator(self.ctx)
        self.k = self.cl.k
        self.d = (self.k + nsp - 1) // nsp
        self.rng = np.random.default_rng(seed)

    def keys(self, secret, ternary):
        n_steps = len(secret) * (2 if ternary else 1)
        seeds = self.rng.integers(0, 2**64, size=(n_steps, 2, self.d, 8), dtype=np.uint64, endpoint=False)
        noise = self.rng.integers(-19, 20, size=(n_steps, 2, self.d, self.n), dtype=np.int32)
        return self.ctx.generate_blind_rotation_keys(self.ctx.upload(self.cl.sk), self.ctx.upload_i32(secret.astype(np.int32)),
                                                     len(secret), ternary, self.k, seeds, self.ctx.upload_i32(noise))


def exact_exponent_run(r, tv):
    """two samples directly modulo 2N under a ternary secret, one shared test vector: (outputs, phi~ per item)"""
    n = r.n
    secret = r.rng.integers(-1, 2, size=n)
    a2 = r.rng.integers(0, 2 * n, size=(2, n))
    b2 = [int(v) for v in r.rng.integers(0, 2 * n, size=2)]
    exps = np.array([B.exps_from_switched(b2[i], a2[i], n, True) for i in range(2)], dtype=np.uint32)
    bits = B.indicators(secret, True)
    out = r.ctx.alloc(2 * 2 * r.k * n)
    r.ev.blind_rotate(r.ctx.upload(tv), r.k, 2, r.ctx.upload_u32(exps), r.keys(secret, True), out)
    return out.download((2, 2, r.k, n)), [B.phi_tilde(exps[i], bits, n) for i in range(2)]


def test_semantic_bfv_exact_exponents(S):
    """BFV, STRICT, t = 65537, log N = 8, 512 steps: decrypts to X^(-phi~) tv exactly"""
    t = 65537
    r = Real(S, 1, 8, [40, 40, 41, 50], 1, t, seed=30)
    plain = r.rng.integers(0, t, size=r.n, dtype=np.uint64)
    out, phis = exact_exponent_run(r, r.cl.encrypt_bfv(plain))
    for i in range(2):
        assert r.cl.decrypt_bfv(out[i]).tolist() == B.rotated(plain, phis[i], t), i


def test_semantic_ckks_exact_exponents(S):
    """CKKS at the shape the restatement's error was measured at (tests/test_blind_rotate_host.py): within B.CKKS_REL_BOUND
    of the largest message coefficient"""
    scheme, bits, nsp, _ = B.CKKS_256
    r = Real(S, scheme, 8, bits, nsp, 0, seed=31)
    msg = [int(round(float(v) * 2.0 ** 40)) for v in r.rng.uniform(-1, 1, size=r.n)]
    out, phis = exact_exponent_run(r, r.cl.encrypt_poly_ntt(msg))
    for i in range(2):
        want = B.rotated(msg, phis[i], 1 << 80)
        want = [v - (1 << 80) if v > 1 << 79 else v for v in want]
        got, _ = G.phase(r.cl, out[i], True)
        rel = max(abs(a - b) for a, b in zip(got, want)) / max(abs(v) for v in msg)
        print("ckks device blind rotation, 512 steps: relative error 2^%.1f" % np.log2(rel))
        assert rel <= B.CKKS_REL_BOUND, rel


def test_lookup_end_to_end(S):
    """BFV STRICT, log N = 8, a generate_sparse_secret_key secret of weight 16, t = 8, messages in [0, 4) in the coefficients:
    the ciphertext goes down to level 1, eight coefficients are extracted as LWE samples and switched to modulus 2N, and the
    blind rotation of lut_test_vector(f) at the first level leaves f(m) in the constant coefficient of every output"""
    from test_blind_rotate_host import E2E_H, E2E_LOGN, E2E_T

    t, n = E2E_T, 1 << E2E_LOGN
    r = Real(S, 1, E2E_LOGN, [30, 35, 40, 45], 1, t, seed=32)
    ctx, ev, k, cl = r.ctx, r.ev, r.k, r.cl
    sk = ctx.generate_sparse_secret_key(r.rng.integers(0, 2**64, size=8, dtype=np.uint64, endpoint=False), E2E_H)
    cl.sk = sk.download((len(r.mods), n))
    s_row = cl.sk[0].copy()
    O.lib().ref_ntt_inverse(O.ptr(s_row), r.ref.tables(0))
    q0 = r.mods[0]
    secret = np.array([int(v) - q0 if int(v) > q0 // 2 else int(v) for v in s_row], dtype=np.int32)
    assert set(secret.tolist()) <= {-1, 0, 1} and np.count_nonzero(secret) == E2E_H
    cl.s = secret.astype(np.int8)
    f = lambda m: (5 * m * m + 3) % t  # 3, 0, 7, 0: not monotone
    messages = r.rng.integers(0, t // 2, size=n, dtype=np.uint64)
    ct = ctx.upload(cl.encrypt_bfv(messages))
    for level in range(k, 1, -1):
        nxt = ctx.alloc(2 * (level - 1) * n)
        ev.mod_switch_to_next(ct, 2, level, 1, nxt)
        ct = nxt
    idx = [0, 1, 2, 3, 100, 101, n - 2, n - 1]
    lwe_a, lwe_b = ctx.alloc(len(idx) * n), ctx.alloc(len(idx))
    ev.extract_lwe(ct, 1, 1, idx, lwe_a, lwe_b)
    exps = ctx.alloc((len(idx) * (1 + 2 * n) + 1) // 2)
    ctx.lwe_mod_switch(lwe_a, lwe_b, len(idx), True, n // t, exps)
    keys = r.keys(secret, True)  # (under cl.sk, which is the device's secret now)
    tv = S.lut_test_vector(f, t, n).astype(np.uint64)
    out = ctx.alloc(len(idx) * 2 * k * n)
    ev.blind_rotate(ctx.upload(cl.encrypt_bfv(tv)), k, len(idx), exps, keys, out)
    got = out.download((len(idx), 2, k, n))
    for j, i in enumerate(idx):
        assert int(cl.decrypt_bfv(got[j])[0]) == f(int(messages[i])), (j, i, int(messages[i]))


# ---------------------------------------------------------------- refusals and edges
def test_refusals_and_the_empty_batch(S):
    """the checks that need handles: an RGSW with too few digits, overlap and alignment on a device context, PARITY BFV, the
    sink's capacity; the empty batch writes nothing"""
    logn, n, k = 8, 256, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    rng = np.random.default_rng(2)
    key = rows(rng, mods, n, (3, 2))
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    full, short = S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, key[:2])
    g, g_short = ctx.rgsw_create(full, full), ctx.rgsw_create(short, short)
    ct = ctx.upload(rows(rng, mods[:k], n, (2, 2)))
    exps = ctx.upload_u32(np.array([1, 2, 3, 4], dtype=np.uint32))
    out = ctx.alloc(2 * 2 * k * n)
    sentinel = np.full(out.words, 7, dtype=np.uint64)
    out.upload(sentinel)
    calls = {"multiply_monomial": lambda g, o, c=2: ev.multiply_monomial(ct, k, c, exps, o),
             "blind_rotate": lambda g, o, c=2: ev.blind_rotate(ct, k, c, exps, [g], o, n_tv=c)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="overlap"):
            call(g, ct.ptr + 16)
        with pytest.raises(ValueError, match="overlap"):
            call(g, exps.ptr - 16)
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(g, out.ptr + 8)
        call(g, out, 0)  # the empty batch
        assert np.array_equal(out.download(), sentinel), name
    with pytest.raises(ValueError, match="rgsw is not valid for encryption parameters"):
        calls["blind_rotate"](g_short, out)
    with pytest.raises(ValueError, match="rgsw is not valid for encryption parameters"):
        calls["blind_rotate"](g_short, out, 0)  # (the handles are checked before the empty batch returns)
    with pytest.raises(ValueError, match="or count"):
        ev.blind_rotate(ct, k, 2, exps, [g], out, n_tv=3)
    ev.blind_rotate(ct, 2, 2, exps, [g_short], out, n_tv=2)  # (two digits are enough one level below)
    ctx.transparency_sink(ctx.alloc(2), 1)
    try:
        for call in calls.values():
            with pytest.raises(ValueError, match="sink"):
                call(g, out)
    finally:
        ctx.transparency_sink(None, 0)
    with pytest.raises(ValueError, match="aligned"):
        ctx.lwe_mod_switch(ct.ptr + 8, ct, 1, False, 0, out)
    parity = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, mode=S.MODE_PARITY)
    pkey = S.KSwitchKeys(parity, key)
    pg = parity.rgsw_create(pkey, pkey)
    pct, pout, pexps = parity.upload(np.zeros(2 * 2 * k * n, dtype=np.uint64)), parity.alloc(out.words), parity.upload_u32(np.arange(4))
    pev = S.Evaluator(parity)
    for call in (lambda: pev.multiply_monomial(pct, k, 2, pexps, pout), lambda: pev.blind_rotate(pct, k, 2, pexps, [pg], pout, n_tv=2)):
        with pytest.raises(ValueError, match="STRICT"):
            call()


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_blind_rotate_check.cpp: KeyGenerator::blind_rotation_keys and Evaluator::multiply_monomial /
    blind_rotate on resident and on host operands give the ABI's words on the same seeded inputs, with the operand's metadata"""
    from support import compile_cpp, run_exe
    from test_gpu_keygen import splitmix

    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_blind_rotate_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    sm = O.SplitMix(0x30A5)
    ct = sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n)
    sk = sm.fill(4, n, mods)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    st = [0xCAFE30]
    seeds, noise = np.zeros((6, 2, 3, 8), dtype=np.uint64), np.zeros((6, 2, 3, n), dtype=np.int32)
    for i in range(6):
        for h in range(2):
            for j in range(3):
                seeds[i, h, j] = [splitmix(st) for _ in range(8)]
                noise[i, h, j] = [splitmix(st) % 83 - 41 for _ in range(n)]
    keys = ctx.generate_blind_rotation_keys(ctx.upload(sk), ctx.upload_i32(np.array([1, -1, 0, 0], dtype=np.int32)), 3, True, k,
                                            seeds, ctx.upload_i32(noise))
    d, out = ctx.upload(ct), ctx.alloc(2 * k * n)
    want = {}
    ev.multiply_monomial(d, k, 1, ctx.upload_u32(np.array([4099], dtype=np.uint32)), out, minus_one=True)
    want["device multiply_monomial"] = want["host multiply_monomial"] = out.download()
    ev.blind_rotate(d, k, 1, ctx.upload_u32(np.array([5, 4097, 8191, 1, 0, 77, 4096], dtype=np.uint32)), keys, out)
    want["device blind_rotate"] = want["host blind_rotate"] = want["device blind_rotate in place"] = out.download()
    for name, words in want.items():
        line = "%s digest %016x meta 1" % (name, O.fnv(words))
        assert line in stdout, (line, stdout)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
