"""Oblivious expansion and the sums against plaintext rows on the device (sealhip_evaluator_expand / _dot_plain, DESIGN.md
section 28) against the CPU restatements of tests/expand_ref.py, word for word.

Shapes: the smallest that reach every path. The expansion at N = 2^4 runs every n, both levels, with and without the
normalisation (random keys: a word comparison needs no valid ones), with 0, 1 and p - 1 planted where the wrap sign and
the automorphism's sign split read; at N = 2^3 less than one wavefront of pairs and a shift of N / 2; at N = 2^12 several
workgroups per row in both kernel forms. The sums run the group edges (1, 16, 17, 33 terms), the tile edges (1, 4, 5
sums), both sides of the block-in-row switch (N = 2^9 against 2^10) and the largest integer sum the kernel can see. The
chunked walks run in a child process under the smallest arena."""
import os
import sys

import numpy as np
import pytest

import expand_ref as X
import oracle_lib as O
import ring_pack_ref as R
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe, top

pytestmark = pytest.mark.gpu
SENTINEL = 0x5E5E5E5E5E5E5E5E
CASES_16 = {"bfv": (1, [30, 35, 40, 45, 50], 1, 65537), "ckks": (2, [40] * 5 + [41] * 2, 2, 0)}


class Session(BaseSession):
    """contexts on both sides, keys for every element of the expansion into N (host arrays and device handles): random
    ones, or (client) an O.Client's"""

    def __init__(self, S, scheme, logn, bits, nsp, t=0, seed=0, client=False, mode=1):
        super().__init__(S, scheme, logn, bits, nsp, mode, t, seed + logn)
        self.kf = self.k_first
        elts = X.galois_elts(logn, self.n)
        assert self.ctx.expand_galois_elts(self.n) == elts
        if client:
            self.cl = O.Client(self.ref, seed=seed + 1)
            self.keys = {g: self.cl.galois_key(g) for g in elts}
        else:
            self.keys = {g: rows(self.rng, self.mods, self.n, (self.nd, 2)) for g in elts}
        self.dkeys = {g: S.KSwitchKeys(self.ctx, key) for g, key in self.keys.items()}

    def expand(self, ct, k, n, normalize):
        """the device's [count][n][2][k][N]; sentinel words behind out and the input must come back as they were"""
        count = ct.shape[0]
        words = count * n * 2 * k * self.n
        out = self.ctx.alloc(words + 4)
        out.upload(np.full(words + 4, SENTINEL, dtype=np.uint64))
        d = self.ctx.upload(ct)
        self.ev.expand(d, k, count, n, self.dkeys, out, normalize=normalize)
        got = out.download()
        assert np.all(got[words:] == SENTINEL), "words behind out were written"
        assert np.array_equal(d.download(ct.shape), ct), "the input was modified"
        return got[:words].reshape(count, n, 2, k, self.n)

    def compare(self, k, count, n, normalize, tag, ct=None):
        if ct is None:
            ct = rows(self.rng, self.mods[:k], self.n, (count, 2))
        got = self.expand(ct, k, n, normalize)
        want = X.expand_batch(self.ref, self.mods, k, ct, self.keys, n, normalize)
        for c in range(count):
            for i in range(n):
                assert np.array_equal(got[c, i], want[c, i]), (tag, "k", k, "n", n, "normalize", normalize, "item", c, "out", i)


def planted(s, k, count):
    """random ciphertexts with 0, 1 and p - 1 at the coefficients 0, 1, sh - 1, sh, N - sh - 1, N - sh, N - 1 of both
    polynomials, for every shift sh = 2^u < N: where the wrap of X^(-sh) and the sign of sigma_g split"""
    N = s.n
    ct = rows(s.rng, s.mods[:k], N, (count, 2))
    spots = sorted({c % N for u in range(s.logn) for sh in [1 << u] for c in (0, 1, sh - 1, sh, N - sh - 1, N - sh, N - 1)})
    for c in range(count):
        for j in range(2):
            for r in range(k):
                for a, pos in enumerate(spots):
                    ct[c, j, r, pos] = (0, 1, s.mods[r] - 1)[(c + j + r + a) % 3]
    return ct


@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_expand_words_log4(S, name):
    """BFV STRICT with one special prime; CKKS with two and a short last digit (five ciphertext primes)"""
    scheme, bits, nsp, t = CASES_16[name]
    s = Session(S, scheme, 4, bits, nsp, t=t, seed=16)
    for k in (s.kf, 1):
        for n in (1, 2, 4, 16):
            for normalize in (False, True):
                s.compare(k, 2, n, normalize, name)
    for normalize in (False, True):
        s.compare(s.kf, 2, 16, normalize, name + " planted", ct=planted(s, s.kf, 2))


def test_expand_words_ckks_parity(S):
    """the fork's mode: the same comparison on a PARITY context (both sides)"""
    s = Session(S, 2, 4, [40] * 5 + [41] * 2, 2, seed=17, mode=S.MODE_PARITY)
    for k in (s.kf, 1):
        for n in (1, 2, 4, 16):
            for normalize in (False, True):
                s.compare(k, 2, n, normalize, "ckks parity")


@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_expand_words_log3(S, name):
    """n = N = 8: four pairs per row, less than one wavefront, and the last step's shift is N / 2"""
    scheme, bits, nsp, t = {"bfv": (1, [30, 40, 41], 1, 257), "ckks": (2, [40, 40, 41], 1, 0)}[name]
    s = Session(S, scheme, 3, bits, nsp, t=t, seed=3)
    s.compare(s.kf, 1, 8, True, name)
    s.compare(s.kf, 3, 8, False, name + " planted", ct=planted(s, s.kf, 3))


@pytest.mark.parametrize("name,scheme,bits,nsp,t", [("bfv nsp 3", 1, [40] * 4 + [41] * 3, 3, 65537),
                                                   ("ckks", 2, [40, 40, 40, 41], 1, 0)])
def test_expand_words_log12(S, name, scheme, bits, nsp, t):
    """n = 8, two items: several workgroups per row in both kernel forms"""
    s = Session(S, scheme, 12, bits, nsp, t=t, seed=12)
    s.compare(s.kf, 2, 8, True, name)


@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_semantic_run(S, name):
    """real keys at log N = 4: expand(n = 16, normalize) on the device, decrypted by the device Decryptor: output i is the
    constant m[i] -- exactly for BFV, within X.CKKS_REL_BOUND for CKKS"""
    scheme, bits, nsp, t = CASES_16[name]
    N = 16
    s = Session(S, scheme, 4, bits, nsp, t=t, seed=5 if scheme == 2 else 3, client=True)
    cl, ctx, k = s.cl, s.ctx, s.kf
    sk = ctx.upload(cl.sk_powers(1))
    rng = np.random.default_rng(28)
    if scheme == 1:
        m = rng.integers(0, t, size=N, dtype=np.uint64)
        ct = cl.encrypt_bfv(m)[None]
    else:
        m = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
        ct = cl.encrypt_poly_ntt(m)[None]
    out = ctx.alloc(N * 2 * k * N)
    s.ev.expand(ctx.upload(ct), k, 1, N, s.dkeys, out, normalize=True)
    words = out.download((N, 2, k, N))
    assert np.array_equal(words, X.expand(s.ref, s.mods, k, ct[0], s.keys, N, True))
    if scheme == 1:
        plain = ctx.alloc(N * N)
        ctx.decrypt(out, 2, k, N, sk, False, plain)
        got = plain.download((N, N))
        for i in range(N):
            assert got[i].tolist() == [int(m[i])] + [0] * (N - 1), i
    else:
        plain = ctx.alloc(N * k * N)
        ctx.decrypt(out, 2, k, N, sk, True, plain)
        got = plain.download((N, k, N))
        worst = 0
        for i in range(N):
            phase, _ = cl.centered_from_ntt_rows(got[i])
            assert phase == R.ckks_phase(cl, words[i])
            worst = max(worst, max(abs(a - b) for a, b in zip(phase, [m[i]] + [0] * (N - 1))))
        rel = worst / max(abs(v) for v in m)
        print("ckks device n=16: relative error 2^%.1f" % (np.log2(rel) if rel else -np.inf))
        assert rel <= X.CKKS_REL_BOUND, rel


@pytest.mark.parametrize("scheme", [1, 2])
def test_pack_then_expand_round_trip(S, scheme):
    """extract_lwe -> pack_lwes(n = N, normalize) -> expand(n = N, normalize) -> decrypt, all on the device with real keys:
    output i's constant coefficient is m[idx[i]]"""
    logn, N = 4, 16
    if scheme == 1:
        s = Session(S, 1, logn, [40, 40, 41], 1, t=257, seed=3, client=True)
    else:
        s = Session(S, 2, logn, [50, 50, 51, 51], 2, seed=5, client=True)
    cl, ctx, k = s.cl, s.ctx, s.kf
    pack_keys = {g: S.KSwitchKeys(ctx, cl.galois_key(g)) for g in ctx.pack_lwes_galois_elts(N)}
    sk = ctx.upload(cl.sk_powers(1))
    rng = np.random.default_rng(7)
    idx = [int(v) for v in rng.permutation(N)]
    if scheme == 1:
        m = rng.integers(0, 257, size=N, dtype=np.uint64)
        ct = cl.encrypt_bfv(m)
    else:
        m = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
        ct = cl.encrypt_poly_ntt(m)
    la, lb, packed, out = ctx.alloc(N * k * N), ctx.alloc(N * k), ctx.alloc(2 * k * N), ctx.alloc(N * 2 * k * N)
    s.ev.extract_lwe(ctx.upload(ct), k, 1, idx, la, lb)
    s.ev.pack_lwes(la, lb, k, N, 1, pack_keys, packed, normalize=True)
    s.ev.expand(packed, k, 1, N, s.dkeys, out, normalize=True)
    if scheme == 1:
        plain = ctx.alloc(N * N)
        ctx.decrypt(out, 2, k, N, sk, False, plain)
        got = plain.download((N, N))
        assert got[:, 0].tolist() == [int(m[i]) for i in idx]
        assert not got[:, 1:].any()
    else:
        plain = ctx.alloc(N * k * N)
        ctx.decrypt(out, 2, k, N, sk, True, plain)
        got = plain.download((N, k, N))
        worst = 0
        for i in range(N):
            phase, _ = cl.centered_from_ntt_rows(got[i])
            worst = max(worst, max(abs(a - b) for a, b in zip(phase, [m[idx[i]]] + [0] * (N - 1))))
        rel = worst / max(abs(v) for v in m)
        print("ckks device round trip: relative error 2^%.1f" % (np.log2(rel) if rel else -np.inf))
        assert rel <= X.CKKS_REL_BOUND + R.CKKS_REL_BOUND, rel  # (each map within its own bound)


def test_refusals_and_flags(S):
    """the empty batch; BFV PARITY; a missing key; a key with too few digits; an even element; overlap; the transparency
    flags from the last key switch and from the read pass"""
    logn, n = 8, 256
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    rng = np.random.default_rng(1)
    k = 3
    key = rows(rng, mods, n, (3, 2))
    parity = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, mode=S.MODE_PARITY)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    dkey, short = S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, key[:2])
    ct_h = rows(rng, mods[:k], n, (3, 2))
    ct_h[1, 1] = 0  # item 1: c_1 is zero, so every target and every output's c_1 is zero -- transparent
    ct = ctx.upload(ct_h)
    out = ctx.alloc(3 * 4 * 2 * k * n)
    sentinel = np.full(out.words, 7, dtype=np.uint64)
    out.upload(sentinel)
    good = {257: dkey, 129: dkey}  # n = 4: N + 1 and N / 2 + 1
    with pytest.raises(ValueError, match="STRICT"):
        pkey = S.KSwitchKeys(parity, key)
        S.Evaluator(parity).expand(parity.upload(ct_h), k, 3, 4, {257: pkey, 129: pkey}, parity.alloc(out.words))
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.expand(ct, k, 3, 4, {257: dkey}, out)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.expand(ct, k, 3, 4, {129: dkey, 3: dkey, 5: dkey}, out)
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        ev.expand(ct, k, 3, 4, {257: dkey, 129: short}, out)
    with pytest.raises(ValueError, match="Galois element is not valid"):
        ev.expand(ct, k, 3, 4, {257: dkey, 129: dkey, 6: dkey}, out)
    with pytest.raises(ValueError, match="Galois element is not valid"):
        ev.expand(ct, k, 3, 4, {257: dkey, 129: dkey, 513: dkey}, out)
    with pytest.raises(ValueError, match="overlap"):
        ev.expand(ct, k, 3, 4, good, ct)
    with pytest.raises(ValueError, match="overlap"):
        ev.expand(out.ptr + 16, k, 3, 4, good, out)
    ev.expand(ct, k, 0, 4, good, out)  # the empty batch
    assert np.array_equal(out.download(), sentinel) and np.array_equal(ct.download(ct_h.shape), ct_h)
    ev.expand(ct, 2, 3, 4, {257: dkey, 129: short}, out)  # (two digits are enough one level below)
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        for n_out, keys in ((4, good), (1, {})):
            flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
            ev.expand(ct, k, 3, n_out, keys, out)
            got = flags.download().view(np.uint32)
            want = [True] * n_out + [False] * n_out + [True] * n_out
            assert (got[:3 * n_out] != 0).tolist() == want and np.all(got[3 * n_out:] == 5), (n_out, got)
        ctx.transparency_sink(flags, 11)
        with pytest.raises(ValueError, match="sink"):
            ev.expand(ct, k, 3, 4, good, out)
    finally:
        ctx.transparency_sink(None, 0)


# ---------------------------------------------------------------- sums against plaintext rows
CHAINS = {"61": [61, 61, 61, 61], "mixed": [61, 20, 45, 61]}
_dot_sessions = {}


def dot_session(S, chain, logn):
    key = (chain, logn)
    if key not in _dot_sessions:
        _dot_sessions[key] = BaseSession(S, 2, logn, CHAINS[chain], 1, 1, 0, 100 + logn)
    return _dot_sessions[key]


def run_dot(s, k, cts, plain, both=True):
    """the device's sums against both restatements; returns the transparency flags (n_sums x count)"""
    count, n_terms, size = cts.shape[:3]
    n_sums = plain.shape[0]
    words = n_sums * count * size * k * s.n
    out = s.ctx.alloc(words + 4)
    out.upload(np.full(words + 4, SENTINEL, dtype=np.uint64))
    dc, dp = s.ctx.upload(cts), s.ctx.upload(plain)
    flags = s.ctx.alloc((n_sums * count + 3) // 2 + 1)
    flags.upload(np.full(flags.words, 0x0000000500000005, dtype=np.uint64))
    s.ctx.transparency_sink(flags, n_sums * count)
    try:
        s.ev.dot_plain(dc, dp, k, count, n_terms, n_sums, out, size=size)
    finally:
        s.ctx.transparency_sink(None, 0)
    got = out.download()
    assert np.all(got[words:] == SENTINEL), "words behind out were written"
    assert np.array_equal(dc.download(cts.shape), cts) and np.array_equal(dp.download(plain.shape), plain)
    got = got[:words].reshape((n_sums, count, size, k, s.n))
    tag = ("N", s.n, "terms", n_terms, "sums", n_sums, "size", size, "count", count)
    assert np.array_equal(got, X.dot_plain(s.ref, k, cts, plain)), tag
    if both:
        assert np.array_equal(got, X.dot_plain_int(s.mods, cts, plain)), tag
    seen = flags.download().view(np.uint32)
    assert np.all(seen[n_sums * count:] == 5), tag
    return seen[:n_sums * count].reshape(n_sums, count) != 0


@pytest.mark.parametrize("chain", ["61", "mixed"])
def test_dot_plain_words_small_ring(S, chain):
    """N = 8: every group edge against every tile edge, both sizes and both batch lengths"""
    s = dot_session(S, chain, 3)
    k = s.k_first
    for n_terms in (1, 16, 17, 33):
        for n_sums in (1, 4, 5):
            for size, count in ((2, 1), (3, 3)):
                cts = rows(s.rng, s.mods[:k], s.n, (count, n_terms, size))
                plain = rows(s.rng, s.mods[:k], s.n, (n_sums, n_terms))
                assert run_dot(s, k, cts, plain).all()


@pytest.mark.parametrize("logn", [8, 9, 10, 12])
@pytest.mark.parametrize("chain", ["61", "mixed"])
def test_dot_plain_words(S, chain, logn):
    """N = 2^8 and 2^9 (a block straddles rows), 2^10 and 2^12 (a block inside one row); at level 1 too"""
    s = dot_session(S, chain, logn)
    k = s.k_first
    shapes = ((17, 5, 3, 3, k), (33, 4, 2, 1, 1)) if logn < 12 else ((17, 5, 2, 1, k), (33, 1, 3, 3, 1))
    for n_terms, n_sums, size, count, kk in shapes:
        cts = rows(s.rng, s.mods[:kk], s.n, (count, n_terms, size))
        plain = rows(s.rng, s.mods[:kk], s.n, (n_sums, n_terms))
        assert run_dot(s, kk, cts, plain).all()


@pytest.mark.parametrize("logn", [3, 10])
@pytest.mark.parametrize("chain", ["61", "mixed"])
def test_dot_plain_extreme_words(S, chain, logn):
    """every word p - 1 at 33 terms: the largest integer sum the kernel can see (two full groups and the partial sum);
    every word 0: the transparency flags stay clear; one item with c_1 = 0 alone clears its own flags"""
    s = dot_session(S, chain, logn)
    k = s.k_first
    n_terms, n_sums, size, count = 33, 5, 2, 2
    cts, plain = top(s.mods[:k], s.n, (count, n_terms, size)), top(s.mods[:k], s.n, (n_sums, n_terms))
    assert run_dot(s, k, cts, plain, both=logn == 3).all()
    assert not run_dot(s, k, np.zeros_like(cts), plain, both=False).any()
    assert not run_dot(s, k, cts, np.zeros_like(plain), both=False).any()
    cts[1, :, 1:] = 0
    flags = run_dot(s, k, cts, plain, both=False)
    assert flags[:, 0].all() and not flags[:, 1].any()


def test_dot_plain_refusals(S):
    s = dot_session(S, "mixed", 3)
    k, n = s.k_first, s.n
    cts = s.ctx.upload(rows(s.rng, s.mods[:k], n, (2, 3, 2)))
    plain = s.ctx.upload(rows(s.rng, s.mods[:k], n, (2, 3)))
    out = s.ctx.alloc(2 * 2 * 2 * k * n)
    sentinel = np.full(out.words, 7, dtype=np.uint64)
    out.upload(sentinel)
    with pytest.raises(ValueError, match="level k out of range"):
        s.ev.dot_plain(cts, plain, k + 1, 2, 3, 2, out)
    with pytest.raises(ValueError, match="encrypted is not valid"):
        s.ev.dot_plain(cts, plain, k, 2, 3, 2, out, size=1)
    with pytest.raises(ValueError, match="must not be empty"):
        s.ev.dot_plain(cts, plain, k, 2, 0, 2, out)
    with pytest.raises(ValueError, match="16-byte aligned"):
        s.ev.dot_plain(cts.ptr + 8, plain, k, 1, 3, 2, out)
    with pytest.raises(ValueError, match="overlap cts"):
        s.ev.dot_plain(cts, plain, k, 2, 3, 2, cts.ptr + 16)
    with pytest.raises(ValueError, match="overlap plain"):
        s.ev.dot_plain(cts, plain, k, 2, 3, 1, plain)
    s.ev.dot_plain(cts, plain, k, 0, 3, 2, out)  # the empty batch
    assert np.array_equal(out.download(), sentinel)
    s.ctx.transparency_sink(s.ctx.alloc(2), 3)
    try:
        with pytest.raises(ValueError, match="sink"):
            s.ev.dot_plain(cts, plain, k, 2, 3, 2, out)
    finally:
        s.ctx.transparency_sink(None, 0)
    assert np.array_equal(out.download(), sentinel)


def test_pir_run(S):
    """BFV STRICT, log N = 4: the query Delta X^idx, expanded into 16 with the normalisation, transformed, summed against
    a 2 x 16 table of batch-encoded plaintexts, transformed back and decrypted: row s gives db[s][idx], exactly"""
    scheme, bits, nsp, t = CASES_16["bfv"]
    N, n_sums = 16, 2
    s = Session(S, scheme, 4, bits, nsp, t=t, seed=3, client=True)
    cl, ctx, k = s.cl, s.ctx, s.kf
    rng = np.random.default_rng(31)
    db = rng.integers(0, t, size=(n_sums, N, N), dtype=np.uint64)  # db[s][i]: the N slot values of entry i of row s
    encoded = ctx.alloc(n_sums * N * N)
    ctx.batch_encode(ctx.upload(db), N, n_sums * N, encoded)
    plain_ntt = ctx.alloc(n_sums * N * k * N)
    s.ev.transform_plain_to_ntt(encoded, N, k, n_sums * N, plain_ntt)
    sk = ctx.upload(cl.sk_powers(1))
    for idx in (0, 5, 15):
        query = np.zeros(N, dtype=np.uint64)
        query[idx] = 1
        expanded = ctx.alloc(N * 2 * k * N)
        s.ev.expand(ctx.upload(cl.encrypt_bfv(query)), k, 1, N, s.dkeys, expanded, normalize=True)
        s.ev.transform_to_ntt_inplace(expanded, 2, k, N)
        sums = ctx.alloc(n_sums * 2 * k * N)
        s.ev.dot_plain(expanded, plain_ntt, k, 1, N, n_sums, sums)
        s.ev.transform_from_ntt_inplace(sums, 2, k, n_sums)
        plain = ctx.alloc(n_sums * N)
        ctx.decrypt(sums, 2, k, n_sums, sk, False, plain)
        assert np.array_equal(plain.download((n_sums, N)), encoded.download((n_sums, N, N))[:, idx]), idx
        values = ctx.alloc(n_sums * N)
        ctx.batch_decode(plain, n_sums, values)
        assert np.array_equal(values.download((n_sums, N)), db[:, idx]), idx


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_expand_check.cpp: Evaluator::expand and dot_plain on resident operands give the ABI's words on
    the same seeded inputs, with the operands' metadata; the ABI's refusals arrive as std::invalid_argument"""
    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_expand_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    sm = O.SplitMix(0x28E4A)
    ct = sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n)
    keys = [sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n) for _ in range(2)]
    plains = np.stack([sm.fill(k, n, mods[:k]) for _ in range(8)]).reshape(2, 4, k, n)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    gk = {g: S.KSwitchKeys(ctx, key) for g, key in zip((2049, 4097), keys)}
    out, sums = ctx.alloc(4 * 2 * k * n), ctx.alloc(2 * 2 * k * n)
    ev.expand(ctx.upload(ct), k, 1, 4, gk, out, normalize=True)
    ev.dot_plain(out, ctx.upload(plains), k, 1, 4, 2, sums)
    for name, words in (("expand", out.download()), ("dot_plain", sums.download())):
        line = "device %s digest %016x meta 1" % (name, O.fnv(words))
        assert line in stdout, (line, stdout)
    assert "refusals ok" in stdout, stdout


# ---------------------------------------------------------------- arena chunks (a child process with the smallest arena)
WALK = dict(scheme=2, logn=9, bits=[40] * 7 + [41], nsp=1, seed=65)  # N = n = 2^9, k = 7


def _walk_case(S):
    """seeded, so that the parent (default arena) and the child (smallest arena) expand the same ciphertext under the same
    keys"""
    s = Session(S, WALK["scheme"], WALK["logn"], WALK["bits"], WALK["nsp"], seed=WALK["seed"])
    return s, rows(s.rng, s.mods[:s.kf], s.n, (1, 2))


def _child():
    """Items: N = n = 2^8, k = 2: ciphertexts of 8 KiB; an item's working set is 2.5 MiB (128 + 64 ciphertexts and 256
    targets of 4 KiB), so half of the 64 MiB arena takes 12 items and 14 items need a second, ragged chunk. The words must
    be those of fourteen calls of one item, which are not chunked; two items are also held to the restatement; the
    transparency flags of the second chunk land behind the first's (item 13 has c_1 = 0, item 12 has not).
    One item over its last step: N = n = 2^9, k = 7: ciphertexts of 56 KiB, 1.25 n of them are 35 MiB; with c sources at a
    time the buffers hold 0.75 n ciphertexts and max(n / 2, 2 c) targets of 28 KiB -- 28 MiB at c = 128, so two groups. The
    parent compares the digest with the unwalked run.
    Refusal: N = n = 2^12, k = 3: the smallest working set (n ciphertexts of 192 KiB) is 768 MiB."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    s = Session(S, 2, 8, [40, 40, 41], 1, seed=64)
    k, n, count = 2, 256, 14
    ct = rows(s.rng, s.mods[:k], n, (count, 2))
    ct[13, 1] = 0
    flags = s.ctx.alloc(count * n // 2 + 2)
    s.ctx.transparency_sink(flags, count * n + 4)
    flags.upload(np.full(flags.words, 0x0000000500000005, dtype=np.uint64))
    s.ctx.chunk_log()
    got = s.expand(ct, k, n, True)
    log = s.ctx.chunk_log()
    seen = flags.download().view(np.uint32)
    s.ctx.transparency_sink(None, 0)
    assert log[-1] == (count, 12), log[-4:]
    assert np.all(seen[:13 * n] != 0) and not seen[13 * n:14 * n].any() and np.all(seen[14 * n:] == 5), seen
    for c in range(count):
        one = s.expand(ct[c:c + 1], k, n, True)
        assert s.ctx.chunk_log()[-1] == (1, 1)
        assert np.array_equal(got[c], one[0]), c
    for c in (0, 13):
        assert np.array_equal(got[c], X.expand(s.ref, s.mods, k, ct[c], s.keys, n, True)), c

    w, ct = _walk_case(S)
    w.ctx.chunk_log()
    got = w.expand(ct, w.kf, w.n, True)
    log = w.ctx.chunk_log()
    assert log[-2:] == [(256, 128), (1, 1)], log[-4:]

    big = Session(S, 1, 12, [40, 40, 40, 41], 1, t=65537, seed=66)
    out = big.ctx.alloc(4096 * 2 * 3 * 4096)
    with pytest.raises(MemoryError, match="smallest working set of one item .805306368 bytes. does not fit half"):
        big.ev.expand(big.ctx.alloc(2 * 3 * 4096), 3, 1, 4096, big.dkeys, out)
    print("EXPAND_CHUNKS_OK walk %016x" % O.fnv(got))


def test_chunked_items_and_walked_last_step(S):
    """the child's three cases; the walked expansion's words are those of this process, whose arena holds the whole item"""
    w, ct = _walk_case(S)
    w.ctx.chunk_log()
    want = w.expand(ct, w.kf, w.n, True)
    assert w.ctx.chunk_log()[-1] == (1, 1)
    run_arena_child(__file__, "EXPAND_CHUNKS_OK walk %016x" % O.fnv(want), timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
