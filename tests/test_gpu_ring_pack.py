"""Ring packing on the device (sealhip_evaluator_extract_lwe / _pack_lwes) against the CPU
restatement of tests/ring_pack_ref.py, word for word.

Shapes: the smallest that reach every path. Extraction at N = 2^3 (less than one wavefront of pairs), 2^8 and 2^12 (several
workgroups per row batch), one item and three, with 0, 1 and p - 1 planted where the sign split reads. The pack at N = 2^4
runs every n, both levels, all four normalize / trace combinations (the trace-only step, the merge step, the embedding
alone; random keys: a word comparison needs no valid ones); at N = 2^12 several workgroups per row in both kernel forms.
The chunked walk runs in a child process under the smallest arena."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import ring_pack_ref as R
from support import ARENA_MB, S, child_main, compile_cpp, rows, run_arena_child, run_exe

pytestmark = pytest.mark.gpu
SENTINEL = 0x5E5E5E5E5E5E5E5E


class Session:
    """contexts on both sides, random keys for every element of the trace (host arrays and device handles)"""

    def __init__(self, S, scheme, logn, bits, nsp, t=0, seed=0, client=False, mode=1):
        self.S, self.logn, self.n = S, logn, 1 << logn
        self.mods = O.coeff_modulus_create(self.n, bits)
        self.ctx = S.Context(scheme, logn, self.mods, nsp, t, mode=mode)
        self.ref = O.RefContext(scheme, logn, self.mods, nsp=nsp, t=t, mode=mode)
        self.ev = S.Evaluator(self.ctx)
        self.rng = np.random.default_rng(seed + logn)
        self.kf = len(self.mods) - nsp
        nd = (self.kf + nsp - 1) // nsp
        elts = R.galois_elts(logn, self.n, True)
        assert self.ctx.pack_lwes_galois_elts(self.n, True) == elts
        if client:
            self.cl = O.Client(self.ref, seed=seed + 1)
            self.keys = {g: self.cl.galois_key(g) for g in elts}
        else:
            self.keys = {g: rows(self.rng, self.mods, self.n, (nd, 2)) for g in elts}
        self.dkeys = {g: S.KSwitchKeys(self.ctx, key) for g, key in self.keys.items()}

    def pack(self, la, lb, k, trace, normalize):
        count, n = la.shape[:2]
        out = self.ctx.alloc(count * 2 * k * self.n)
        da, db = self.ctx.upload(la), self.ctx.upload(lb)
        self.ev.pack_lwes(da, db, k, n, count, self.dkeys, out, trace=trace, normalize=normalize)
        got = out.download((count, 2, k, self.n))
        assert np.array_equal(da.download(la.shape), la) and np.array_equal(db.download(lb.shape), lb)
        return got

    def samples(self, k, count, n):
        return rows(self.rng, self.mods[:k], self.n, (count, n)), \
            np.ascontiguousarray(rows(self.rng, self.mods[:k], 1, (count, n))[..., 0])

    def compare(self, k, count, n, trace, normalize, tag):
        la, lb = self.samples(k, count, n)
        got = self.pack(la, lb, k, trace, normalize)
        want = R.pack_batch(self.ref, self.mods, k, la, lb, self.keys, trace, normalize)
        for c in range(count):
            assert np.array_equal(got[c], want[c]), (tag, "k", k, "n", n, "trace", trace, "normalize", normalize, "item", c)


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("logn", [3, 8, 12])
def test_extraction_words(S, scheme, logn):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [30, 45, 61, 50])
    t = 65537 if scheme == 1 else 0
    ctx = S.Context(scheme, logn, mods, 1, t, mode=S.MODE_STRICT)
    ref = O.RefContext(scheme, logn, mods, nsp=1, t=t, mode=1)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(logn)
    idx = [0, 1, n // 2, n - 1, 1]
    for k, count in ((3, 1), (3, 3), (1, 3)):
        coeff = rows(rng, mods[:k], n, (count, 2))
        plant = [0, 1, None]  # (None: p - 1)
        for c in range(count):
            for r in range(k):
                for s, pos in enumerate((0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1)):
                    v = plant[(c + r + s) % 3]
                    coeff[c, 1, r, pos] = mods[r] - 1 if v is None else v
        ct = R.transform(ref, coeff) if scheme == 2 else coeff
        assert np.array_equal(R.transform(ref, ct, inverse=True), coeff) or scheme == 1
        want_a, want_b = R.extract_samples(ref, mods, ct, idx)
        d = ctx.upload(ct)
        da, db = ctx.alloc(want_a.size + 4), ctx.alloc(want_b.size + 4)
        da.upload(np.full(da.words, SENTINEL, dtype=np.uint64))
        db.upload(np.full(db.words, SENTINEL, dtype=np.uint64))
        ev.extract_lwe(d, k, count, idx, da, db)
        ga, gb = da.download(), db.download()
        assert np.array_equal(ga[:-4].reshape(want_a.shape), want_a), (scheme, logn, k, count)
        assert np.array_equal(gb[:-4].reshape(want_b.shape), want_b), (scheme, logn, k, count)
        assert np.all(ga[-4:] == SENTINEL) and np.all(gb[-4:] == SENTINEL)
        assert np.array_equal(d.download(ct.shape), ct), "the input was modified"


CASES_16 = {"bfv": (1, [30, 35, 40, 45, 50], 1, 65537), "ckks": (2, [40] * 5 + [41] * 2, 2, 0)}


@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_pack_words_log4(S, name):
    """BFV STRICT with one special prime; CKKS with two and a short last digit (five ciphertext primes)"""
    scheme, bits, nsp, t = CASES_16[name]
    s = Session(S, scheme, 4, bits, nsp, t=t, seed=16)
    for k in (s.kf, 1):
        for n in (1, 2, 4, 16):
            for trace in (False, True):
                for normalize in (False, True):
                    s.compare(k, 2, n, trace, normalize, name)


def test_pack_words_ckks_parity(S):
    """the fork's mode: the same comparison on a PARITY context (both sides), every n, with and without the trace"""
    s = Session(S, 2, 4, [40] * 5 + [41] * 2, 2, seed=17, mode=S.MODE_PARITY)
    for k in (s.kf, 1):
        for n in (1, 2, 4, 16):
            for trace in (False, True):
                s.compare(k, 2, n, trace, True, "ckks parity")


@pytest.mark.parametrize("name,scheme,bits,nsp,t", [("bfv nsp 3", 1, [40] * 4 + [41] * 3, 3, 65537),
                                                   ("ckks", 2, [40, 40, 40, 41], 1, 0)])
def test_pack_words_log12(S, name, scheme, bits, nsp, t):
    """n = 8 with the trace: 7 merges and 9 trace steps per item"""
    s = Session(S, scheme, 12, bits, nsp, t=t, seed=12)
    s.compare(s.kf, 2, 8, True, True, name)


@pytest.mark.parametrize("scheme", [1, 2])
def test_semantic_run(S, scheme):
    """real keys at log N = 4: extract -> pack (normalize, trace) on the device, decrypted by the device Decryptor, is
    m[idx[j]] at (N / n) j and 0 elsewhere -- exactly for BFV, within R.CKKS_REL_BOUND for CKKS"""
    logn, N = 4, 16
    if scheme == 1:
        s = Session(S, 1, logn, [40, 40, 41], 1, t=257, seed=3, client=True)
    else:
        s = Session(S, 2, logn, [50, 50, 51, 51], 2, seed=5, client=True)
    cl, ctx, k = s.cl, s.ctx, s.kf
    sk = ctx.upload(cl.sk_powers(1))
    for n in (1, 2, 4, 16):
        rng = np.random.default_rng(n)
        idx = [int(v) for v in rng.permutation(N)[:n]]
        if scheme == 1:
            m = rng.integers(0, 257, size=N, dtype=np.uint64)
            ct = cl.encrypt_bfv(m)[None]
        else:
            m = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
            ct = cl.encrypt_poly_ntt(m)[None]
        la, lb = ctx.alloc(n * k * N), ctx.alloc(n * k)
        s.ev.extract_lwe(ctx.upload(ct), k, 1, idx, la, lb)
        out = ctx.alloc(2 * k * N)
        s.ev.pack_lwes(la, lb, k, n, 1, s.dkeys, out, trace=True, normalize=True)
        want_words = R.pack(s.ref, s.mods, k, *[x[0] for x in R.extract_samples(s.ref, s.mods, ct, idx)], s.keys, True, True)
        assert np.array_equal(out.download((2, k, N)), want_words)
        want = [0] * N
        for j, i in enumerate(idx):
            want[(N // n) * j] = int(m[i])
        if scheme == 1:
            plain = ctx.alloc(N)
            ctx.decrypt(out, 2, k, 1, sk, False, plain)
            assert plain.download().tolist() == want, (n, idx)
        else:
            plain = ctx.alloc(k * N)
            ctx.decrypt(out, 2, k, 1, sk, True, plain)
            got, _ = cl.centered_from_ntt_rows(plain.download((k, N)))
            assert got == R.ckks_phase(cl, out.download((2, k, N)))
            rel = max(abs(a - b) for a, b in zip(got, want)) / max(abs(v) for v in m)
            print("ckks device n=%d: relative error 2^%.1f" % (n, np.log2(rel) if rel else -np.inf))
            assert rel <= R.CKKS_REL_BOUND, (n, rel)


def test_refusals_and_flags(S):
    """the empty batch; BFV PARITY; a missing key; a key with too few digits; overlap; the transparency flags"""
    logn, n = 8, 256
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    rng = np.random.default_rng(1)
    k = 3
    key = rows(rng, mods, n, (3, 2))
    parity = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, mode=S.MODE_PARITY)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    dkey, short = S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, key[:2])
    la_h = rows(rng, mods[:k], n, (3, 4))
    lb_h = np.ascontiguousarray(rows(rng, mods[:k], 1, (3, 4))[..., 0])
    la_h[1] = 0  # item 1: every a is zero, so c_1 of its pack is zero -- transparent
    la, lb = ctx.upload(la_h), ctx.upload(lb_h)
    out = ctx.alloc(3 * 2 * k * n)
    sentinel = np.full(out.words, 7, dtype=np.uint64)
    out.upload(sentinel)
    with pytest.raises(ValueError, match="STRICT"):
        pkey = S.KSwitchKeys(parity, key)
        S.Evaluator(parity).pack_lwes(parity.upload(la_h), parity.upload(lb_h), k, 4, 3, {3: pkey, 5: pkey}, parity.alloc(out.words))
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.pack_lwes(la, lb, k, 4, 3, {3: dkey}, out)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.pack_lwes(la, lb, k, 4, 3, {3: dkey, 5: dkey}, out, trace=True)
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        ev.pack_lwes(la, lb, k, 4, 3, {3: dkey, 5: short}, out)
    with pytest.raises(ValueError, match="Galois element is not valid"):
        ev.pack_lwes(la, lb, k, 4, 3, {3: dkey, 5: dkey, 6: dkey}, out)
    with pytest.raises(ValueError, match="overlap"):
        ev.pack_lwes(la, lb, k, 4, 3, {3: dkey, 5: dkey}, la)
    with pytest.raises(ValueError, match="overlap"):
        ev.pack_lwes(la, lb.ptr, k, 4, 3, {3: dkey, 5: dkey}, lb.ptr - 16)
    with pytest.raises(ValueError, match="overlap"):
        ev.extract_lwe(out, k, 3, [1, 2], out, lb)
    ev.pack_lwes(la, lb, k, 4, 0, {3: dkey, 5: dkey}, out)   # the empty batch
    ev.extract_lwe(out, k, 0, [1, 2], la, lb)
    ev.extract_lwe(out, k, 3, [], la, lb)
    assert np.array_equal(out.download(), sentinel) and np.array_equal(la.download(la_h.shape), la_h)
    ev.pack_lwes(la, lb, 2, 4, 3, {3: dkey, 5: short}, out)  # (two digits are enough one level below)
    flags = ctx.alloc(4)  # 8 uint32 words
    ctx.transparency_sink(flags, 8)
    try:
        for n_pack, count, keys, want in ((4, 3, {3: dkey, 5: dkey}, [True, False, True]), (1, 3, {}, [True, False, True])):
            flags.upload(np.full(4, 0x0000000500000005, dtype=np.uint64))
            a = ctx.upload(la_h[:, :n_pack])
            b = ctx.upload(lb_h[:, :n_pack])
            ev.pack_lwes(a, b, k, n_pack, count, keys, out)
            got = flags.download().view(np.uint32)
            assert (got[:3] != 0).tolist() == want and np.all(got[3:] == 5), (n_pack, got)
        ctx.transparency_sink(flags, 2)
        with pytest.raises(ValueError, match="sink"):
            ev.pack_lwes(la, lb, k, 4, 3, {3: dkey, 5: dkey}, out)
    finally:
        ctx.transparency_sink(None, 0)


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_ring_pack_check.cpp: LweSamples and the DeviceCiphertext methods give the ABI's words on the same
    seeded inputs, with the operand's metadata; the ABI's refusals arrive as std::invalid_argument"""
    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_ring_pack_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    sm = O.SplitMix(0x27ACC)
    ct = sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n)
    keys = [sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n) for _ in range(2)]
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    gk = {g: S.KSwitchKeys(ctx, key) for g, key in zip((3, 5), keys)}
    la, lb, out = ctx.alloc(4 * k * n), ctx.alloc(4 * k), ctx.alloc(2 * k * n)
    ev.extract_lwe(ctx.upload(ct), k, 1, [7, 0, 4095, 7], la, lb)
    ev.pack_lwes(la, lb, k, 4, 1, gk, out, normalize=True)
    for name, words in (("extract_lwe", np.concatenate([la.download(), lb.download()])), ("pack_lwes", out.download())):
        line = "device %s digest %016x meta 1" % (name, O.fnv(words))
        assert line in stdout, (line, stdout)
    assert "refusals ok" in stdout, stdout


# ---------------------------------------------------------------- arena chunks (a child process with the smallest arena)
WALK = dict(scheme=2, logn=10, bits=[40, 40, 41], nsp=1, seed=65)  # N = n = 2^10, k = 2


def _walk_case(S):
    """seeded, so that the parent (default arena) and the child (smallest arena) pack the same samples under the same keys"""
    s = Session(S, WALK["scheme"], WALK["logn"], WALK["bits"], WALK["nsp"], seed=WALK["seed"])
    la, lb = s.samples(2, 2, s.n)
    return s, la, lb


def _child():
    """Items: N = 2^8, n = N, k = 2: an item's working set is 3.5 MiB (256 + 128 ciphertexts of 8 KiB and 128 targets of
    4 KiB), so half of the 64 MiB arena takes 9 items and 11 items need a second, ragged chunk. The words must be those of
    eleven calls of one item, which are not chunked; two items are also held to the restatement; the transparency flags of
    the second chunk land behind the first's (item 10 has c_1 = 0).
    One item over its samples: N = n = 2^10, k = 2: ciphertexts of 32 KiB, 1.75 n of them are 56 MiB, so the first step is
    walked in groups: with c merges at a time the buffers hold max(2 c, n / 4) + n / 2 ciphertexts and max(c, n / 4)
    targets -- 36 MiB at c = 256, 28 MiB at c = 128, so four groups. The parent compares the digest with the unwalked run.
    Refusal: N = n = 2^12, k = 3: the smallest working set (0.875 n ciphertexts of 192 KiB) is 672 MiB."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    s = Session(S, 2, 8, [40, 40, 41], 1, seed=64)
    k, n, count = 2, 256, 11
    la, lb = s.samples(k, count, n)
    la[10] = 0
    flags = s.ctx.alloc(8)  # 16 uint32 words
    s.ctx.transparency_sink(flags, 16)
    flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
    s.ctx.chunk_log()
    got = s.pack(la, lb, k, False, True)
    log = s.ctx.chunk_log()
    seen = flags.download().view(np.uint32)
    s.ctx.transparency_sink(None, 0)
    assert log[-1] == (count, 9), log[-4:]
    assert (seen[:11] != 0).tolist() == [True] * 10 + [False] and np.all(seen[11:] == 5), seen
    for c in range(count):
        one = s.pack(la[c:c + 1], lb[c:c + 1], k, False, True)
        assert s.ctx.chunk_log()[-1] == (1, 1)
        assert np.array_equal(got[c], one[0]), c
    for c in (0, 10):
        assert np.array_equal(got[c], R.pack(s.ref, s.mods, k, la[c], lb[c], s.keys, False, True)), c

    w, la, lb = _walk_case(S)
    w.ctx.chunk_log()
    got = w.pack(la, lb, 2, True, True)
    log = w.ctx.chunk_log()
    assert log[-2:] == [(512, 128), (2, 1)], log[-4:]

    big = Session(S, 1, 12, [40, 40, 40, 41], 1, t=65537, seed=66)
    out = big.ctx.alloc(2 * 3 * 4096)
    with pytest.raises(MemoryError, match="smallest working set of one item .704643072 bytes. does not fit half"):
        big.ev.pack_lwes(big.ctx.alloc(4096 * 3 * 4096), big.ctx.alloc(4096 * 3), 3, 4096, 1, big.dkeys, out)
    print("RING_PACK_CHUNKS_OK walk %016x" % O.fnv(got))


def test_chunked_items_and_walked_samples(S):
    """the child's three cases; the walked pack's words are those of this process, whose arena holds the whole item"""
    w, la, lb = _walk_case(S)
    w.ctx.chunk_log()
    want = w.pack(la, lb, 2, True, True)
    assert w.ctx.chunk_log()[-1] == (2, 2)
    run_arena_child(__file__, "RING_PACK_CHUNKS_OK walk %016x" % O.fnv(want), timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
