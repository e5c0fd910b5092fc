"""Fixed-weight secrets on the device and sparse-secret encapsulation.

1. sealhip_sample_fixed_weight: device = host = the numpy restatement (tests/fixed_weight_ref.py) at N = 2^3 (less than one
   wavefront), 2^8, 2^13 (several tiles and workgroups) and 2^16 (the longest tile loop, the largest grid); the rank kernel
   itself on planted words (sealhip_debug_fixed_weight_map): ties, the extreme words, words that differ in one bit.
2. sealhip_generate_sparse_secret_key against the lifted host sample; sealhip_generate_switching_keys word for word against
   generate_one_kswitch_key restated from oracle entries (tests/test_gpu_keygen.py's Setup.expected with sk = s_to and
   new_key = s_from), with the rows and digits a lower `level` leaves out.
3. sealhip_evaluator_switch_secret against ref_switch_key_inplace on (c_0, 0), and what it decrypts to.
4. sealhip_evaluator_bootstrap_encapsulated end to end with keys the library made, decrypted under the dense secret."""
import ctypes as C

import numpy as np
import pytest

import fixed_weight_ref as F
import hoist_ref as H
import homdft_ref as R
import oracle_lib as O
import sample_ref as SR
from support import S, compile_cpp, rows, run_exe
from test_gpu_keygen import Setup, fnv, wire
from test_sparse_secret_host import bootstrap_mods, primes_next_to

pytestmark = pytest.mark.gpu
T = 786433


# ------------------------------------------------------------------ 1. the sampler
def ring(S, logn):
    n = 1 << logn
    return S.Context(S.SCHEME_CKKS, logn, O.get_primes(n, 30, 2), 1, 0), n


@pytest.mark.parametrize("logn", [3, 8, 13, 16])
def test_sampler_words(S, logn):
    ctx, n = ring(S, logn)
    rng = np.random.default_rng(40 + logn)
    seeds = np.stack([np.zeros(8, dtype=np.uint64), rng.integers(0, 2**64, size=8, dtype=np.uint64),
                      np.full(8, 2**64 - 1, dtype=np.uint64)])
    words = np.stack([SR.stream_words(S, s, n) for s in seeds])
    pad = 12  # a stride of N + 12 words: sentinels behind each item
    for h in (1, n // 2, n):
        want = F.fixed_weight_map(words, h)
        assert np.array_equal(ctx.sample_fixed_weight_host(seeds, h), want), (logn, h)
        for count in (1, 3):
            out = ctx.alloc(count * n // 2)
            ctx.sample_fixed_weight(seeds[:count], h, out)
            got = out.download().view(np.int32).reshape(count, n)
            assert np.array_equal(got, want[:count]), (logn, h, count)
            assert np.all(np.count_nonzero(got, axis=1) == h)
        buf = ctx.upload(np.full(3 * (n + pad) // 2, 0x7777777777777777, dtype=np.uint64))
        ctx.sample_fixed_weight(seeds, h, buf, n + pad)
        got = buf.download().view(np.int32).reshape(3, n + pad)
        assert np.array_equal(got[:, :n], want) and np.all(got[:, n:] == 0x77777777), (logn, h, "stride")
    ctx.sample_fixed_weight(seeds[:0], 1, out)  # the empty batch launches nothing
    with pytest.raises(ValueError, match="1 .. N"):
        ctx.sample_fixed_weight(seeds, n + 1, out)
    with pytest.raises(ValueError, match="aligned"):
        ctx.sample_fixed_weight(seeds[:1], 1, out.ptr + 8)
    ctx.close()


def test_planted_words(S):
    """N = 2^12: four workgroups of 1024 words, one LDS tile each, a lane owns four consecutive words. Every case is one
    polynomial of the batch, compared with the restatement at several weights."""
    ctx, n = ring(S, 12)
    rng = np.random.default_rng(5)
    top = 2**64 - 1
    cases = {}
    cases["all equal"] = np.full(n, 0x1234567812345679, dtype=np.uint64)
    w = rng.integers(1 << 32, 1 << 63, size=n, dtype=np.uint64)
    for a, b in ((1023, 1024), (3, 4), (2047, 2048), (0, n - 1), (1020, 3075)):  # tile / workgroup / lane boundaries
        w[a] = w[b] = np.uint64(a + 1)  # equal pairs among the smallest words
    cases["equal pairs across boundaries"] = w
    w = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    w[[5, 1023, 1024, n - 1]] = 0
    w[[6, 1022, 2048, n - 2]] = top
    cases["words 0 and 2^64 - 1"] = w
    cases["only 0 and 2^64 - 1"] = np.where(rng.integers(0, 2, size=n) == 1, np.uint64(top), np.uint64(0)).astype(np.uint64)
    cases["differ only in bit 0"] = np.uint64(0x4000000000000000) | rng.integers(0, 2, size=n, dtype=np.uint64)
    cases["differ only in bit 63"] = np.uint64(0x0123456789ABCDEF) | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63))
    cases["differ only in bit 32"] = np.uint64(0x0123456789ABCDEF) ^ (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(32))
    cases["strictly decreasing"] = (np.uint64(top) - np.arange(n, dtype=np.uint64) * np.uint64(0x000FFFFFFFFFFFFF))
    cases["strictly increasing"] = np.arange(n, dtype=np.uint64) * np.uint64(0x000FFFFFFFFFFFFF)
    words = np.stack(list(cases.values()))
    for h in (1, 2, 1023, 1024, 1025, n // 2, n - 1, n):
        got, want = ctx.debug_fixed_weight_map(words, h), F.fixed_weight_map(words, h)
        for i, name in enumerate(cases):
            assert np.array_equal(got[i], want[i]), (name, h)
        assert np.array_equal(np.flatnonzero(got[0]), np.arange(h)), "all words equal: the support is 0 .. h-1"
        assert np.array_equal(np.flatnonzero(got[-2]), np.arange(n - h, n)), "decreasing: the last h"
    with pytest.raises(ValueError, match="1 .. N"):
        ctx.debug_fixed_weight_map(words, 0)
    # a ring smaller than one wavefront, and one smaller than a tile
    for logn in (3, 8):
        small, m = ring(S, logn)
        w = rng.integers(0, 4, size=(3, m), dtype=np.uint64) << np.uint64(62)  # four distinct values: ties everywhere
        for h in (1, m // 2, m):
            assert np.array_equal(small.debug_fixed_weight_map(w, h), F.fixed_weight_map(w, h)), (logn, h)
        small.close()
    ctx.close()


# ------------------------------------------------------------------ 2. keys
@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("logn", [3, 12])
def test_generate_sparse_secret_key(S, scheme, logn):
    """the inverse transform of row j is the host sample lifted modulo q_j (the oracle's inverse NTT on the device's words)"""
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [40, 41, 42, 50] if logn == 12 else [20, 21, 22, 23])
    t = T if scheme == 1 else 0
    ref = O.RefContext(scheme, logn, mods, nsp=1, t=t)
    ctx = S.Context(scheme, logn, mods, 1, t)
    for seed, h in ((np.zeros(8, dtype=np.uint64), 1), (np.arange(8, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15), n // 4),
                    (np.full(8, 3, dtype=np.uint64), n)):
        s = ctx.sample_fixed_weight_host(seed, h)[0]
        assert np.array_equal(s, F.sample_fixed_weight(S, seed, n, h)[0]) and np.count_nonzero(s) == h
        got = ctx.generate_sparse_secret_key(seed, h).download((len(mods), n))
        for j in range(len(mods)):
            O.lib().ref_ntt_inverse(O.ptr(got[j]), ref.tables(j))
        assert np.array_equal(got, F.lifted(s, mods)), (scheme, logn, h)
    with pytest.raises(ValueError, match="1 .. N"):
        ctx.generate_sparse_secret_key(seed, 0)
    ctx.close()


# (scheme, logn, bit sizes, nsp): nsp 1..3, n_ct = 4 or 5 with a short last digit for nsp 2 and 3
SWITCHING_CASES = [(2, 4, [30, 35, 40, 45, 50], 1), (1, 4, [30, 35, 40, 45, 50, 55, 60], 2), (2, 12, [40, 40, 45, 50, 50, 60, 60], 2),
                   (1, 12, [36, 36, 37, 40, 60, 60, 60], 3), (2, 12, [50, 50, 50, 50, 55, 59, 59, 59], 3)]


@pytest.mark.parametrize("case", SWITCHING_CASES, ids=lambda c: "s%d-logn%d-k%d-nsp%d" % (c[0], c[1], len(c[2]), c[3]))
def test_switching_keys_word_for_word(S, case):
    scheme, logn, bits, nsp = case
    st = Setup(S, scheme, logn, bits, nsp)
    W = wire()
    assert st.k % nsp or nsp == 1, "a short last digit"
    n_keys = 2
    other = [O.Client(st.ref, seed=90 + i) for i in range(n_keys)]
    s_from = np.stack([c.sk for c in other])
    d_from = st.ctx.upload(s_from)
    ev = S.Evaluator(st.ctx)
    seeds, noise = st.samples(n_keys)
    full = [st.expected(s_from[i], seeds[i], noise[i]) for i in range(n_keys)]
    keys_full = st.ctx.generate_switching_keys(st.sk, d_from, n_keys, st.k, seeds, st.ctx.upload_i32(noise))
    assert S.save_kswitch_keys(st.ctx, keys_full) == st.stream(W, full), (case, "full")
    rng = np.random.default_rng(logn + nsp)
    for level in (1, 2):
        kept = (level + nsp - 1) // nsp
        exp = [k.copy() for k in full]
        for k in exp:
            k[:, :, level : st.k] = 0
            k[kept:] = 0
        keys = st.ctx.generate_switching_keys(st.sk, d_from, n_keys, level, seeds, st.ctx.upload_i32(noise))
        assert S.save_kswitch_keys(st.ctx, keys) == st.stream(W, exp), (case, level)
        assert any(np.any(k[:kept, :, :level]) for k in exp) and all(not np.any(k[:, :, level : st.k]) for k in exp)
        # at levels <= level it is the full key; above, it is refused
        for k in range(1, level + 1):
            ct = st.ctx.upload(rows(rng, st.mods[:k], st.n, (3, 2)))
            a, b = st.ctx.alloc(3 * 2 * k * st.n), st.ctx.alloc(3 * 2 * k * st.n)
            ev.switch_secret(ct, k, 3, keys[1], a)
            ev.switch_secret(ct, k, 3, keys_full[1], b)
            assert np.array_equal(a.download(), b.download()), (case, level, k)
        if level < st.k:
            with pytest.raises(ValueError, match="not valid for encryption parameters"):
                ev.switch_secret(ct, level + 1, 1, keys[0], a)
            with pytest.raises(ValueError, match="not valid for encryption parameters"):
                st.ctx.switch_key_inplace(level + 1, ct, ct, 1, keys[0])


def test_switching_keys_edges(S):
    st = Setup(S, 1, 8, [30, 40, 50, 60], 1)
    L = S.lib()
    seeds, noise = st.samples(3)
    dn = st.ctx.upload_i32(noise)
    sp = seeds.ctypes.data
    three = st.ctx.upload(np.stack([st.cl.sk] * 3))
    assert st.ctx.generate_switching_keys(st.sk, three, 0, 1, seeds[:0], dn) == []
    assert st.ctx.generate_switching_keys(st.sk, None, 0, 1, seeds[:0], dn) == []
    for args in ((None, three.ptr, 3, 1, sp, dn.ptr), (st.sk.ptr, None, 3, 1, sp, dn.ptr), (st.sk.ptr, three.ptr, 3, 1, None, dn.ptr),
                 (st.sk.ptr, three.ptr, 3, 1, sp, None)):
        out = (C.c_void_p * 3)(1, 2, 3)
        with pytest.raises(TypeError):
            S._check(L.sealhip_generate_switching_keys(st.ctx.handle, *args, 0, out))
    for level in (0, st.k + 1):
        out = (C.c_void_p * 3)(1, 2, 3)
        with pytest.raises(ValueError, match="level"):
            S._check(L.sealhip_generate_switching_keys(st.ctx.handle, st.sk.ptr, three.ptr, 3, level, sp, dn.ptr, 0, out))
        assert list(out) == [None, None, None]
    with pytest.raises(ValueError, match="invalid count"):
        st.ctx.generate_switching_keys(st.sk, three, 15, 1, np.zeros((15, st.d, 8), np.uint64), dn)
    with pytest.raises(ValueError, match="keeps no seeds"):
        st.ctx.generate_switching_keys(st.sk, three, 1, 1, seeds[:1], dn, keep_seeds=True)
    # the full key keeps its seeds like a relin key: the seeded stream is the oracle's
    W = wire()
    keys = st.ctx.generate_switching_keys(st.sk, three, 1, st.k, seeds[:1], dn, keep_seeds=True)
    exp = [st.expected(st.cl.sk, seeds[0], noise[0])]
    assert S.save_kswitch_keys_seeded(st.ctx, keys) == st.seeded_stream(W, exp, seeds[:1])


# ------------------------------------------------------------------ 3. switch_secret
@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
@pytest.mark.parametrize("scheme,logn,bits,nsp", [(2, 12, [40, 45, 50, 50, 60, 60], 2), (1, 12, [36, 36, 37, 40, 60], 1),
                                                 (2, 4, [40, 45, 50, 60], 1), (1, 13, [40, 40, 45, 60, 60, 60], 3)],
                         ids=["ckks-2sp", "bfv-1sp", "ckks-n16", "bfv-3sp"])
def test_switch_secret_words(S, scheme, logn, bits, nsp, mode):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits)
    t = T if scheme == 1 else 0
    ctx = S.Context(scheme, logn, mods, nsp, t, mode=mode)
    ref = O.RefContext(scheme, logn, mods, nsp=nsp, t=t, mode=mode)
    ev = S.Evaluator(ctx)
    n_ct = len(mods) - nsp
    rng = np.random.default_rng(7 * logn + scheme + mode)
    key = rows(rng, mods, n, ((n_ct + nsp - 1) // nsp, 2))
    d_key = S.KSwitchKeys(ctx, key)
    for k in sorted({1, 2, n_ct}):
        for count in (1, 5):
            ct = rows(rng, mods[:k], n, (count, 2))
            d_ct, out = ctx.upload(ct), ctx.alloc(count * 2 * k * n)
            ev.switch_secret(d_ct, k, count, d_key, out)
            want = np.stack([F.switch_secret(ref, ct[i], key) for i in range(count)])
            assert np.array_equal(out.download(ct.shape), want), (k, count)
            assert np.array_equal(d_ct.download(ct.shape), ct), "the input is not modified"
            # the words of switch_key_inplace on a copy whose c_1 is zeroed, with target c_1
            z = ct.copy()
            z[:, 1] = 0
            d_z = ctx.upload(z)
            ctx.switch_key_inplace(k, d_z, ctx.upload(np.ascontiguousarray(ct[:, 1])), count, d_key)
            assert np.array_equal(d_z.download(ct.shape), want), (k, count, "switch_key_inplace")


def test_switch_secret_decrypts_and_edges(S):
    """CKKS with 59-bit special primes (60-bit ones do not decrypt on the oracle itself at N = 2^12) and
    STRICT BFV: a ciphertext under s_from, switched with a key the device made, decrypts under s_to to what it decrypted to
    under s_from -- exactly for BFV, within the key switch's noise for CKKS. Then refusals, the empty batch, a host-only
    context, transparency flags."""
    logn, n = 12, 1 << 12
    rng = np.random.default_rng(12)
    for scheme, bits, nsp, mode in ((2, [50, 50, 50, 59, 59], 2, 0), (1, [45, 45, 45, 45, 45], 2, 1)):
        st = Setup(S, scheme, logn, bits, nsp, mode=mode)
        ctx, ev, k = st.ctx, S.Evaluator(st.ctx), st.k
        s_to = st.cl
        s_from = F.SecretClient(st.ref, ctx.sample_fixed_weight_host(np.full(8, 9, dtype=np.uint64), 64)[0], seed=3)
        seeds, noise = st.samples(1)
        key = ctx.generate_switching_keys(st.sk, ctx.upload(s_from.sk), 1, k, seeds, ctx.upload_i32(noise))[0]
        if scheme == 1:
            m = rng.integers(0, T, size=n, dtype=np.uint64)
            ct = s_from.encrypt_bfv(m)
            assert np.array_equal(s_from.decrypt_bfv(ct), m)
        else:
            m = rng.integers(-(1 << 40), 1 << 40, size=n).astype(np.int64)
            ct = s_from.encrypt_poly_ntt([int(v) for v in m])
        out = ctx.alloc(2 * k * n)
        ev.switch_secret(ctx.upload(ct), k, 1, key, out)
        got = out.download((2, k, n))
        if scheme == 1:
            assert np.array_equal(s_to.decrypt_bfv(got), m)
        else:
            before, _ = F.decrypt_centred(s_from, ct)
            after, _ = F.decrypt_centred(s_to, got)
            worst = max(abs(a - b) for a, b in zip(before, after))
            print("CKKS switch_secret: max|difference of the decryptions| =", worst)
            assert worst < 1 << 16 and max(abs(int(v) - int(x)) for v, x in zip(after, m)) < 1 << 16
    # ---- edges (the CKKS... the last context is BFV strict: any will do)
    d_ct = ctx.upload(ct)
    count = 3
    three = ctx.upload(np.stack([ct] * count))
    out3 = ctx.alloc(count * 2 * k * n)
    for bad_k in (0, k + 1):
        with pytest.raises(ValueError, match="level"):
            ev.switch_secret(d_ct, bad_k, 1, key, out)
    with pytest.raises(ValueError, match="overlap"):
        ev.switch_secret(d_ct, k, 1, key, d_ct)
    short = S.KSwitchKeys(ctx, rows(rng, st.mods, n, (1, 2)))
    with pytest.raises(ValueError, match="not valid for encryption parameters"):
        ev.switch_secret(d_ct, k, 1, short, out)
    for args in ((None, k, 1, key, out), (d_ct, k, 1, None, out), (d_ct, k, 1, key, None)):
        with pytest.raises(TypeError):
            ev.switch_secret(*args)
    before = out.download().copy()
    ev.switch_secret(d_ct, k, 0, key, out)  # the empty batch launches nothing
    assert np.array_equal(out.download(), before)
    host = S.Context(1, logn, st.mods, 2, T, mode=1, device=-1)
    hev = S.Evaluator(host)
    with pytest.raises(ValueError, match="overlap"):
        hev.switch_secret(d_ct, k, 1, key, d_ct)
    hev.switch_secret(d_ct, k, 0, key, out)
    with pytest.raises(S.LogicError, match="host-only"):
        hev.switch_secret(d_ct, k, 1, key, out)
    # transparency: the result's c_1 is the key switch's; a zero key makes it zero
    flags = ctx.alloc(4)
    ctx.transparency_sink(flags, 8)
    ev.switch_secret(three, k, count, key, out3)
    assert list(flags.download().view(np.uint32)[:count] != 0) == [True, True, True]
    zero_key = S.KSwitchKeys(ctx, np.zeros((st.d, 2, st.n_key, n), dtype=np.uint64))
    ev.switch_secret(three, k, count, zero_key, out3)
    assert list(flags.download().view(np.uint32)[:count] != 0) == [False, False, False]
    with pytest.raises(ValueError, match="transparency sink"):
        ev.switch_secret(ctx.upload(np.stack([ct] * 9)), k, 9, key, ctx.alloc(9 * 2 * k * n))
    ctx.transparency_sink(None, 0)


# ------------------------------------------------------------------ 4. the encapsulated bootstrap, end to end
def test_bootstrap_encapsulated_end_to_end(S):
    """The parameters of test_bootstrap_end_to_end (N = 2^12 -- a test shape, not a secure ring --, a 50-bit q_0, fifteen primes
    next to 12 q_0, two 59-bit special primes; (K, r, d) = (12, 3, 31), stages [4,4,3] / [6,5]); every key made by the
    library on the device: the dense secret from generate_secret_key, the weight-32 one from generate_sparse_secret_key,
    to_sparse with level 1, to_dense at the full level, Galois and relinearization keys under the dense secret.
    (a) the words are those of the chain through the separate entries; (b) the result decrypts under the DENSE secret to m
    within 2^-16 max|m| (the sine term alone is 2^-19.3); (c) the pool returns to zero after destroy; (d) a batch of 3 equals
    three single calls.
    Measured on the MI355X: max|I| = 7 after the encapsulated raise; max coefficient error / max|m| = 2^-19.28, the sine
    term, as for the plain bootstrap under a sparse working key."""
    logn, n, K, r, d, nb = 12, 1 << 12, 12, 3, 31, 8
    mods = bootstrap_mods(logn)
    q0 = mods[0]
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 2, 0)
    ref = O.RefContext(2, logn, mods, nsp=2, t=0, mode=0)
    ev = S.Evaluator(ctx)
    k_top, c2s_counts, s2c_counts, nd = 16, [4, 4, 3], [6, 5], 8
    plan = ev.bootstrap_plan(k_top, c2s_counts, s2c_counts, K, r, d, n_baby=nb)
    assert (plan["c2s_out_level"], plan["evalmod_out_level"], plan["out_level"]) == (13, 4, 2)
    rng = np.random.default_rng(79)
    seed_dense, seed_sparse = rng.integers(0, 2**64, size=(2, 8), dtype=np.uint64)
    d_dense, d_sparse = ctx.generate_secret_key(seed_dense), ctx.generate_sparse_secret_key(seed_sparse, 32)
    s_dense = ctx.sample_polys_host(seed_dense, 1, 0)[0]
    assert abs(np.count_nonzero(s_dense) - 2 * n / 3) < 150 and np.count_nonzero(ctx.sample_fixed_weight_host(seed_sparse, 32)) == 32
    cl = F.SecretClient(ref, s_dense, seed=23)
    assert np.array_equal(d_dense.download((len(mods), n)), cl.sk)

    def samples(count):
        return (rng.integers(0, 2**64, size=(count, nd, 8), dtype=np.uint64, endpoint=False),
                ctx.upload_i32(rng.integers(-6, 7, size=(count, nd, n), dtype=np.int32)))

    elts = sorted({H.elt_from_step(n, s) for s in plan["key_steps"]} | {2 * n - 1})
    gk = dict(zip(elts, ctx.generate_galois_keys(d_dense, elts, *samples(len(elts)))))
    rk = ctx.generate_relin_keys(d_dense, 1, *samples(1))
    to_sparse = ctx.generate_switching_keys(d_sparse, d_dense, 1, 1, *samples(1))[0]
    to_dense = ctx.generate_switching_keys(d_dense, d_sparse, 1, k_top, *samples(1))[0]
    count = 3
    m = rng.integers(-(1 << 39), 1 << 39, size=(count, n)).astype(np.int64)
    low = np.stack([np.ascontiguousarray(cl.encrypt_poly_ntt([int(v) for v in m[i]])[:, :1]) for i in range(count)])
    d_low = ctx.upload(low)  # (3, 2, 1, N): the q_0 rows
    tables = S.BootstrapTables(ctx, k_top, c2s_counts, s2c_counts, K, r, d, n_baby=nb)
    out = ctx.alloc(count * 2 * 2 * n)
    ev.bootstrap_encapsulated(tables, d_low, 1, count, gk, rk, to_sparse, to_dense, out)
    got = out.download((count, 2, 2, n))
    held = ctx.pool_stats()["bytes_in_use"]
    ev.bootstrap_encapsulated(tables, d_low, 1, count, gk, rk, to_sparse, to_dense, out)
    assert ctx.pool_stats()["bytes_in_use"] == held, "no new block after the first call"
    # (d) a batch of 3 equals three single calls
    one = ctx.alloc(2 * 2 * n)
    for i in range(count):
        ev.bootstrap_encapsulated(tables, ctx.upload(low[i]), 1, 1, gk, rk, to_sparse, to_dense, one)
        assert np.array_equal(one.download((2, 2, n)), got[i]), i
    # (a) the chain through the separate entries, first item
    em = plan["evalmod"]
    low_sparse, up_sparse, up = ctx.alloc(2 * n), ctx.alloc(2 * k_top * n), ctx.alloc(2 * k_top * n)
    ev.switch_secret(ctx.upload(low[0]), 1, 1, to_sparse, low_sparse)
    ev.mod_raise(low_sparse, 1, 1, k_top, up_sparse)
    ev.switch_secret(up_sparse, k_top, 1, to_dense, up)
    t1 = S.DftTables(ctx, R.C2S, k_top, c2s_counts)
    t2 = S.DftTables(ctx, R.S2C, 4, s2c_counts, gain=plan["s2c_gain"])
    re, im = ctx.alloc(2 * 13 * n), ctx.alloc(2 * 13 * n)
    ev.coeffs_to_slots(t1, up, 1, gk, re, im)
    halves = []
    for half in (re, im):
        sine = ctx.alloc(2 * 4 * n)
        assert ev.eval_mod(half, 13, 1, plan["raise_scale"], K, r, d, rk, sine, n_baby=nb) == (4, em["out_scale"])
        halves.append(sine)
    chain = ctx.alloc(2 * 2 * n)
    ev.slots_to_coeffs(t2, halves[0], halves[1], 1, gk, chain)
    assert np.array_equal(got[0], chain.download((2, 2, n))), "bootstrap_encapsulated differs from the chain of entries"
    # the raise ran under the sparse secret: I stays inside K
    c, _ = F.decrypt_centred(cl, up.download((2, k_top, n)))
    I = [(c[j] - int(m[0, j]) + q0 // 2) // q0 for j in range(n)]
    print("encapsulated ModRaise on the device: max|I| = %d" % max(abs(v) for v in I))
    assert max(abs(v) for v in I) <= K - 1
    # (b) under the DENSE secret
    plain = ctx.alloc(count * 2 * n)
    ctx.decrypt(out, 2, 2, count, ctx.upload(cl.sk_powers(1)), True, plain)
    dec = plain.download((count, 2, n))
    worst = 0.0
    for i in range(count):
        vals, _ = cl.centered_from_ntt_rows(dec[i])
        worst = max(worst, max(abs(int(vals[j]) - int(m[i, j])) for j in range(n)) / float(np.max(np.abs(m[i]))))
    print("bootstrap_encapsulated: max coefficient error / max|m| = 2^%.2f" % np.log2(worst))
    assert worst < 2.0 ** -16
    # the keys' checks: to_sparse serves level 1 only, so it cannot stand in for to_dense
    with pytest.raises(ValueError, match="not valid for encryption parameters"):
        ev.bootstrap_encapsulated(tables, d_low, 1, count, gk, rk, to_sparse, to_sparse, out)
    for a, b in ((None, to_dense), (to_sparse, None)):
        with pytest.raises(TypeError):
            ev.bootstrap_encapsulated(tables, d_low, 1, count, gk, rk, a, b, out)
    # (c)
    for t in (t1, t2, tables):
        t.free()
    assert ctx.pool_stats()["bytes_in_use"] == 0, "destroy releases the blocks"


# ------------------------------------------------------------------ 5. the C++ adapter
def seed_number(i):
    mask = (1 << 64) - 1
    return np.array([((0x5EED000000000000 + i + j) * 0x9E3779B97F4A7C15) & mask for j in range(8)], dtype=np.uint64)


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_sparse_secret_check.cpp on the device: from a counting SeedSource, KeyGenerator's sparse secret key,
    its dense -> sparse (level 1) and sparse -> dense switching keys and Evaluator::switch_secret give the bytes of the C ABI
    entries fed the same seeds (the noise of digit j drawn from the second seed of its pair as sample_polys (0, 1)); inside the
    program, the host and DeviceCiphertext forms of switch_secret and of the encapsulated bootstrap equal the C ABI's words."""
    logn, n, nd = 8, 256, 10
    q0 = O.get_primes(n, 40, 1)[0]
    mods = [q0] + primes_next_to(2 * q0, logn, 9) + O.get_primes(n, 59, 1)
    exe = compile_cpp(tmp_path, "host_adapter_sparse_secret_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    assert "sparse secret adapter checks ok" in stdout, stdout
    lines = dict(l.split(" digest ") for l in stdout.splitlines() if " digest " in l)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ctx.set_parms_id(len(mods), (0x1111, 0x2222, 0x3333, 0x4444))
    dense, sparse = ctx.generate_secret_key(seed_number(0)), ctx.generate_sparse_secret_key(seed_number(1), 16)
    assert int(lines["sparse_sk"], 16) == O.fnv(sparse.download())

    def key(to, frm, first, level):
        public = np.stack([seed_number(first + 2 * j) for j in range(nd)])
        noise = ctx.alloc(nd * n // 2)
        ctx.sample_polys(np.stack([seed_number(first + 2 * j + 1) for j in range(nd)]), 0, 1, noise)
        return ctx.generate_switching_keys(to, frm, 1, level, public, noise)[0]

    to_sparse, to_dense = key(sparse, dense, 2, 1), key(dense, sparse, 2 + 2 * nd, nd)
    assert int(lines["to_sparse"], 16) == fnv(S.save_kswitch_keys(ctx, [to_sparse]))
    assert int(lines["to_dense"], 16) == fnv(S.save_kswitch_keys(ctx, [to_dense]))
    top = O.SplitMix(0x5A25E).fill(2 * nd, n, mods[:nd] * 2)
    out = ctx.alloc(2 * nd * n)
    S.Evaluator(ctx).switch_secret(ctx.upload(top), nd, 1, to_dense, out)
    assert int(lines["switch_secret"], 16) == O.fnv(out.download())
