"""Seed expansion on the device (sealhip_expand_seed, sealhip_ciphertext_load_many, sealhip_debug_seed_slack): what can be
checked without a GPU. The exports exist; on a host-only context the new entries fail like every compute entry (no CPU
fallback), with E_POINTER first for null pointers; and the parallel form of the rule that DESIGN.md "Seed expansion"
documents -- candidate m is word m & 7 of leaf (m >> 3) & 63 of PRNG buffer m >> 9, r = (low32 << 31) | (high32 >> 1),
row j takes its N accepted candidates in stream order -- restated here from sealhip.blake2xb, equals the library's host
expansion (csrc/blake2xb.cpp, pinned to the reference by tests/test_host.py)."""
import ctypes as C
import struct

import numpy as np
import pytest

import oracle_lib as O

MAX_RANDOM = (1 << 63) - 1


def is_prime(n):
    if n < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in bases:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:  # deterministic below 2^64
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def reject_chain(logn, count):
    """`count` 60-bit primes = 1 mod 2N just above 2^63 / 9: each rejects about 11 % of the candidates"""
    step = 2 << logn
    m, out = (2**63 // 9) // step + 1, []
    while len(out) < count:
        if is_prime(m * step + 1):
            out.append(m * step + 1)
        m += 1
    return out


def threshold(q):
    return MAX_RANDOM - (MAX_RANDOM % q) - 1  # util/rlwe.cpp:113-117


def restated_expand(S, seed_words, moduli, n):
    """The rule of DESIGN.md "Seed expansion" in numpy: returns (rows x n words, rejected candidates)"""
    key = struct.pack("<8Q", *[int(x) for x in seed_words])
    bufs = []

    def candidates(upto):  # r of candidates 0 .. upto-1
        while len(bufs) * 512 < upto:
            raw = S.blake2xb(4096, struct.pack("<Q", len(bufs)), key)  # buffer c: in = c (8 LE bytes), key = seed
            w = np.frombuffer(raw, dtype="<u8").astype(np.uint64)  # leaf i = bytes 64i..64i+63, word = 8 bytes each
            lo32, hi32 = w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)
            bufs.append((lo32 << np.uint64(31)) | (hi32 >> np.uint64(1)))
        return np.concatenate(bufs)[:upto]

    out = np.zeros((len(moduli), n), dtype=np.uint64)
    pos, rejected = 0, 0
    for j, q in enumerate(moduli):
        T, need = threshold(q), n
        upto = pos + n + 64
        while True:
            r = candidates(upto)[pos:]
            acc = np.nonzero(r < np.uint64(T))[0]
            if len(acc) >= need:
                break
            upto += n
        last = acc[need - 1]
        out[j] = r[acc[:need]] % np.uint64(q)
        rejected += int(last + 1 - need)
        pos += int(last) + 1
    return out, rejected


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in ("sealhip_expand_seed", "sealhip_ciphertext_load_many", "sealhip_debug_seed_slack"):
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("expand_seeds", "load_ciphertexts", "debug_seed_slack"):
        assert callable(getattr(S.Context, name))


def test_host_only_context_has_no_cpu_fallback():
    import sealhip as S

    logn, n = 6, 64
    mods = O.coeff_modulus_create(n, [30, 30])
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, device=-1)
    L = S.lib()
    seeds = np.zeros((2, 8), dtype=np.uint64)
    out = np.zeros(2 * n, dtype=np.uint64)
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.expand_seeds(1, seeds, out.ctypes.data)
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.expand_seeds(1, seeds[:0], out.ctypes.data)  # count 0 too: the entry itself needs a device
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.debug_seed_slack(0)
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.load_ciphertexts([b"x" * 16], out.ctypes.data, 2 * n)
    # null pointers are reported before the context is looked at
    with pytest.raises(TypeError):
        S._check(L.sealhip_expand_seed(ctx.handle, 1, None, 1, out.ctypes.data, 0))
    with pytest.raises(TypeError):
        S._check(L.sealhip_expand_seed(ctx.handle, 1, seeds.ctypes.data, 1, None, 0))
    with pytest.raises(TypeError):
        S._check(L.sealhip_expand_seed(None, 1, seeds.ctypes.data, 1, out.ctypes.data, 0))
    with pytest.raises(TypeError):
        S._check(L.sealhip_debug_seed_slack(None, 0))
    lens = (C.c_size_t * 1)(16)
    infos = (S.CiphertextInfo * 1)()
    ptrs = (C.c_void_p * 1)(None)
    with pytest.raises(TypeError):  # a null stream inside the array
        S._check(L.sealhip_ciphertext_load_many(ctx.handle, C.addressof(ptrs), C.addressof(lens), 1, C.addressof(infos),
                                                out.ctypes.data, 2 * n))
    with pytest.raises(TypeError):
        S._check(L.sealhip_ciphertext_load_many(ctx.handle, None, C.addressof(lens), 1, C.addressof(infos), out.ctypes.data,
                                                2 * n))
    # the host reference stays available on host-only contexts
    assert ctx.expand_seed(2, [0] * 8).shape == (2, n)


@pytest.mark.parametrize("logn", [3, 6, 10])
def test_restated_rule_equals_host_expansion(logn):
    """the parallel form of the rule (buffer / leaf / word, r, per-row thresholds, row hand-over) equals sample_poly_uniform
    over BlakePRNG word for word, on primes that reject about 11 % and on primes that almost never reject"""
    import sealhip as S

    n = 1 << logn
    rng = np.random.default_rng(logn)
    chains = [reject_chain(logn, 4), O.coeff_modulus_create(n, [20, 36, 50, 55, 60])]
    for mods in chains:
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0, device=-1)
        total_rejected = 0
        for seed in ([0] * 8, [int(x) for x in rng.integers(0, 2**63, size=8)], [2**64 - 1 - i for i in range(8)]):
            for rows in (1, len(mods) - 1, len(mods)):
                want = ctx.expand_seed(rows, seed)
                got, rejected = restated_expand(S, seed, mods[:rows], n)
                assert np.array_equal(got, want), (logn, rows, mods)
                total_rejected += rejected
        if mods[0] > 2**59:
            assert total_rejected > 0  # the rejection chain did take the rejection branch
