"""Encryptor on the device (sealhip_encryptor_encrypt, sealhip_encryptor_encrypt_symmetric, sealhip_ciphertext_save_seeded).
Every word is compared with Encryptor::encrypt_internal / encrypt_zero_internal (encryptor.cpp:106-259) restated from oracle
entries only, on the same samples:
  public key: ref_encrypt_zero_asymmetric_given over the k + 1 rows of the previous level (k rows at the key level), the
  oracle's divide_and_round_q_last(_ntt)_inplace with RefContext.rns_tool(k + 1), the first k rows, then
  ref_multiply_add_plain_with_scaling_variant (BFV) or ref_add_poly_coeffmod of the NTT-form plaintext (CKKS);
  secret key: ref_encrypt_zero_symmetric_given with a = the oracle's expand_seed of the seed (BFV seeded: a sampled in
  coefficient form and transformed with ref_ntt_forward, c_1 = the sample), then the same plaintext step.
The fused entries are also compared with the existing entries chained on the device, and fresh encryptions are decrypted
with sealhip_decryptor_decrypt."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from encrypt_edge_ref import divround_restated
from support import S, compile_cpp, run_exe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PID = (0x5151, 0x6262, 0x7373, 0x8484)
T = 786433  # prime, = 1 mod 2^18


def wire():
    spec = importlib.util.spec_from_file_location("wire_format", os.path.join(ROOT, "oracle", "wire_format.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    return W


class Setup:
    """a context on both sides, a secret key, and the key-level public key (2 x n_key x N, NTT form); not a BaseSession:
    the oracle side and its client come first, the moduli may be given, there is no evaluator"""

    def __init__(self, S, scheme, logn, bits, nsp, mods=None):
        self.S, self.scheme = S, scheme
        self.n = n = 1 << logn
        self.logn, self.nsp = logn, nsp
        self.mods = [int(q) for q in mods] if mods is not None else O.coeff_modulus_create(n, bits)
        self.n_key = len(self.mods)
        self.k = self.n_key - nsp
        self.t = T if scheme == 1 else 0
        self.ref = O.RefContext(scheme, logn, self.mods, nsp=nsp, t=self.t)
        self.cl = O.Client(self.ref, seed=logn * 11 + nsp + 3 * scheme)
        self.ctx = S.Context(scheme, logn, self.mods, nsp, self.t)
        for k in range(1, self.n_key + 1):
            self.ctx.set_parms_id(k, (PID[0] + k,) + PID[1:])
        self.pk = np.zeros((2, self.n_key, n), dtype=np.uint64)
        O.lib().ref_encrypt_zero_symmetric(C.byref(self.ref.c), self.n_key, O.ptr(self.cl.sk), 1, C.byref(self.cl.state),
                                           O.ptr(self.pk))
        self.d_pk = self.ctx.upload(self.pk)
        self.d_sk = self.ctx.upload(self.cl.sk)
        self.rng = np.random.default_rng(977 * logn + 13 * nsp + scheme + len(self.mods))

    # ---- samples
    def asym_samples(self, count):
        u = self.rng.integers(-1, 2, size=(count, self.n), dtype=np.int32)
        e = self.rng.integers(-41, 42, size=(count, 2, self.n), dtype=np.int32)
        return u, e

    def sym_samples(self, count):
        seeds = self.rng.integers(0, 2**64, size=(count, 8), dtype=np.uint64, endpoint=False)
        e = self.rng.integers(-41, 42, size=(count, self.n), dtype=np.int32)
        return seeds, e

    def plains(self, k, count):
        if self.scheme == 1:
            return self.rng.integers(0, self.t, size=(count, self.n), dtype=np.uint64)
        return np.stack([np.stack([self.rng.integers(0, self.mods[r], size=self.n, dtype=np.uint64) for r in range(k)])
                         for _ in range(count)])

    # ---- oracle compositions (one item)
    def add_plain(self, k, ct, plain):
        L, c = O.lib(), self.ref.c
        if plain is None:
            return ct
        if self.scheme == 1:
            L.ref_multiply_add_plain_with_scaling_variant(C.byref(c), k, O.ptr(np.ascontiguousarray(plain)), 0, O.ptr(ct[0]))
        else:
            for r in range(k):
                L.ref_add_poly_coeffmod(O.ptr(ct[0, r]), O.ptr(np.ascontiguousarray(plain[r])), self.n, C.byref(c.key_mod[r]),
                                        O.ptr(ct[0, r]))
        return ct

    def expected_asym(self, k, u, e, plain):
        L, c = O.lib(), self.ref.c
        R = k + 1 if k < self.n_key else k
        ntt = 1 if self.scheme == 2 else 0
        pk = np.ascontiguousarray(self.pk[:, :R])
        big = np.zeros((2, R, self.n), dtype=np.uint64)
        L.ref_encrypt_zero_asymmetric_given(C.byref(c), R, O.ptr(pk), ntt, np.ascontiguousarray(u).ctypes.data,
                                            np.ascontiguousarray(e).ctypes.data, O.ptr(big))
        if R == k + 1:
            tool = L.ref_context_rns_tool(C.byref(c), R)
            for j in range(2):
                if not tool:  # the oracle builds no RNSTool where the level's Bsk base cannot be formed (60-bit primes)
                    divround_restated(big[j], self.mods, R, ntt, c)
                elif ntt:
                    L.ref_divide_and_round_q_last_ntt_inplace(tool, O.ptr(big[j]), c.key_tables, 0)
                else:
                    L.ref_divide_and_round_q_last_inplace(tool, O.ptr(big[j]))
        ct = np.ascontiguousarray(big[:, :k])
        return self.add_plain(k, ct, plain)

    def expected_sym(self, k, seed, e, plain, save_seed):
        L, c = O.lib(), self.ref.c
        a = np.ascontiguousarray(O.expand_seed(seed, self.mods[:k], self.n))
        sample = a.copy()
        seeded = save_seed and self.scheme == 1 and k * self.n >= 9
        if seeded:  # rlwe.cpp:233-243: a sampled in coefficient form, transformed before a*s; c_1 keeps the sample
            for r in range(k):
                L.ref_ntt_forward(O.ptr(a[r]), C.byref(c.key_tables[r]), 0)
        ct = np.zeros((2, k, self.n), dtype=np.uint64)
        L.ref_encrypt_zero_symmetric_given(C.byref(c), k, O.ptr(self.cl.sk), 1 if self.scheme == 2 else 0, O.ptr(a),
                                           np.ascontiguousarray(e).ctypes.data, O.ptr(ct))
        if seeded:  # c_1 is stored as the seed: what Ciphertext::expand_seed restores is the sample itself. (On 60-bit primes
            ct[1] = sample  # the reference's uncorrected forward NTT wraps (DESIGN F2), so INTT(NTT(sample)) is not the sample.)
        return self.add_plain(k, ct, plain)

    # ---- device
    def encrypt(self, k, u, e, plain, count, stride=None):
        ct = self.ctx.alloc(count * 2 * k * self.n)
        dp = self.ctx.upload(plain) if plain is not None else None
        self.ctx.encrypt(k, self.d_pk, dp, self.ctx.upload_i32(u), self.ctx.upload_i32(e), count, ct, plain_item_stride=stride)
        return ct.download((count, 2, k, self.n))

    def encrypt_sym(self, k, seeds, e, plain, count, save_seed, stride=None):
        ct = self.ctx.alloc(count * 2 * k * self.n)
        dp = self.ctx.upload(plain) if plain is not None else None
        self.ctx.encrypt_symmetric(k, self.d_sk, dp, seeds, self.ctx.upload_i32(e), count, ct, save_seed=save_seed,
                                   plain_item_stride=stride)
        return ct.download((count, 2, k, self.n))


# (scheme, logn, bits, nsp): every prime class -- 55-bit (integer instances), below 2^50 (FP64 instances), 60-bit -- and
# nsp 1..3 (the previous level of the first level has k_first + 1 rows)
ASYM_CASES = [
    (1, 3, [60, 60], 1),
    (1, 5, [30, 40, 50], 2),
    (1, 12, [55, 55, 55, 55], 1),
    (1, 12, [49, 49, 49, 49, 49], 3),
    (1, 13, [60, 60, 60, 60], 2),
    (1, 16, [55] * 4, 1),
    (2, 3, [60, 60], 1),
    (2, 10, [49, 40, 40, 49], 2),
    (2, 12, [55, 55, 55, 55], 1),
    (2, 13, [60, 50, 50, 60, 60], 3),
    (2, 16, [49] * 3, 1),
]


def case_id(c):
    return "%s-n%d-%s-nsp%d" % ("bfv" if c[0] == 1 else "ckks", c[1], "x".join(map(str, c[2])), c[3])


@pytest.mark.parametrize("case", ASYM_CASES, ids=case_id)
def test_public_key_encrypt_matches_oracle(S, case):
    """encrypt (plaintext levels) and encrypt_zero (every level, the key level included), 3 items each"""
    st = Setup(S, *case)
    count = 3
    levels = range(1, st.n_key + 1)
    for k in levels:
        u, e = st.asym_samples(count)
        got = st.encrypt(k, u, e, None, count)
        for i in range(count):
            assert np.array_equal(got[i], st.expected_asym(k, u[i], e[i], None)), ("zero", k, i)
    plain_levels = [st.k] if st.scheme == 1 else range(1, st.k + 1)
    for k in plain_levels:
        u, e = st.asym_samples(count)
        pl = st.plains(k, count)
        got = st.encrypt(k, u, e, pl, count)
        for i in range(count):
            assert np.array_equal(got[i], st.expected_asym(k, u[i], e[i], pl[i])), ("plain", k, i)
    # one plaintext for all (plain_item_stride 0)
    k = st.k
    u, e = st.asym_samples(count)
    pl = st.plains(k, 1)
    got = st.encrypt(k, u, e, pl, count, stride=0)
    for i in range(count):
        assert np.array_equal(got[i], st.expected_asym(k, u[i], e[i], pl[0])), ("stride0", i)


SYM_CASES = [
    (1, 3, [60, 60], 1),  # k x N = 8 < 9: save_seed is dropped
    (1, 4, [60, 60], 1),
    (1, 12, [49, 55, 60, 55], 2),
    (1, 15, [55] * 4, 1),
    (2, 3, [60, 60], 1),
    (2, 12, [49, 49, 49, 49], 1),
    (2, 13, [60, 55, 55, 60], 3),
]


@pytest.mark.parametrize("save_seed", [False, True])
@pytest.mark.parametrize("case", SYM_CASES, ids=case_id)
def test_symmetric_encrypt_matches_oracle(S, case, save_seed):
    st = Setup(S, *case)
    count = 3
    for k in sorted({1, st.k, st.n_key}):
        seeds, e = st.sym_samples(count)
        got = st.encrypt_sym(k, seeds, e, None, count, save_seed)
        for i in range(count):
            assert np.array_equal(got[i], st.expected_sym(k, seeds[i], e[i], None, save_seed)), ("zero", k, i)
    plain_levels = [st.k] if st.scheme == 1 else sorted({1, st.k})
    for k in plain_levels:
        seeds, e = st.sym_samples(count)
        pl = st.plains(k, count)
        got = st.encrypt_sym(k, seeds, e, pl, count, save_seed)
        for i in range(count):
            assert np.array_equal(got[i], st.expected_sym(k, seeds[i], e[i], pl[i], save_seed)), ("plain", k, i)


def cfg3(S, scheme=1):
    import bench

    return Setup(S, scheme, 15, None, 1, mods=bench.CFG3_PRIMES)


@pytest.mark.parametrize("count", [1, 3, 1024])
def test_public_key_encrypt_cfg3_counts(S, count):
    """the cfg3 shape (BFV 2^15, 8 primes): counts 1, 3 and 1024, checked against the oracle on a spread of items"""
    st = cfg3(S)
    k = st.k
    u, e = st.asym_samples(count)
    pl = st.plains(k, count)
    got = st.encrypt(k, u, e, pl, count)
    for i in sorted({0, count // 2, count - 1}):
        assert np.array_equal(got[i], st.expected_asym(k, u[i], e[i], pl[i])), i


@pytest.mark.parametrize("scheme", [1, 2])
def test_fused_equals_composed_on_device(S, scheme):
    """the new entries produce the words of the existing entries chained on the device with the same samples:
    encrypt_zero_asymmetric at k + 1 rows, divide_and_round_q_last(_ntt)_inplace, the first k rows, then
    multiply_add_plain_with_scaling_variant / evaluator_add_plain; encrypt_zero_symmetric with the expanded seeds"""
    st = Setup(S, scheme, 13, [55, 49, 50, 55, 55], 2)
    ctx, n, count = st.ctx, st.n, 5
    for k in range(1, st.k + 1):
        R = k + 1
        u, e = st.asym_samples(count)
        pl = st.plains(k, count) if (scheme == 2 or k == st.k) else None
        fused = st.encrypt(k, u, e, pl, count)
        big = ctx.alloc(count * 2 * R * n)
        ctx.encrypt_zero_asymmetric(R, scheme == 2, ctx.upload(np.ascontiguousarray(st.pk[:, :R])), ctx.upload_i32(u),
                                    ctx.upload_i32(e), count, big)
        if scheme == 1:
            ctx.divide_and_round_q_last_inplace(R, big, count * 2)
        else:
            ctx.divide_and_round_q_last_ntt_inplace(R, big, count * 2)
        comp = ctx.upload(big.download((count, 2, R, n))[:, :, :k].copy())
        if pl is not None and scheme == 1:
            ctx.multiply_add_plain_with_scaling_variant(k, ctx.upload(pl), comp, 2, count)
        elif pl is not None:
            assert S.lib().sealhip_evaluator_add_plain(ctx.handle, k, comp.ptr, 2, count, ctx.upload(pl).ptr, k * n, 0) == 0
        assert np.array_equal(fused, comp.download((count, 2, k, n))), k
    # symmetric: encrypt_zero_symmetric over the device-expanded c_1, at the first level
    k = st.k
    seeds, e = st.sym_samples(count)
    fused = st.encrypt_sym(k, seeds, e, None, count, False)
    a = ctx.alloc(count * k * n)
    ctx.expand_seeds(k, seeds, a)
    comp = ctx.alloc(count * 2 * k * n)
    ctx.encrypt_zero_symmetric(k, scheme == 2, a, ctx.upload_i32(e), st.d_sk, count, comp)
    assert np.array_equal(fused, comp.download((count, 2, k, n)))


@pytest.mark.parametrize("scheme", [1, 2])
def test_fresh_encryptions_decrypt(S, scheme):
    """sealhip_decryptor_decrypt returns the plaintext (BFV mod t; CKKS the NTT-form plaintext plus small error), and the
    noise budget of the device ciphertext equals that of the oracle's"""
    st = Setup(S, scheme, 12, [55, 55, 55, 55], 1)
    ctx, n, k, count = st.ctx, st.n, st.k, 4
    pw = ctx.upload(st.cl.sk_powers(1))
    for mode in ("asym", "sym"):
        if scheme == 1:
            pl = st.plains(k, count)
        else:  # a small integer polynomial in NTT form, so that the error is visible against it
            coeffs = st.rng.integers(-(1 << 30), 1 << 30, size=(count, n))
            pl = np.zeros((count, k, n), dtype=np.uint64)
            for i in range(count):
                for r in range(k):
                    row = np.array([int(v) % st.mods[r] for v in coeffs[i]], dtype=np.uint64)
                    O.lib().ref_ntt_forward(O.ptr(row), C.byref(st.ref.c.key_tables[r]), 0)
                    pl[i, r] = row
        if mode == "asym":
            u, e = st.asym_samples(count)
            got = st.encrypt(k, u, e, pl, count)
            want = np.stack([st.expected_asym(k, u[i], e[i], pl[i]) for i in range(count)])
        else:
            seeds, e = st.sym_samples(count)
            got = st.encrypt_sym(k, seeds, e, pl, count, False)
            want = np.stack([st.expected_sym(k, seeds[i], e[i], pl[i], False) for i in range(count)])
        assert np.array_equal(got, want)
        dct = ctx.upload(got)
        if scheme == 1:
            out = ctx.alloc(count * n)
            ctx.decrypt(dct, 2, k, count, pw, False, out)
            assert np.array_equal(out.download((count, n)), pl), mode
            budgets = ctx.invariant_noise_budget(dct, 2, k, count, pw)
            assert (budgets == ctx.invariant_noise_budget(ctx.upload(want), 2, k, count, pw)).all()
            assert (budgets > 0).all()
        else:
            out = ctx.alloc(count * k * n)
            ctx.decrypt(dct, 2, k, count, pw, True, out)
            dec = out.download((count, k, n))
            for i in range(count):
                err = np.array(st.cl.centered_from_ntt_rows(dec[i])[0], dtype=object) - np.array(
                    [int(v) for v in coeffs[i]], dtype=object)
                assert max(abs(int(x)) for x in err) < 1 << 24, mode


@pytest.mark.parametrize("logn", [4, 12])
def test_seeded_stream(S, logn):
    """sealhip_ciphertext_save_seeded writes oracle/wire_format.py's save_ciphertext(..., seed=...), and
    sealhip_ciphertext_load of that stream restores the device ciphertext word for word"""
    W = wire()
    st = Setup(S, 1, logn, [55, 55, 55], 1)
    ctx, n, k = st.ctx, st.n, st.k
    seeds, e = st.sym_samples(2)
    pl = st.plains(k, 2)
    ct = ctx.alloc(2 * 2 * k * n)
    ctx.encrypt_symmetric(k, st.d_sk, ctx.upload(pl), seeds, ctx.upload_i32(e), 2, ct, save_seed=True)
    words = ct.download((2, 2, k, n))
    pid = (PID[0] + k,) + PID[1:]
    for i in range(2):
        info = S.CiphertextInfo()
        for j in range(4):
            info.parms_id[j] = pid[j]
        info.is_ntt_form, info.size, info.coeff_modulus_size = 0, 2, k
        info.poly_modulus_degree, info.scale = n, 1.0
        src = ctx.upload(words[i])
        raw = ctx.save_seeded(info, src, seeds[i])
        assert raw == W.save_ciphertext(pid, False, 2, n, k, 1.0, words[i, 0].reshape(-1), seed=seeds[i].tobytes())
        back = ctx.alloc(2 * k * n)
        got = ctx.load_ciphertext(raw, back)
        assert got.seeded == 1 and got.size == 2
        assert np.array_equal(back.download((2, k, n)), words[i])


def _batch_child():
    """run in a child process with a 512 MB arena: 1024 items at the cfg5 shape span several chunks"""
    import bench
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == "512"
    st = Setup(S, 1, 16, None, 1, mods=bench.CFG5_PRIMES)
    ctx, n, k, count = st.ctx, st.n, st.k, 1024
    u, e = st.asym_samples(count)
    pl = st.plains(k, count)
    ct = ctx.alloc(count * 2 * k * n)
    ctx.chunk_log()
    ctx.encrypt(k, st.d_pk, ctx.upload(pl), ctx.upload_i32(u), ctx.upload_i32(e), count, ct)
    log = ctx.chunk_log()
    assert log and log[-1][0] == count and log[-1][1] < count, log
    seeds, es = st.sym_samples(count)
    cs = ctx.alloc(count * 2 * k * n)
    ctx.encrypt_symmetric(k, st.d_sk, ctx.upload(pl), seeds, ctx.upload_i32(es), count, cs, save_seed=True)
    log = ctx.chunk_log()
    assert log and log[-1][0] == count and log[-1][1] < count, log
    item = 2 * k * n
    ctx.synchronize()
    for i in (0, 1, 511, 700, 1023):
        one = np.empty(item, dtype=np.uint64)
        for buf, want_fn in ((ct, lambda: st.encrypt(k, u[i:i + 1], e[i:i + 1], pl[i:i + 1], 1)),
                             (cs, lambda: st.encrypt_sym(k, seeds[i:i + 1], es[i:i + 1], pl[i:i + 1], 1, True))):
            assert S.lib().sealhip_memcpy_d2h(ctx.handle, one.ctypes.data, buf.ptr + i * item * 8, item * 8) == 0
            assert np.array_equal(one.reshape(1, 2, k, n), want_fn()), i
    print("BATCH_OK")


def test_batch_spans_arena_chunks():
    # (not run_arena_child: a 512 MB arena, and the child imports this module instead of running it)
    env = dict(os.environ, SEALHIP_WORKSPACE_MB="512")
    code = "import sys; sys.path[:0] = %r; import test_gpu_encryptor as T; T._batch_child()" % (
        [HERE, ROOT, os.path.join(ROOT, "gemini-seal_amd")],)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "BATCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_errors_on_device(S):
    st = Setup(S, 1, 12, [55, 55, 55], 1)
    L, h, n, k = S.lib(), st.ctx.handle, st.n, st.k
    u, e = st.asym_samples(1)
    du, de = st.ctx.upload_i32(u), st.ctx.upload_i32(e)
    ct = st.ctx.alloc(2 * st.n_key * n)
    pl = st.ctx.upload(st.plains(k, 1))
    seeds = np.zeros(8, dtype=np.uint64)
    enc = L.sealhip_encryptor_encrypt
    sym = L.sealhip_encryptor_encrypt_symmetric
    assert enc(h, k, None, pl.ptr, n, du.ptr, de.ptr, 1, ct.ptr) == S.E_POINTER
    assert enc(h, k, st.d_pk.ptr, pl.ptr, n, None, de.ptr, 1, ct.ptr) == S.E_POINTER
    assert enc(h, k, st.d_pk.ptr, pl.ptr, n, du.ptr, None, 1, ct.ptr) == S.E_POINTER
    assert enc(h, k, st.d_pk.ptr, pl.ptr, n, du.ptr, de.ptr, 1, None) == S.E_POINTER
    assert sym(h, k, None, pl.ptr, n, seeds.ctypes.data, de.ptr, 0, 1, ct.ptr) == S.E_POINTER
    assert sym(h, k, st.d_sk.ptr, pl.ptr, n, None, de.ptr, 0, 1, ct.ptr) == S.E_POINTER
    for bad in (0, st.n_key + 1):
        assert enc(h, bad, st.d_pk.ptr, None, 0, du.ptr, de.ptr, 1, ct.ptr) == S.E_INVALIDARG
        assert sym(h, bad, st.d_sk.ptr, None, 0, seeds.ctypes.data, de.ptr, 0, 1, ct.ptr) == S.E_INVALIDARG
    assert "parms_id is not valid" in S.lib().sealhip_last_error_string().decode()
    # a BFV plaintext at a level other than the first
    for bad in (1, st.n_key):
        assert enc(h, bad, st.d_pk.ptr, pl.ptr, n, du.ptr, de.ptr, 1, ct.ptr) == S.E_INVALIDARG
        assert "plain is not valid for encryption parameters" in S.lib().sealhip_last_error_string().decode()
        assert sym(h, bad, st.d_sk.ptr, pl.ptr, n, seeds.ctypes.data, de.ptr, 0, 1, ct.ptr) == S.E_INVALIDARG
    # count = 0: S_OK, nothing written
    guard = np.full(2 * k * n, 7, dtype=np.uint64)
    ct0 = st.ctx.upload(guard)
    assert enc(h, k, st.d_pk.ptr, pl.ptr, n, du.ptr, de.ptr, 0, ct0.ptr) == S.S_OK
    assert sym(h, k, st.d_sk.ptr, pl.ptr, n, seeds.ctypes.data, de.ptr, 1, 0, ct0.ptr) == S.S_OK
    assert np.array_equal(ct0.download(), guard)
    # a CKKS plaintext at the key level is not valid (no key-level plaintexts)
    sc = Setup(S, 2, 12, [55, 55, 55], 1)
    plk = sc.ctx.upload(sc.plains(sc.n_key, 1))
    ctk = sc.ctx.alloc(2 * sc.n_key * sc.n)
    assert L.sealhip_encryptor_encrypt(sc.ctx.handle, sc.n_key, sc.d_pk.ptr, plk.ptr, 0, du.ptr, de.ptr, 1,
                                       ctk.ptr) == S.E_INVALIDARG
    # the seeded save refuses a ring too small for the seed, and a size other than 2
    info = S.CiphertextInfo()
    for j in range(4):
        info.parms_id[j] = ((PID[0] + k,) + PID[1:])[j]
    info.is_ntt_form, info.size, info.coeff_modulus_size, info.poly_modulus_degree, info.scale = 0, 3, k, n, 1.0
    need = C.c_size_t(0)
    assert L.sealhip_ciphertext_save_seeded(h, C.addressof(info), ct.ptr, seeds.ctypes.data, None, 0,
                                            C.byref(need)) == S.E_INVALIDARG
    assert L.sealhip_ciphertext_save_seeded(h, C.addressof(info), ct.ptr, None, None, 0, C.byref(need)) == S.E_POINTER


def test_cpp_encryptor_on_device(S, tmp_path):
    """host/evaluator.hpp's Encryptor (public key, secret key, seeded) into its Decryptor: digests of the ciphertext words
    against the oracle compositions on the same samples, and the seeded stream against oracle/wire_format.py"""
    W = wire()
    st = Setup(S, 1, 10, [50, 50, 55, 60], 2)
    n, k, count = st.n, st.k, 3
    pl = st.plains(k, count)
    pl[0, n // 2:] = 0  # handed over short: the Encryptor zero-pads it
    u, e = st.asym_samples(count)
    seeds, es = st.sym_samples(count + 1)
    pid = (PID[0] + k,) + PID[1:]
    asym_words = np.concatenate([u[:, None, :], e], axis=1).astype(np.int64).view(np.uint64)  # count x 3 x N
    sym_words = np.concatenate([seeds, es.astype(np.int64).view(np.uint64)], axis=1)  # (count + 1) x (8 + N)
    head = [1, st.logn, st.n_key, st.nsp, st.t] + st.mods
    blob = np.concatenate([np.array(head, np.uint64), st.cl.sk.reshape(-1), st.pk.reshape(-1), np.array([count], np.uint64),
                           pl.reshape(-1), asym_words.reshape(-1), sym_words.reshape(-1), np.array(pid, np.uint64)])
    path, stream_path = str(tmp_path / "in.bin"), str(tmp_path / "seeded.bin")
    blob.astype(np.uint64).tofile(path)
    exe = compile_cpp(tmp_path, "host_adapter_encrypt_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", path, stream_path, timeout=300)
    lines = stdout.split("\n")
    for key in ("decrypt_asym=ok", "decrypt_sym=ok", "decrypt_seeded=ok", "meta=ok"):
        assert key in lines, stdout
    for i in range(count):
        want = st.expected_asym(k, u[i], e[i], pl[i])
        assert "asym %d %d" % (i, O.fnv(want)) in lines, (i, stdout)
        want = st.expected_sym(k, seeds[i], es[i], pl[i], False)
        assert "sym %d %d" % (i, O.fnv(want)) in lines, (i, stdout)
    want = st.expected_sym(k, seeds[count], es[count], pl[1], True)
    assert "seeded %d" % O.fnv(want) in lines, stdout
    with open(stream_path, "rb") as f:
        raw = f.read()
    assert raw == W.save_ciphertext(pid, False, 2, n, k, 1.0, want[0].reshape(-1), seed=seeds[count].tobytes())
