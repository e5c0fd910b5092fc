"""Relinearization and Galois keys generated on the device (sealhip_generate_relin_keys, sealhip_generate_galois_keys,
sealhip_kswitch_keys_save_seeded). Every word is compared with KeyGenerator::generate_one_kswitch_key (keygenerator.cpp:325-369)
restated from oracle entries only: ref_encrypt_zero_symmetric_given per digit with a = the oracle's expand_seed of the digit's
seed, then ref_multiply_uint_mod factors added with ref_multiply_poly_scalar_coeffmod / ref_add_poly_coeffmod on
ref_apply_galois_ntt / ref_dyadic_product_coeffmod new keys. The keys are read back through sealhip_kswitch_keys_save and
compared with oracle/wire_format.py's stream of the expected words."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O
from support import S, run_exe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PID = (0x1111, 0x2222, 0x3333, 0x4444)
T = 786433  # prime, = 1 mod 2^18: batching at every ring up to 2^16


def wire():
    spec = importlib.util.spec_from_file_location("wire_format", os.path.join(ROOT, "oracle", "wire_format.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    return W


class Setup:
    """(not a BaseSession: the oracle side and its client come first, the context gets parms_ids, there is no evaluator)"""

    def __init__(self, S, scheme, logn, bits, nsp, mode=0):
        self.n = n = 1 << logn
        self.logn, self.nsp = logn, nsp
        self.mods = O.coeff_modulus_create(n, bits)
        self.n_key = len(self.mods)
        self.k = self.n_key - nsp
        self.d = (self.k + nsp - 1) // nsp
        t = T if scheme == 1 else 0
        self.ref = O.RefContext(scheme, logn, self.mods, nsp=nsp, t=t, mode=mode)
        self.cl = O.Client(self.ref, seed=logn * 7 + nsp)
        self.ctx = S.Context(scheme, logn, self.mods, nsp, t, mode=mode)
        self.ctx.set_parms_id(self.n_key, PID)
        self.sk = self.ctx.upload(self.cl.sk)
        self.rng = np.random.default_rng(1000 * logn + 10 * nsp + scheme)

    def samples(self, n_keys):
        seeds = self.rng.integers(0, 2**64, size=(n_keys, self.d, 8), dtype=np.uint64, endpoint=False)
        noise = self.rng.integers(-41, 42, size=(n_keys, self.d, self.n), dtype=np.int32)
        return seeds, noise

    def rotated(self, elt):
        rot = np.zeros((self.n_key, self.n), dtype=np.uint64)
        for r in range(self.n_key):
            O.lib().ref_apply_galois_ntt(O.ptr(self.cl.sk[r]), self.logn, elt, O.ptr(rot[r]))
        return rot

    def expected(self, new_key, seeds, noise):
        """generate_one_kswitch_key from oracle entries: d x 2 x n_key x N"""
        L, c = O.lib(), self.ref.c
        key = np.zeros((self.d, 2, self.n_key, self.n), dtype=np.uint64)
        for j in range(self.d):
            a = np.ascontiguousarray(O.expand_seed(seeds[j], self.mods, self.n))
            e = np.ascontiguousarray(noise[j], dtype=np.int32)
            ct = np.zeros((2, self.n_key, self.n), dtype=np.uint64)
            L.ref_encrypt_zero_symmetric_given(C.byref(c), self.n_key, O.ptr(self.cl.sk), 1, O.ptr(a), e.ctypes.data, O.ptr(ct))
            for r in range(j * self.nsp, min((j + 1) * self.nsp, self.k)):
                f = 1
                for s in range(self.nsp):
                    f = L.ref_multiply_uint_mod(f, self.mods[self.k + s], C.byref(c.key_mod[r]))
                tmp = np.zeros(self.n, dtype=np.uint64)
                src = np.ascontiguousarray(new_key[r])
                L.ref_multiply_poly_scalar_coeffmod(O.ptr(src), self.n, f, C.byref(c.key_mod[r]), O.ptr(tmp))
                L.ref_add_poly_coeffmod(O.ptr(ct[0, r]), O.ptr(tmp), self.n, C.byref(c.key_mod[r]), O.ptr(ct[0, r]))
            key[j] = ct
        return key

    def stream(self, W, keys):
        return W.save_kswitch_keys(PID, [list(k) if k is not None else [] for k in keys], self.n, self.n_key)

    def seeded_stream(self, W, keys, seeds):
        """what Serializable<KSwitchKeys>::save writes: per digit save_ciphertext(..., seed=...) with the words of c_0, wrapped
        as save_kswitch_keys wraps the digits (kswitchkeys.cpp:43-85, ciphertext.cpp:189-208)"""
        import struct

        body = struct.pack("<4Q", *PID) + struct.pack("<Q", len(keys))
        for key, sd in zip(keys, seeds):
            body += struct.pack("<Q", len(key))
            for j, dig in enumerate(key):
                body += W.save_ciphertext(PID, True, 2, self.n, self.n_key, 1.0, dig[0].reshape(-1),
                                          seed=np.ascontiguousarray(sd[j], dtype="<u8").tobytes())
        return W.header(16 + len(body)) + body


def galois_elts(n):
    """3, 2N - 1, the elements of steps +-1 and +-2^i (GaloisTool::get_elts_all's list), a random odd element"""
    out = [3, 2 * n - 1]
    m = 2 * n
    for step in [1, -1] + [s for i in range(1, max(1, (n // 2).bit_length() - 1)) for s in (1 << i, -(1 << i))]:
        if abs(step) >= n // 2:
            continue
        s = step if step > 0 else n // 2 + step
        out.append(pow(5, s, m))
    rng = np.random.default_rng(n)
    out.append(int(rng.integers(0, n)) * 2 + 1)
    uniq = []
    for e in out:
        if e not in uniq:
            uniq.append(e)
    return uniq


# (scheme, logn, bit sizes, nsp): every prime class of the NTT dispatch (< 2^50 on the FP64 pipe, 55- and 60-bit),
# nsp 1..3 with n_ct not a multiple of nsp (a short last digit)
CASES = [
    (1, 3, [20, 30, 40], 1),
    (2, 3, [40, 50, 55, 60], 2),
    (1, 8, [30, 45, 55, 60, 60], 2),
    (2, 8, [40, 40, 40, 40, 50, 55, 60], 3),
    (2, 12, [55, 55, 55, 60], 1),
    (1, 12, [36, 36, 37, 60, 60], 3),
    (2, 14, [50, 50, 50, 60, 60], 2),
    (1, 14, [60, 60, 60, 60], 1),
    (2, 15, [45, 55, 60, 60, 60, 60, 60], 3),
    (1, 15, [40, 40, 40, 60, 60], 2),
    (2, 16, [55, 60, 60], 1),
    (1, 16, [45, 50, 60, 60, 60], 2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-logn%d-k%d-nsp%d" % (c[0], c[1], len(c[2]), c[3]))
def test_generated_keys_word_for_word(S, case):
    scheme, logn, bits, nsp = case
    st = Setup(S, scheme, logn, bits, nsp)
    W = wire()
    elts = galois_elts(st.n)
    if logn >= 15:
        elts = elts[:3] + elts[-1:]  # 3, 2N - 1, step 1, a random element (the full list runs at logn 14 and below)
    seeds, noise = st.samples(len(elts))
    keys = st.ctx.generate_galois_keys(st.sk, elts, seeds, st.ctx.upload_i32(noise))
    exp = [st.expected(st.rotated(e), seeds[i], noise[i]) for i, e in enumerate(elts)]
    assert S.save_kswitch_keys(st.ctx, keys) == st.stream(W, exp), (case, "galois")
    powers = st.cl.sk_powers(4)
    for count in (1, 3):
        seeds, noise = st.samples(count)
        keys = st.ctx.generate_relin_keys(st.sk, count, seeds, st.ctx.upload_i32(noise))
        exp = [st.expected(powers[i + 1], seeds[i], noise[i]) for i in range(count)]
        assert S.save_kswitch_keys(st.ctx, keys) == st.stream(W, exp), (case, "relin", count)


def test_short_last_digit_shapes():
    """the CASES above include n_ct not a multiple of nsp for nsp = 2 and 3"""
    short = [(len(b) - nsp) % nsp for _, _, b, nsp in CASES if nsp > 1]
    assert any(short) and {2, 3} <= {nsp for _, _, b, nsp in CASES if (len(b) - nsp) % nsp}


def test_large_batch_and_seed_slack(S):
    """40 keys in one call (two assemble launches of 32 and 8), and the same words with every rejection sent through the
    seed expander's in-kernel continuation (sealhip_debug_seed_slack(0))"""
    st = Setup(S, 2, 10, [50, 55, 60, 60], 2)
    W = wire()
    elts = list(range(3, 3 + 2 * 40, 2))
    seeds, noise = st.samples(len(elts))
    dn = st.ctx.upload_i32(noise)
    exp = st.stream(W, [st.expected(st.rotated(e), seeds[i], noise[i]) for i, e in enumerate(elts)])
    keys = st.ctx.generate_galois_keys(st.sk, elts, seeds, dn)
    assert S.save_kswitch_keys(st.ctx, keys) == exp
    st.ctx.debug_seed_slack(0)
    try:
        keys = st.ctx.generate_galois_keys(st.sk, elts, seeds, dn)
        assert S.save_kswitch_keys(st.ctx, keys) == exp
    finally:
        st.ctx.debug_seed_slack(-1)


@pytest.mark.parametrize("scheme", [1, 2])
def test_seeded_stream(S, scheme):
    st = Setup(S, scheme, 12, [40, 55, 60, 60, 60], 2)
    W = wire()
    elts = [3, 2 * st.n - 1, 25]
    seeds, noise = st.samples(len(elts))
    keys = st.ctx.generate_galois_keys(st.sk, elts, seeds, st.ctx.upload_i32(noise), keep_seeds=True)
    exp = [st.expected(st.rotated(e), seeds[i], noise[i]) for i, e in enumerate(elts)]
    seeded = S.save_kswitch_keys_seeded(st.ctx, keys)
    assert seeded == st.seeded_stream(W, exp, seeds)
    # GaloisKeys slots: index (elt - 1) / 2, unused slots empty
    slots = [None] * st.n
    for e, k in zip(elts, keys):
        slots[(e - 1) // 2] = k
    full = S.save_kswitch_keys_seeded(st.ctx, slots)
    for e, k in zip(elts, keys):
        back = S.KSwitchKeys.from_stream(st.ctx, full, (e - 1) // 2)  # expands the seeds on the device
        assert S.save_kswitch_keys(st.ctx, [back]) == S.save_kswitch_keys(st.ctx, [k])
    # relin keys carry their seeds too; without keep_seeds the seeded save is refused
    seeds, noise = st.samples(2)
    rk = st.ctx.generate_relin_keys(st.sk, 2, seeds, st.ctx.upload_i32(noise), keep_seeds=True)
    powers = st.cl.sk_powers(3)
    exp = [st.expected(powers[i + 1], seeds[i], noise[i]) for i in range(2)]
    assert S.save_kswitch_keys_seeded(st.ctx, rk) == st.seeded_stream(W, exp, seeds)
    plain = st.ctx.generate_relin_keys(st.sk, 1, seeds[:1], st.ctx.upload_i32(noise[:1]))
    with pytest.raises(ValueError, match="no seeds"):
        S.save_kswitch_keys_seeded(st.ctx, plain)
    with pytest.raises(ValueError, match="no seeds"):
        S.save_kswitch_keys_seeded(st.ctx, [rk[0], None, plain[0]])


def test_edges(S):
    st = Setup(S, 1, 8, [30, 40, 60], 1)
    L = S.lib()
    seeds, noise = st.samples(3)
    dn = st.ctx.upload_i32(noise)
    out = (C.c_void_p * 3)(1, 2, 3)
    sp = seeds.ctypes.data
    # empty lists: nothing made, S_OK
    assert st.ctx.generate_galois_keys(st.sk, [], seeds[:0], dn) == []
    assert st.ctx.generate_relin_keys(st.sk, 0, seeds[:0], dn) == []
    # null pointers first
    el = (C.c_uint32 * 3)(3, 5, 7)
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_galois_keys(st.ctx.handle, st.sk.ptr, None, 3, sp, dn.ptr, 0, out))
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_relin_keys(st.ctx.handle, st.sk.ptr, 1, sp, None, 0, out))
    # invalid elements: no handle, every output NULL
    for bad in ([3, 4, 7], [3, 2 * st.n + 1, 5], [3, 5, 3], [0, 3, 5]):
        arr = (C.c_uint32 * 3)(*bad)
        out = (C.c_void_p * 3)(1, 2, 3)
        with pytest.raises(ValueError):
            S._check(L.sealhip_generate_galois_keys(st.ctx.handle, st.sk.ptr, arr, 3, sp, dn.ptr, 0, out))
        assert list(out) == [None, None, None]
    with pytest.raises(ValueError, match="invalid count"):
        st.ctx.generate_relin_keys(st.sk, 15, np.zeros((15, st.d, 8), np.uint64), dn)
    # BFV without batching (t not = 1 mod 2N)
    ctx = S.Context(1, 8, st.mods, 1, 65539)
    arr = (C.c_uint32 * 1)(3)
    out = (C.c_void_p * 1)(1)
    with pytest.raises(S.LogicError, match="batching"):
        S._check(L.sealhip_generate_galois_keys(ctx.handle, st.sk.ptr, arr, 1, sp, dn.ptr, 0, out))
    assert out[0] is None
    # relin keys need no batching
    rk = ctx.generate_relin_keys(st.sk, 1, seeds[:1], dn)
    assert rk[0].handle
    # a context without key switching (a single prime) cannot be created
    with pytest.raises(ValueError):
        S.Context(1, 8, st.mods[:1], 1, T)


def test_semantics_strict_bfv(S):
    """keys from the new entries, sk and encryptions from the oracle client, STRICT BFV: multiply + relinearize decrypts to the
    negacyclic product; rotate_vector by +-1, +-2^i (and 3, composed) with the galois_keys() set, and element 2N - 1, decrypt
    to m(x^elt)"""
    logn, n, t = 10, 1 << 10, T
    st = Setup(S, 1, logn, [45, 45, 45, 45, 45], 2, mode=1)
    ctx, cl, k = st.ctx, st.cl, st.k
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(9)
    m1 = rng.integers(0, t, size=n, dtype=np.uint64)
    m2 = rng.integers(0, t, size=n, dtype=np.uint64)
    pw = ctx.upload(cl.sk_powers(2))

    def dec(dct, size):
        dot = ctx.alloc(k * n)
        ctx.dot_product_ct_sk(dct, size, k, 1, pw, False, dot)
        out = ctx.alloc(n)
        ctx.decrypt_scale_and_round(k, dot, 1, out)
        return out.download((n,))

    seeds, noise = st.samples(1)
    rk = ctx.generate_relin_keys(st.sk, 1, seeds, ctx.upload_i32(noise))
    prod = ctx.alloc(3 * k * n)
    ev.multiply(ctx.upload(cl.encrypt_bfv(m1)), 2, ctx.upload(cl.encrypt_bfv(m2)), 2, k, 1, prod)
    ev.relinearize_inplace(prod, 3, k, 1, rk)
    c2 = ctx.upload(prod.download((3, k, n))[:2].copy())
    assert np.array_equal(dec(c2, 2), O.negacyclic_mod_t(m1, m2, t))
    # galois_keys(): get_elts_all (galois.cpp:102-127): 2N - 1 and 5^(+-2^i); 5^(N/4) = 5^(-N/4) is listed twice and made once
    elts = [2 * n - 1]
    for i in range(logn - 1):
        for e in (pow(5, 1 << i, 2 * n), pow(5, n // 2 - (1 << i), 2 * n)):
            if e not in elts:
                elts.append(e)
    assert len(elts) == 2 * (logn - 1)
    seeds, noise = st.samples(len(elts))
    gk = ctx.generate_galois_keys(st.sk, elts, seeds, ctx.upload_i32(noise))
    by_elt = dict(zip(elts, gk))
    # a rotation by `step` maps the plaintext polynomial m(x) to m(x^elt) (galois.cpp:144-186): in slots, the rows rotate by
    # `step`; elt 2N - 1 swaps the rows
    vals = rng.integers(0, t, size=n, dtype=np.uint64)
    ct = cl.encrypt_bfv(vals)

    def permuted(elt):
        idx = (np.arange(n, dtype=np.int64) * elt) % (2 * n)
        out = np.zeros(n, dtype=np.uint64)
        out[idx % n] = np.where(idx < n, vals, (t - vals) % t)
        return out

    for step in (1, -1, 2, -4, 16, 3):  # 3: rotate_vector's NAF composition of generated keys
        g = ctx.upload(ct)
        ev.rotate_vector_inplace(g, k, 1, step, by_elt)
        assert np.array_equal(dec(g, 2), permuted(ctx.galois_elt_from_step(step))), step
    g = ctx.upload(ct)
    ev.apply_galois_inplace(g, k, 1, 2 * n - 1, by_elt[2 * n - 1])
    assert np.array_equal(dec(g, 2), permuted(2 * n - 1))


def splitmix(state):
    state[0] = (state[0] + 0x9E3779B97F4A7C15) & (2**64 - 1)
    z = state[0]
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return z ^ (z >> 31)


def fnv(raw):
    """(not oracle_lib.fnv: over a byte stream whose length need not be whole words)"""
    h = 0xCBF29CE484222325
    for b in raw:
        h = ((h ^ b) * 0x100000001B3) & (2**64 - 1)
    return h


def test_cpp_keygenerator_on_device(S, tmp_path):
    """host/evaluator.hpp KeyGenerator: relin_keys(2), galois_keys(steps {1, -1}) and public_key() made from the same samples
    as the C ABI calls below give the same bytes"""
    from test_keygen_host import build_keygen_adapter

    import subprocess

    stdout = run_exe(build_keygen_adapter(tmp_path), "0", timeout=300)
    lines = dict(l.split(" digest ") for l in stdout.splitlines() if " digest " in l)
    mods = [1073738753, 1099511603713, 1152921504606830593, 1152921504606844417]
    n = 256
    ctx = S.Context(1, 8, mods, 2, T)
    ctx.set_parms_id(4, PID)
    st = [0x5EC2E7]
    sk = np.array([[splitmix(st) % q for _ in range(n)] for q in mods], dtype=np.uint64)
    dsk = ctx.upload(sk)
    ss = [0xCAFE]

    def sample(count):
        seeds, noise = [], []
        for _ in range(count):
            seeds.append([splitmix(ss) for _ in range(8)])
            noise.append([splitmix(ss) % 83 - 41 for _ in range(n)])
        return np.array(seeds, dtype=np.uint64), np.array(noise, dtype=np.int32)

    seeds, noise = sample(2)
    rk = ctx.generate_relin_keys(dsk, 2, seeds, ctx.upload_i32(noise))
    assert int(lines["relin_keys(2)"], 16) == fnv(S.save_kswitch_keys(ctx, rk))
    elts = [ctx.galois_elt_from_step(1), ctx.galois_elt_from_step(-1)]
    seeds, noise = sample(2)
    gk = dict(zip(elts, ctx.generate_galois_keys(dsk, elts, seeds, ctx.upload_i32(noise))))
    digest, lo, hi = lines["galois_keys(steps 1, -1)"].replace(" elts ", " ").split()
    assert (int(lo), int(hi)) == (min(elts), max(elts))
    assert int(digest, 16) == fnv(S.save_kswitch_keys(ctx, [gk[e] for e in sorted(elts)]))
    seeds, noise = sample(1)
    a = ctx.alloc(4 * n)
    ctx.expand_seeds(4, seeds, a)
    pk = ctx.alloc(2 * 4 * n)
    ctx.encrypt_zero_symmetric(4, True, a, ctx.upload_i32(noise), dsk, 1, pk)
    assert int(lines["public_key"], 16) == fnv(pk.download().astype("<u8").tobytes())
    assert "samples asked 5" in stdout
