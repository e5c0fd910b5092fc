"""RLWE samples drawn on the device from seeds (sealhip_sample_polys, sealhip_sample_polys_split, sealhip_debug_sample_map,
sealhip_generate_secret_key). The device's words equal the numpy restatement of the rule
(tests/sample_ref.py, pinned to the host sampler by tests/test_sample_host.py) at every shape where the kernel's indexing
changes; the map functions are driven across every threshold; and a whole session -- secret key, public key, key-switch
keys, encryptions -- made from seeds alone equals the existing entries fed the restatement's samples, decrypts, and
evaluates."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import noise_ref as NR
import sample_ref as R
from support import S, compile_cpp, run_exe

pytestmark = pytest.mark.gpu

T = 786433  # prime, = 1 mod 2^18
KINDS = [(1, 0), (0, 1), (1, 2), (0, 3), (2, 2)]
MAX_POLYS = 4
SENTINEL = -1234567


@functools.lru_cache(maxsize=None)
def ring(logn):
    """one device context per ring, and the seeds and stream words its cases share (computed once, never modified)"""
    import sealhip

    n = 1 << logn
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, O.coeff_modulus_create(n, [30, 30]), 1, 0)
    rng = np.random.default_rng(7000 + logn)
    seeds = rng.integers(0, 2**64, size=(67, 8), dtype=np.uint64, endpoint=False)
    seeds[1] = 0
    seeds[2] = 2**64 - 1
    words = np.stack([R.stream_words(sealhip, s, MAX_POLYS * n) for s in seeds])
    words.setflags(write=False)
    return ctx, seeds, words


def restated(logn, count, nt, nn):
    _, _, words = ring(logn)
    n = 1 << logn
    out = np.empty((count, nt + nn, n), dtype=np.int32)
    out[:, :nt] = R.ternary_map(words[:count, : nt * n]).reshape(count, nt, n)
    out[:, nt:] = R.noise_map(words[:count, nt * n : (nt + nn) * n]).reshape(count, nn, n)
    return out


def download_i32(buf, count):
    return buf.download().view(np.int32)[:count].copy()


@pytest.mark.parametrize("count", [1, 3, 67])
@pytest.mark.parametrize("logn", [3, 6, 9, 10, 12, 16])
def test_sample_polys_equals_the_restatement(S, logn, count):
    """log N 3: a polynomial is one leaf; 6: several polynomials share one partial buffer; 9: a polynomial is one buffer;
    16: a (1, 2) item spans 384 buffers. Stride 0 (with N < 512 item i + 1 starts right after item i's partial buffer: its
    first words must be its own) and a padded stride whose sentinel words survive; the split layout gives the same samples."""
    ctx, seeds, _ = ring(logn)
    n = 1 << logn
    for nt, nn in KINDS:
        want = restated(logn, count, nt, nn)
        item = (nt + nn) * n
        out = ctx.alloc(count * item // 2)
        ctx.sample_polys(seeds[:count], nt, nn, out)
        got = download_i32(out, count * item).reshape(want.shape)
        assert np.array_equal(got, want), (logn, count, nt, nn, "stride 0")
        if count == 67 and logn == 16:
            continue  # (the padded and split forms run the same kernel: the smaller counts cover them at this ring)
        stride = item + 12
        padded = ctx.upload(np.full(count * stride, SENTINEL, dtype=np.int32).view(np.uint64))
        ctx.sample_polys(seeds[:count], nt, nn, padded, stride)
        got = download_i32(padded, count * stride).reshape(count, stride)
        assert np.array_equal(got[:, :item].reshape(want.shape), want), (logn, count, nt, nn, "padded")
        assert np.all(got[:, item:] == SENTINEL), (logn, count, nt, nn, "sentinel")
        tern = ctx.upload(np.full(max(2, count * nt * n), SENTINEL, dtype=np.int32).view(np.uint64))
        noise = ctx.upload(np.full(max(2, count * nn * n), SENTINEL, dtype=np.int32).view(np.uint64))
        ctx.sample_polys_split(seeds[:count], nt, nn, tern if nt else None, noise if nn else None)
        assert np.array_equal(download_i32(tern, count * nt * n).reshape(count, nt, n), want[:, :nt])
        assert np.array_equal(download_i32(noise, count * nn * n).reshape(count, nn, n), want[:, nt:])
        for b in (out, padded, tern, noise):
            b.free()


def test_sample_polys_empty_batch_and_checks(S):
    ctx, seeds, _ = ring(6)
    out = ctx.upload(np.full(3 * 64, SENTINEL, dtype=np.int32).view(np.uint64))
    ctx.sample_polys(seeds[:0], 1, 2, out)  # count 0: S_OK, nothing launched
    assert np.all(download_i32(out, 3 * 64) == SENTINEL)
    with pytest.raises(ValueError):
        ctx.sample_polys(seeds[:1], 0, 0, out)
    with pytest.raises(ValueError):
        ctx.sample_polys(seeds[:1], 16, 1, out)
    with pytest.raises(ValueError):
        ctx.sample_polys(seeds[:1], 1, 2, out, 3 * 64 - 4)
    with pytest.raises(ValueError, match="aligned"):
        ctx.sample_polys(seeds[:1], 1, 2, out.ptr + 8)


def test_debug_sample_map_at_every_threshold(S):
    """for every m: r = T_m - 1, T_m and 2^63 - 1, with either sign bit, give magnitudes m, m + 1 and 19 with that sign
    (magnitude 0 is 0 either way); the ternary map at its two boundaries and the ends of the range"""
    ctx, _, _ = ring(6)
    Tm = R.thresholds()
    words, want = [], []
    for m, t in enumerate(Tm):
        for r, mag in ((t - 1, m), (t, m + 1), ((1 << 63) - 1, 19)):
            for sign in (0, 1):
                words.append((r << 1) | sign)
                want.append(-mag if sign else mag)
    words += [0, 1]
    want += [0, 0]
    got = ctx.debug_sample_map(np.array(words, dtype=np.uint64), 1)
    assert got.tolist() == want
    assert np.array_equal(got, R.noise_map(np.array(words, dtype=np.uint64)))
    third, two_thirds = (1 << 64) // 3, (1 << 65) // 3
    tw = [0, third, third + 1, two_thirds, two_thirds + 1, (1 << 64) - 1]
    assert ctx.debug_sample_map(np.array(tw, dtype=np.uint64), 0).tolist() == [-1, -1, 0, 0, 1, 1]
    with pytest.raises(ValueError, match="kind"):
        ctx.debug_sample_map(np.array(tw, dtype=np.uint64), 2)


def lifted_ntt(ref, s, n_key):
    """KeyGenerator::generate_sk's lift and transform on the oracle: n_key x N words"""
    n = s.size
    sk = np.zeros((n_key, n), dtype=np.uint64)
    s8 = np.ascontiguousarray(s, dtype=np.int8)
    O.lib().ref_small_poly_to_rns(C.byref(ref.c), s8.ctypes.data, n_key, 1, O.ptr(sk))
    return sk


@pytest.mark.parametrize("nsp", [1, 2])
@pytest.mark.parametrize("logn", [3, 12])
def test_generate_secret_key_equals_lift_and_oracle_ntt(S, logn, nsp):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [40, 41, 42, 50] if logn == 12 else [20, 21, 22, 23])
    ref = O.RefContext(2, logn, mods, nsp=nsp)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, nsp, 0)
    for seed in (np.zeros(8, dtype=np.uint64), np.arange(8, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)):
        s = R.sample_polys(S, seed, n, 1, 0)[0, 0]
        assert set(np.unique(s)) <= {-1, 0, 1}
        got = ctx.generate_secret_key(seed).download((len(mods), n))
        assert np.array_equal(got, lifted_ntt(ref, s, len(mods))), (logn, nsp)
    ctx.close()


def sparse_times(m, t, n):
    """m(x) (1 + 2 x^3) in Z_t[x] / (x^N + 1)"""
    shifted = np.concatenate([(t - m[n - 3 :]) % t, m[: n - 3]])
    return (m + 2 * shifted) % t


@pytest.mark.parametrize("scheme", [1, 2])
def test_session_from_seeds_alone(S, scheme):
    """A secret key from a seed, then a public key, a relinearization key and a Galois key whose noise is sampled on the
    device: every word equals the existing entries fed the restatement's samples. Public-key and secret-key encryptions
    from device samples equal sealhip_encryptor_encrypt / _encrypt_symmetric fed the restatement's samples; they decrypt
    (BFV: exactly, with the oracle's noise budget on those words; CKKS: to the plaintext plus small noise), and multiply +
    relinearize and one rotate_vector with the generated keys decrypt correctly."""
    logn, n, nsp = 12, 1 << 12, 1
    mods = O.coeff_modulus_create(n, [40, 40, 40, 50])
    n_key, k = len(mods), len(mods) - nsp
    t = T if scheme == 1 else 0
    bfv = scheme == 1
    # (STRICT: the mode whose key switch is the mathematically correct one, so that evaluated ciphertexts decrypt)
    ref = O.RefContext(scheme, logn, mods, nsp=nsp, t=t, mode=1)
    ctx = S.Context(scheme, logn, mods, nsp, t, mode=S.MODE_STRICT)
    ev = S.Evaluator(ctx)
    d = ctx.kswitch_digits(k)
    rng = np.random.default_rng(40 + scheme)
    seed = lambda *shape: rng.integers(0, 2**64, size=shape + (8,), dtype=np.uint64, endpoint=False)
    host = lambda seeds, nt, nn: R.sample_polys(S, seeds, n, nt, nn)

    def device_noise(seeds):  # (0, 1) per seed -> count x N int32 on the device
        seeds = np.asarray(seeds).reshape(-1, 8)
        buf = ctx.alloc(seeds.shape[0] * n // 2)
        ctx.sample_polys(seeds, 0, 1, buf)
        return buf

    # ---- secret key
    sk_seed = seed()
    d_sk = ctx.generate_secret_key(sk_seed)
    sk = d_sk.download((n_key, n))
    s = host(sk_seed, 1, 0)[0, 0]
    assert np.array_equal(sk, lifted_ntt(ref, s, n_key))
    cl = O.Client(ref, seed=1)
    cl.s, cl.sk = s.astype(np.int8), sk
    pw = ctx.upload(cl.sk_powers(2))

    # ---- public key: encrypt_zero_symmetric at the key level, c_1 from one seed, the noise from another
    pk_c1, pk_noise = seed(), seed()
    assert not np.array_equal(pk_c1, pk_noise)
    a = ctx.alloc(n_key * n)
    ctx.expand_seeds(n_key, pk_c1, a)
    pk, pk_fed = ctx.alloc(2 * n_key * n), ctx.alloc(2 * n_key * n)
    ctx.encrypt_zero_symmetric(n_key, True, a, device_noise(pk_noise), d_sk, 1, pk)
    ctx.encrypt_zero_symmetric(n_key, True, a, ctx.upload_i32(host(pk_noise, 0, 1)), d_sk, 1, pk_fed)
    assert np.array_equal(pk.download(), pk_fed.download())

    # ---- key-switch keys: one relinearization key, one Galois key
    elt = ctx.galois_elt_from_step(1)
    rk_c1, rk_noise, gk_c1, gk_noise = seed(1, d), seed(1, d), seed(1, d), seed(1, d)
    rk = ctx.generate_relin_keys(d_sk, 1, rk_c1, device_noise(rk_noise))
    gk = ctx.generate_galois_keys(d_sk, [elt], gk_c1, device_noise(gk_noise))
    rk_fed = ctx.generate_relin_keys(d_sk, 1, rk_c1, ctx.upload_i32(host(rk_noise, 0, 1)))
    gk_fed = ctx.generate_galois_keys(d_sk, [elt], gk_c1, ctx.upload_i32(host(gk_noise, 0, 1)))
    ctx.set_parms_id(n_key, (1, 2, 3, 4))
    assert S.save_kswitch_keys(ctx, rk) == S.save_kswitch_keys(ctx, rk_fed)
    assert S.save_kswitch_keys(ctx, gk) == S.save_kswitch_keys(ctx, gk_fed)

    # ---- plaintexts
    count = 3
    if bfv:
        plain_host = rng.integers(0, t, size=(count, n), dtype=np.uint64)
        plain = ctx.upload(plain_host)
    else:
        scale = 2.0**30
        values = rng.uniform(-1, 1, size=(count, n // 2)) + 1j * rng.uniform(-1, 1, size=(count, n // 2))
        plain = ctx.ckks_encode(values, k, scale)
        plain_host = plain.download((count, k, n))

    # ---- public-key encryption: (1, 2) = u, e_0, e_1 per item
    enc_seeds = seed(count)
    u, e = ctx.alloc(count * n // 2 + 1), ctx.alloc(count * n)
    ctx.sample_polys_split(enc_seeds, 1, 2, u, e)
    ct_pk, ct_pk_fed = ctx.alloc(count * 2 * k * n), ctx.alloc(count * 2 * k * n)
    ctx.encrypt(k, pk, plain, u, e, count, ct_pk)
    fed = host(enc_seeds, 1, 2)
    ctx.encrypt(k, pk, plain, ctx.upload_i32(fed[:, 0]), ctx.upload_i32(fed[:, 1:]), count, ct_pk_fed)
    assert np.array_equal(ct_pk.download(), ct_pk_fed.download())

    # ---- secret-key encryption: c_1's seed, and a separate noise seed sampled as (0, 1)
    sym_c1, sym_noise = seed(count), seed(count)
    ct_sk, ct_sk_fed = ctx.alloc(count * 2 * k * n), ctx.alloc(count * 2 * k * n)
    ctx.encrypt_symmetric(k, d_sk, plain, sym_c1, device_noise(sym_noise), count, ct_sk)
    ctx.encrypt_symmetric(k, d_sk, plain, sym_c1, ctx.upload_i32(host(sym_noise, 0, 1)[:, 0]), count, ct_sk_fed)
    assert np.array_equal(ct_sk.download(), ct_sk_fed.download())

    # ---- decrypt
    def decrypted(ct, size=2):
        out = ctx.alloc(count * (n if bfv else k * n))
        ctx.decrypt(ct, size, k, count, pw, not bfv, out)
        return out

    def ckks_close(plain_buf, want, scale_, tol):
        got = ctx.ckks_decode(plain_buf, k, count, scale_)
        assert np.max(np.abs(got - want)) < tol, np.max(np.abs(got - want))

    for ct in (ct_pk, ct_sk):
        if bfv:
            assert np.array_equal(decrypted(ct).download((count, n)), plain_host)
            words = ct.download((count, 2, k, n))
            budgets = ctx.invariant_noise_budget(ct, 2, k, count, pw)
            for i in range(count):
                dot = np.zeros((k, n), dtype=np.uint64)
                O.lib().ref_dot_product_ct_sk(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(words[i])), 2, 0,
                                              O.ptr(cl.sk_powers(1)), O.ptr(dot))
                assert int(budgets[i]) == NR.ref_noise_budget(dot, mods[:k], t) > 0
        else:
            ckks_close(decrypted(ct), values, scale, 1e-3)

    # ---- multiply + relinearize, and one rotation, with the generated keys
    prod = ctx.alloc(count * 3 * k * n)
    if bfv:
        f = np.zeros(n, dtype=np.uint64)
        f[0], f[3] = 1, 2
        f_ct = ctx.alloc(2 * k * n)
        one_seed = seed(1)
        u1, e1 = ctx.alloc(n // 2), ctx.alloc(n)
        ctx.sample_polys_split(one_seed, 1, 2, u1, e1)
        ctx.encrypt(k, pk, ctx.upload(f), u1, e1, 1, f_ct)
        fs = ctx.upload(np.tile(f_ct.download(), count))
        ev.multiply(ct_pk, 2, fs, 2, k, count, prod)
    else:
        ev.multiply(ct_pk, 2, ct_sk, 2, k, count, prod)
    ev.relinearize_inplace(prod, 3, k, count, rk)
    lin = ctx.upload(np.ascontiguousarray(prod.download((count, 3, k, n))[:, :2]))
    if bfv:
        got = decrypted(lin).download((count, n))
        for i in range(count):
            assert np.array_equal(got[i], sparse_times(plain_host[i], t, n)), i
    else:
        ckks_close(decrypted(lin), values * values, scale * scale, 1e-3)
    rot = ctx.upload(ct_sk.download())
    ev.rotate_vector_native(rot, k, count, 1, {elt: gk[0]})
    got = decrypted(rot)
    if bfv:
        got = got.download((count, n))
        for i in range(count):
            want = np.zeros(n, dtype=np.uint64)
            O.lib().ref_apply_galois(O.ptr(np.ascontiguousarray(plain_host[i])), logn, elt, C.byref(O.modulus(t)), O.ptr(want))
            assert np.array_equal(got[i], want), i
    else:
        moved = np.zeros((count, k, n), dtype=np.uint64)
        for i in range(count):
            for r in range(k):
                O.lib().ref_apply_galois_ntt(O.ptr(np.ascontiguousarray(plain_host[i, r])), logn, elt, O.ptr(moved[i, r]))
        want = ctx.ckks_decode(ctx.upload(moved), k, count, scale)
        assert np.max(np.abs(ctx.ckks_decode(got, k, count, scale) - want)) < 1e-3
    ctx.close()


# ---------------------------------------------------------------- through the C++ adapter
@pytest.fixture(scope="module")
def adapter_exe(tmp_path_factory):
    return compile_cpp(tmp_path_factory.mktemp("sample_adapter"), "host_adapter_sample_check.cpp", link_sealhip=True, opt="-O1")


def seed_number(i):
    """seed number i of the check program's seed source"""
    mask = (1 << 64) - 1
    return np.array([((0x5EED000000000000 + i + j) * 0x9E3779B97F4A7C15) & mask for j in range(8)], dtype=np.uint64)


@pytest.mark.parametrize("scheme", [1, 2])
def test_cpp_adapter_with_a_seed_source(S, adapter_exe, tmp_path, scheme):
    """tests/host_adapter_sample_check.cpp on the device: KeyGenerator::generate_secret_key, public_key and relin_keys and
    resident Encryptor::encrypt / encrypt_symmetric with a seed source draw 1, 2, 2 per digit, 1 and 2 seeds in that order,
    no noise seed is in the seeded save, the sample scratch reads back zero; and every word they make equals the C ABI
    entries fed the restatement's samples of those seeds (the words of test_session_from_seeds_alone's construction)."""
    logn, n, nsp = 12, 1 << 12, 1
    mods = O.coeff_modulus_create(n, [40, 40, 40, 50])
    n_key, k = len(mods), len(mods) - nsp
    bfv = scheme == 1
    t = T if bfv else 0
    pid = (0x7171, 0x8282, 0x9393, 0xA4A4)
    rng = np.random.default_rng(90 + scheme)
    if bfv:
        plain_host = rng.integers(0, t, size=n, dtype=np.uint64)
    else:
        plain_host = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods[:k]])
    path = str(tmp_path / "input.bin")
    np.concatenate([np.array([scheme, logn, n_key, nsp, t] + mods + list(pid), dtype=np.uint64),
                    plain_host.reshape(-1)]).astype("<u8").tofile(path)
    stdout = run_exe(adapter_exe, "0", path, timeout=300)
    for line in ("seeded save ok", "scratch zero ok", "sample adapter ok"):
        assert line in stdout, stdout
    ctx = S.Context(scheme, logn, mods, nsp, t)
    ctx.set_parms_id(n_key, pid)
    d = ctx.kswitch_digits(k)
    assert "seeds drawn %d" % (3 + 2 * d + 3) in stdout, stdout
    host = lambda seeds, nt, nn: R.sample_polys(S, seeds, n, nt, nn)
    d_sk = ctx.generate_secret_key(seed_number(0))
    assert "sk digest %016x" % O.fnv(d_sk.download()) in stdout, stdout
    a, pk = ctx.alloc(n_key * n), ctx.alloc(2 * n_key * n)
    ctx.expand_seeds(n_key, seed_number(1), a)
    ctx.encrypt_zero_symmetric(n_key, True, a, ctx.upload_i32(host(seed_number(2), 0, 1)), d_sk, 1, pk)
    assert "pk digest %016x" % O.fnv(pk.download()) in stdout, stdout
    c1 = np.stack([seed_number(3 + 2 * j) for j in range(d)])
    noise = np.stack([seed_number(4 + 2 * j) for j in range(d)])
    rk = ctx.generate_relin_keys(d_sk, 1, c1, ctx.upload_i32(host(noise, 0, 1)))
    stream = S.save_kswitch_keys(ctx, rk)
    assert "rk digest %016x" % O.fnv(np.frombuffer(stream[: len(stream) // 8 * 8], dtype=np.uint64)) in stdout, stdout
    first = 3 + 2 * d
    plain = ctx.upload(plain_host)
    fed = host(seed_number(first), 1, 2)
    ct = ctx.alloc(2 * k * n)
    ctx.encrypt(k, pk, plain, ctx.upload_i32(fed[:, 0]), ctx.upload_i32(fed[:, 1:]), 1, ct)
    assert "asym digest %016x" % O.fnv(ct.download()) in stdout, stdout
    ctx.encrypt_symmetric(k, d_sk, plain, seed_number(first + 1), ctx.upload_i32(host(seed_number(first + 2), 0, 1)), 1, ct)
    assert "sym digest %016x" % O.fnv(ct.download()) in stdout, stdout
    ctx.close()
