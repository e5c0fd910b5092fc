"""Decryptor on the device: sealhip_decryptor_invariant_noise_budget against planted budgets and the restatement of
tests/noise_ref.py (rings 2^12..2^16, every limb instance of the kernel and both sides of each boundary, sizes 2 and 3,
55- and 60-bit primes, PARITY and STRICT, the extremes of the centring), a batch of 1024 items with distinct budgets,
sealhip_decryptor_decrypt bit-exact against the oracle (BFV and CKKS), the error codes, an end-to-end STRICT chain, and the
C++ Decryptor on the device."""
import ctypes as C

import numpy as np
import pytest

import noise_ref as R
import oracle_lib as O
from support import S, compile_cpp, run_exe

pytestmark = pytest.mark.gpu

T = 786433


def planted_items(n, q, rng):
    """(small targets, large targets) per item: the zero polynomial, norm (Q-1)/2 from W = (Q-1)/2 at coefficient 0 and from
    W = (Q+1)/2 at N-1, W = Q - 1 (norm 1), a mid-sized maximum at a random place, and the batch maximum in the last item"""
    half = (q - 1) // 2
    z = np.zeros(n, np.int64)
    small = rng.integers(-(1 << 20), 1 << 20, size=n)
    return [
        (z, {}),
        (small, {0: half}),
        (small, {n - 1: -half}),
        (z, {5 % n: -1}),
        (rng.integers(-1000, 1000, size=n), {int(rng.integers(0, n)): 1 << (q.bit_length() // 2)}),
        (rng.integers(-3, 3, size=n), {int(rng.integers(0, n)): half - 12345}),
    ]


def check_level(S, ctx, mods, logn, k, size, t, rng, pw_dev, restate=False):
    """planted budgets with c_1 = ... = 0: the dot product is c_0 whatever the key and the transform"""
    n = 1 << logn
    q = R.prod(mods[:k])
    items = planted_items(n, q, rng)
    cts, want = [], []
    for x, big in items:
        rows = R.planted_rows(x, big, mods[:k], t)
        if restate:
            assert R.ref_noise_budget(rows, mods[:k], t) == R.planted_budget(x, big, mods[:k])
        ct = np.zeros((size, k, n), dtype=np.uint64)
        ct[0] = rows
        cts.append(ct)
        want.append(R.planted_budget(x, big, mods[:k]))
    ct = np.ascontiguousarray(np.stack(cts))
    got = ctx.invariant_noise_budget(ctx.upload(ct), size, k, len(items), pw_dev)
    assert got.dtype == np.int32
    assert list(got) == want, (k, size, list(got), want)
    assert want[0] == q.bit_length() - 1 and want[3] == q.bit_length() - 2


RINGS = [(12, 2, 1 << 20), (13, 3, T), (14, 2, T), (15, 3, 1 << 16), (16, 2, T)]


@pytest.mark.parametrize("logn,size,t", RINGS)
def test_budget_rings(S, logn, size, t):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [55, 60, 55, 60])
    for mode in (S.MODE_PARITY, S.MODE_STRICT):
        ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=mode)
        rng = np.random.default_rng(logn * 3 + mode)
        pw = R.random_sk_powers(mods, logn, size - 1, rng)
        dpw = ctx.upload(pw)
        for k in (1, 3):
            check_level(S, ctx, mods, logn, k, size, t, rng, dpw, restate=(logn <= 13))
        # random c_1..: the restatement of the oracle's dot product (the transform in the context's mode)
        ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=mode)
        k = 3
        for x, big in planted_items(n, R.prod(mods[:k]), rng)[3:5]:
            rows = R.planted_rows(x, big, mods[:k], t)
            ct = R.ciphertext_with_dot(rows, size, pw, mods, logn, rng)
            dot = np.zeros((k, n), dtype=np.uint64)
            O.lib().ref_dot_product_ct_sk(C.byref(ref.c), k, O.ptr(ct), size, 0, O.ptr(pw), O.ptr(dot))
            got = ctx.invariant_noise_budget(ctx.upload(ct), size, k, 1, dpw)
            assert int(got[0]) == R.ref_noise_budget(dot, mods[:k], t)
        ctx.close()


# every limb instance (4 / 8 / 16 / 32 / 64) and both sides of each boundary, up to the top level of a 64-prime context
LEVELS = [1, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]


@pytest.mark.parametrize("bits,n_primes,mode,t", [(55, 64, 0, T), (60, 40, 1, 1 << 20)])
def test_budget_every_limb_instance(S, bits, n_primes, mode, t):
    logn, n = 12, 1 << 12
    mods = O.coeff_modulus_create(n, [bits] * n_primes)
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=mode)
    rng = np.random.default_rng(bits)
    dpw = ctx.upload(R.random_sk_powers(mods, logn, 2, rng))
    for i, k in enumerate(x for x in LEVELS if x <= n_primes):
        check_level(S, ctx, mods, logn, k, 2 + (i & 1), t, rng, dpw, restate=(k in (5, 17, 33)))
    check_level(S, ctx, mods, logn, n_primes, 3, t, rng, dpw)
    ctx.close()


def test_budget_batch_of_1024_distinct(S):
    """1024 ciphertexts at N=2^15, k=20: item i holds one planted coefficient of bit length i+1 at its own position and zeros
    elsewhere, so every item has its own budget; a maximum leaking across items or workgroups changes one"""
    logn, n, k, count = 15, 1 << 15, 20, 1024
    mods = O.coeff_modulus_create(n, [55] * (k + 1))
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, T)
    q = R.prod(mods[:k])
    tinv = pow(T, -1, q)
    vals = np.zeros((count, k), dtype=np.uint64)
    pos = np.array([(i * 7919) % n for i in range(count)], dtype=np.int64)
    want = []
    for i in range(count):
        x = (1 << i) + i if i else 1
        x = -x if i & 1 else x
        w = (x * tinv) % q
        vals[i] = [w % int(p) for p in mods[:k]]
        want.append(q.bit_length() - (i + 1) - 1)
    assert len(set(want)) == count and min(want) > 0
    one = np.zeros((2, k, n), dtype=np.uint64)
    ct = ctx.alloc(count * one.size)
    for i in range(count):
        one[0, :, pos[i]] = vals[i]
        S._check(S.lib().sealhip_memcpy_h2d(ctx.handle, ct.ptr + i * one.nbytes, one.ctypes.data, one.nbytes))
        one[0, :, pos[i]] = 0
    pw = ctx.upload(np.zeros((1, len(mods), n), dtype=np.uint64))
    got = ctx.invariant_noise_budget(ct, 2, k, count, pw)
    assert list(got) == want
    ct.free()
    ctx.close()


def test_budget_empty_batch(S):
    n = 1 << 12
    mods = O.coeff_modulus_create(n, [50, 50, 60])
    ctx = S.Context(S.SCHEME_BFV, 12, mods, 1, T)
    buf = ctx.alloc(16)
    assert ctx.invariant_noise_budget(buf, 2, 2, 0, buf).shape == (0,)
    ctx.decrypt(buf, 2, 2, 0, buf, False, buf)
    ctx.synchronize()
    ctx.close()


@pytest.mark.parametrize("size", [2, 3])
def test_decrypt_bit_exact(S, size):
    logn, n = 12, 1 << 12
    mods = O.coeff_modulus_create(n, [50, 50, 50, 60])
    L = O.lib()
    rng = np.random.default_rng(size)
    count = 3
    # BFV: dot product + decrypt_scale_and_round
    ref = O.RefContext(1, logn, mods, nsp=1, t=T)
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, T)
    pw = R.random_sk_powers(mods, logn, size - 1, rng)
    for k in (1, 3):
        ct = np.stack([np.stack([np.stack([rng.integers(0, int(p), size=n, dtype=np.uint64) for p in mods[:k]])
                                 for _ in range(size)]) for _ in range(count)])
        out = ctx.alloc(count * n)
        ctx.decrypt(ctx.upload(ct), size, k, count, ctx.upload(pw), False, out)
        got = out.download((count, n))
        for i in range(count):
            dot = np.zeros((k, n), dtype=np.uint64)
            L.ref_dot_product_ct_sk(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(ct[i])), size, 0, O.ptr(pw), O.ptr(dot))
            exp = np.zeros(n, dtype=np.uint64)
            assert L.ref_decrypt_scale_and_round(C.byref(ref.c), k, O.ptr(dot), O.ptr(exp)) == 0
            assert np.array_equal(got[i], exp), (k, i)
    dct = ctx.upload(np.zeros((2, 3, n), np.uint64))
    with pytest.raises(ValueError, match="cannot be in NTT form"):
        ctx.decrypt(dct, 2, 3, 1, ctx.upload(pw), True, ctx.alloc(n))
    with pytest.raises(ValueError):
        ctx.invariant_noise_budget(dct, 1, 3, 1, ctx.upload(pw))
    with pytest.raises(ValueError):
        ctx.invariant_noise_budget(dct, 2, 0, 1, ctx.upload(pw))
    with pytest.raises(ValueError):
        ctx.decrypt(dct, 17, 3, 1, ctx.upload(pw), False, ctx.alloc(n))
    with pytest.raises(TypeError):
        S._check(S.lib().sealhip_decryptor_invariant_noise_budget(ctx.handle, 3, dct.ptr, 2, 1, None, None))
    ctx.close()
    # CKKS: the dot product in NTT form is the plaintext
    ref = O.RefContext(2, logn, mods, nsp=1)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    for k in (1, 3):
        ct = np.stack([np.stack([np.stack([rng.integers(0, int(p), size=n, dtype=np.uint64) for p in mods[:k]])
                                 for _ in range(size)]) for _ in range(count)])
        out = ctx.alloc(count * k * n)
        ctx.decrypt(ctx.upload(ct), size, k, count, ctx.upload(pw), True, out)
        got = out.download((count, k, n))
        for i in range(count):
            dot = np.zeros((k, n), dtype=np.uint64)
            L.ref_dot_product_ct_sk(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(ct[i])), size, 1, O.ptr(pw), O.ptr(dot))
            assert np.array_equal(got[i], dot), (k, i)
    dct = ctx.upload(np.zeros((2, 3, n), np.uint64))
    with pytest.raises(ValueError, match="must be in NTT form"):
        ctx.decrypt(dct, 2, 3, 1, ctx.upload(pw), False, ctx.alloc(3 * n))
    with pytest.raises(S.LogicError, match="unsupported scheme"):
        ctx.invariant_noise_budget(dct, 2, 3, 1, ctx.upload(pw))
    ctx.close()


def test_strict_chain_end_to_end(S):
    """encrypt (oracle client), then multiply + relinearize on the device; after each step the device budget equals the
    restatement, does not increase, and while it is above 0 the device decrypt gives the plaintext arithmetic"""
    logn, n, t = 12, 1 << 12, T
    mods = O.coeff_modulus_create(n, [55, 55, 55, 60])
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    cl = O.Client(ref, seed=3)
    k = cl.k
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT)
    ev = S.Evaluator(ctx)
    rk = S.KSwitchKeys(ctx, cl.relin_key())
    pw = ctx.upload(cl.sk_powers(2))
    rng = np.random.default_rng(4)
    m = rng.integers(0, t, size=n, dtype=np.uint64)
    f = rng.integers(0, 3, size=n, dtype=np.uint64)
    ct = ctx.upload(cl.encrypt_bfv(m))
    fct = ctx.upload(cl.encrypt_bfv(f))
    expect, budgets = m, []
    for step in range(6):
        b = int(ctx.invariant_noise_budget(ct, 2, k, 1, pw)[0])
        assert b == R.ref_noise_budget(_dot(cl, ct.download((2, k, n))), mods[:k], t)
        if budgets:
            assert b <= budgets[-1], budgets
        budgets.append(b)
        out = ctx.alloc(n)
        ctx.decrypt(ct, 2, k, 1, pw, False, out)
        if b > 0:
            assert np.array_equal(out.download((n,)), expect), (step, budgets)
        prod = ctx.alloc(3 * k * n)
        ev.multiply(ct, 2, fct, 2, k, 1, prod)
        ev.relinearize_inplace(prod, 3, k, 1, [rk])
        ct = ctx.upload(prod.download((3, k, n))[:2].copy())
        expect = O.negacyclic_mod_t(expect, f, t)
    assert budgets[0] > 0 and budgets[-1] < budgets[0]
    ctx.close()


def _dot(cl, ct):
    k, size = ct.shape[1], ct.shape[0]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), size, 0,
                                  O.ptr(cl.sk_powers(size - 1)), O.ptr(dot))
    return dot


@pytest.mark.parametrize("scheme", [1, 2])
def test_cpp_decryptor_on_device(S, tmp_path, scheme):
    """the adapter's budgets and plaintext digests (batch and one by one) equal the C ABI's for the same inputs"""
    logn, n = 10, 1 << 10
    mods = O.coeff_modulus_create(n, [50, 50, 50, 60])
    t = T if scheme == 1 else 0
    ref = O.RefContext(scheme, logn, mods, nsp=1, t=t)
    cl = O.Client(ref, seed=8)
    k, size, count = 3, 3, 4
    rng = np.random.default_rng(scheme)
    if scheme == 1:
        m = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(count)]
        m[1][n // 2:] = 0  # trimmed by get_significant_uint64_count_uint
        m[2][:] = 0
        cts = [cl.encrypt_bfv(x) for x in m]
    else:
        cts = [cl.encrypt_poly_ntt([int(v) for v in rng.integers(-1000, 1000, size=n)]) for _ in range(count)]
    # size 3: a zero third polynomial, except in the last item (which then decrypts to something else, the same on both paths)
    extra = [np.zeros((1, k, n), np.uint64) for _ in range(count - 1)]
    extra.append(np.stack([rng.integers(0, int(p), size=n, dtype=np.uint64) for p in mods[:k]])[None])
    ct = np.stack([np.concatenate([c, x]) for c, x in zip(cts, extra)])
    sk = cl.sk
    words = [scheme, logn, len(mods), 1, t] + [int(p) for p in mods]
    blob = np.concatenate([np.array(words, np.uint64), sk.reshape(-1), np.array([k, size, count], np.uint64),
                           ct.reshape(-1)])
    path = str(tmp_path / "in.bin")
    blob.astype(np.uint64).tofile(path)
    exe = compile_cpp(tmp_path, "host_adapter_decrypt_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", path, timeout=300)
    assert "device decrypt ok" in stdout, stdout
    ctx = S.Context(scheme, logn, mods, 1, t)
    pw = ctx.upload(cl.sk_powers(size - 1))
    dct = ctx.upload(ct)
    lines = stdout.split("\n")
    if scheme == 1:
        budgets = ctx.invariant_noise_budget(dct, size, k, count, pw)
        assert [f"budget {i} {int(b)}" for i, b in enumerate(budgets)] == [x for x in lines if x.startswith("budget")]
        plain = ctx.alloc(count * n)
        ctx.decrypt(dct, size, k, count, pw, False, plain)
        p = plain.download((count, n))
        trimmed = []
        for row in p:
            nz = np.nonzero(row)[0]
            trimmed.append(row[: max(1, int(nz[-1]) + 1 if len(nz) else 1)])
        assert np.array_equal(p[0], m[0]) and len(trimmed[1]) <= n // 2 and len(trimmed[2]) == 1
    else:
        plain = ctx.alloc(count * k * n)
        ctx.decrypt(dct, size, k, count, pw, True, plain)
        trimmed = list(plain.download((count, k * n)))
    assert [f"plain {i} {len(w)} {O.fnv(w)}" for i, w in enumerate(trimmed)] == [x for x in lines if x.startswith("plain")]
    ctx.close()
