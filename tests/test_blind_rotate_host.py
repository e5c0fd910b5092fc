"""Blind rotation (sealhip_evaluator_multiply_monomial, sealhip_lwe_mod_switch, sealhip_generate_blind_rotation_keys,
sealhip_evaluator_blind_rotate): what can be checked without a GPU. The restatement of
tests/blind_rotate_ref.py against the definitions (the oracle's transform of a one-hot row, exact rounding, decryption under
real keys with the phase in Python integers), the modulus switch's error bound and the margin of the device's end-to-end
case, and the argument checks of every entry on host-only contexts in the header's order."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import blind_rotate_ref as B
import oracle_lib as O
import rgsw_ref as G
from test_rgsw_host import CASES_16, LOGN, N, ckks_rel_error, fresh, ks_error_bound

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_multiply_monomial", "sealhip_lwe_mod_switch", "sealhip_generate_blind_rotation_keys",
       "sealhip_evaluator_blind_rotate")
# the device's end-to-end case (tests/test_tfhe_blind_rotate_gpu.py): ring, secret weight, plain modulus of the lookup
E2E_LOGN, E2E_H, E2E_T = 8, 16, 8


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS and name in header
    for name in ("multiply_monomial", "blind_rotate"):
        assert callable(getattr(S.Evaluator, name))
    for name in ("lwe_mod_switch", "generate_blind_rotation_keys"):
        assert callable(getattr(S.Context, name))
    f = lambda m: (3 * m + 1) % 8
    assert S.lut_test_vector(f, 8, 32).tolist() == B.lut_test_vector(f, 8, 32) == [f(j // 8) for j in range(32)]


# ---------------------------------------------------------------- the monomial product
@pytest.mark.parametrize("logn", [3, 4])
def test_monomial_product_is_the_oracles_transform_of_the_one_hot_row(logn):
    """for all 2N exponents: the integer factors equal the oracle's NTT of +-X^(e mod N), the NTT-form product equals its
    dyadic product with a random row, and the coefficient-form product transforms to the same words"""
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [30, 45, 61])
    ref = O.RefContext(2, logn, mods, nsp=1, t=0, mode=1)
    rng = np.random.default_rng(logn)
    L = O.lib()
    for r, p in enumerate(int(v) for v in mods):
        psi = B.psi_of(ref, r)
        assert pow(psi, n, p) == p - 1
        row = rng.integers(0, p, size=n, dtype=np.uint64)
        row[0], row[1] = p - 1, 0
        row_ntt = row.copy()
        L.ref_ntt_forward(O.ptr(row_ntt), ref.tables(r), B.STRICT)
        for e in range(2 * n):
            hot = np.zeros(n, dtype=np.uint64)
            hot[e % n] = 1 if e < n else p - 1
            L.ref_ntt_forward(O.ptr(hot), ref.tables(r), B.STRICT)
            assert hot.tolist() == B.monomial_factors(n, e, p, psi), (logn, r, e)
            want = np.zeros(n, dtype=np.uint64)
            L.ref_dyadic_product_coeffmod(O.ptr(row_ntt), O.ptr(hot), n, C.byref(ref.c.key_mod[r]), O.ptr(want))
            assert np.array_equal(B.monomial_ntt(row_ntt, e, p, psi), want), (logn, r, e)
            for minus_one in (False, True):
                coeff = B.monomial_coeff(row, e, p, minus_one)
                L.ref_ntt_forward(O.ptr(coeff), ref.tables(r), B.STRICT)
                assert np.array_equal(coeff, B.monomial_ntt(row_ntt, e, p, psi, minus_one)), (logn, r, e, minus_one)
        # an exponent is taken modulo 2N
        assert np.array_equal(B.monomial_coeff(row, 2 * n + 3, p), B.monomial_coeff(row, 3, p))


def test_monomial_product_in_coefficient_form_by_hand():
    p = 97
    row = np.arange(1, 9, dtype=np.uint64)
    assert B.monomial_coeff(row, 0, p).tolist() == list(range(1, 9))
    assert B.monomial_coeff(row, 1, p).tolist() == [p - 8, 1, 2, 3, 4, 5, 6, 7]
    assert B.monomial_coeff(row, 8, p).tolist() == [p - v for v in range(1, 9)]
    assert B.monomial_coeff(row, 9, p).tolist() == [8, p - 1, p - 2, p - 3, p - 4, p - 5, p - 6, p - 7]
    assert B.monomial_coeff(row, 15, p).tolist() == [2, 3, 4, 5, 6, 7, 8, p - 1]  # (X^15 = X^(-1))
    assert B.monomial_coeff(row, 0, p, minus_one=True).tolist() == [0] * 8


# ---------------------------------------------------------------- the modulus switch
def ms_boundaries(q, n):
    """for v = 0 .. 2N - 1 the least x with round(2N x / q) = v + 1"""
    return [-(-((v + 1) * q - q // 2) // (2 * n)) for v in range(2 * n)]


@pytest.mark.parametrize("logn,q", [(3, 1073741441), (8, (1 << 61) - 1), (4, 17 * 32 + 1), (8, 1099511590913)])
def test_ms_on_both_sides_of_every_rounding_boundary(logn, q):
    """ms against rounding to nearest in exact fractions; the value that rounds to 2N wraps to 0"""
    n = 1 << logn

    def nearest(x):
        return int(Fraction(2 * n * x, q) + Fraction(1, 2)) % (2 * n)

    assert B.ms(0, q, n) == 0 and B.ms(q - 1, q, n) == 0
    for v, x in enumerate(ms_boundaries(q, n)):
        if x >= q:
            continue
        assert B.ms(x - 1, q, n) == v == nearest(x - 1), (v, x)
        assert B.ms(x, q, n) == (v + 1) % (2 * n) == nearest(x), (v, x)
    last = ms_boundaries(q, n)[-1]
    assert last < q and B.ms(last, q, n) == 0 and B.ms(last - 1, q, n) == 2 * n - 1


def lwe_sample(rng, secret, phi, q):
    a = [int(v) for v in rng.integers(0, q, size=len(secret), dtype=np.uint64)]
    return a, (phi - sum(x * int(s) for x, s in zip(a, secret))) % q


def centred(v, m):
    v %= m
    return v - m if v > m // 2 else v


@pytest.mark.parametrize("logn,h", [(4, 5), (E2E_LOGN, E2E_H), (8, 256)])
def test_mod_switch_error_is_within_half_of_one_plus_the_weight(logn, h):
    """|phi~ - 2N phi / q| <= (1 + h) / 2 for a secret of weight h: each of the 1 + h rounded words that meet a non-zero
    coefficient is off by at most a half"""
    n = 1 << logn
    q = int(O.coeff_modulus_create(n, [40])[0])
    rng = np.random.default_rng(logn * 100 + h)
    for _ in range(16):
        secret = np.zeros(n, dtype=np.int64)
        secret[rng.permutation(n)[:h]] = rng.choice([-1, 1], size=h)
        phi = int(rng.integers(0, q))
        a, b = lwe_sample(rng, secret, phi, q)
        row = B.exps_rows([a], [b], q, n, True)[0]
        got = B.phi_tilde(row, B.indicators(secret, True), n)
        want = Fraction(2 * n * phi, q)
        err = min(abs(got + w * 2 * n - want) for w in (-1, 0, 1))
        assert err <= Fraction(1 + h, 2), (logn, h, float(err))


def test_margin_of_the_end_to_end_case():
    """the device's lookup at log N = 8, weight 16, t = 8: the modulus switch's error and one for the ciphertext's own noise
    stay inside half a window of N / t coefficients"""
    n = 1 << E2E_LOGN
    assert Fraction(1 + E2E_H, 2) + 1 < Fraction(n, E2E_T)
    # with b_offset = N / t every message m < t / 2 reads f(m) from the constant coefficient, at both ends of its window
    f = lambda m: (5 * m * m + 3) % E2E_T
    tv = B.lut_test_vector(f, E2E_T, n)
    off = n // E2E_T
    for m in range(E2E_T // 2):
        for err in (-(off - 1), 0, off - 1):
            phi = 2 * n * m // E2E_T + off + err
            assert 0 <= phi < n and B.rotated(tv, phi, 1 << 20)[0] == f(m) == tv[phi]
    assert B.rotated(tv, n + 3, 1 << 20)[0] == (1 << 20) - tv[3]  # (the upper half comes back negated)


# ---------------------------------------------------------------- the restatement under real keys
def planted_samples(rng, n, n_lwe, ternary):
    """an LWE secret and a sample directly modulo 2N"""
    secret = rng.integers(-1 if ternary else 0, 2, size=n_lwe)
    secret[0], secret[1] = 1, (-1 if ternary else 0)
    a2 = rng.integers(0, 2 * n, size=n_lwe)
    a2[0], a2[2] = n + 1, 0
    return secret, a2, int(rng.integers(0, 2 * n))


@pytest.mark.parametrize("ternary", [False, True], ids=["binary", "ternary"])
@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_restatement_rotates_the_phase(name, ternary):
    """out decrypts to X^(-phi~) tv (BFV exactly); the phase error is within n_steps key switches' (the bound
    tests/test_rgsw_host.py asserts for one)"""
    mods, ref, cl = fresh(name, 53 + ternary)
    scheme, _, _, t = CASES_16[name]
    rng = np.random.default_rng(11 + ternary)
    secret, a2, b2 = planted_samples(rng, N, N, ternary)
    bits = B.indicators(secret, ternary)
    zero, one = np.zeros(N, dtype=np.int8), G.monomial(N, 0)
    rgsws = [G.rgsw(cl, one if b else zero) for b in bits]
    row = B.exps_from_switched(b2, a2, N, ternary, b_offset=1)
    assert len(row) == 1 + len(bits) == 1 + N * (2 if ternary else 1)
    phi = B.phi_tilde(row, bits, N)
    assert phi == (b2 + 1 + sum(int(a) * int(s) for a, s in zip(a2, secret))) % (2 * N)
    if scheme == 1:
        plain = rng.integers(0, t, size=N, dtype=np.uint64)
        tv = cl.encrypt_bfv(plain)
    else:
        plain = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
        tv = cl.encrypt_poly_ntt(plain)
    for k in (cl.k, 1):
        c = np.ascontiguousarray(tv[:, :k])
        out = B.blind_rotate(ref, k, c, row, rgsws, scheme == 2)
        got, q = G.phase(cl, out, scheme == 2)
        src, _ = G.phase(cl, c, scheme == 2)
        want = B.rotated(src, phi, q)
        err = max(abs(v) for v in G.centered([a - b for a, b in zip(got, want)], q))
        assert err <= len(bits) * ks_error_bound(ref, k), (name, ternary, k, err)
    out = B.blind_rotate(ref, cl.k, tv, row, rgsws, scheme == 2)
    if scheme == 1:
        assert cl.decrypt_bfv(out).tolist() == B.rotated(plain, phi, t), (name, ternary)
    # no steps: the rotation of tv alone, word for word the monomial product
    assert np.array_equal(B.blind_rotate(ref, cl.k, tv, row[:1], [], scheme == 2),
                          B.multiply_monomial(ref, cl.k, tv, row[0], scheme == 2))


def device_shape_session(seed=61):
    scheme, bits, nsp, t = B.CKKS_256
    n = 1 << E2E_LOGN
    mods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(scheme, E2E_LOGN, mods, nsp=nsp, t=t, mode=1)
    return mods, ref, O.Client(ref, seed=seed)


def test_restatement_ckks_error_at_the_device_shape():
    """the figure blind_rotate_ref.CKKS_REL_MEASURED records: log N = 8, a ternary secret, 2N = 512 exact-exponent steps at
    scale 2^40"""
    mods, ref, cl = device_shape_session()
    n = 1 << E2E_LOGN
    rng = np.random.default_rng(8)
    secret, a2, b2 = planted_samples(rng, n, n, True)
    bits = B.indicators(secret, True)
    zero, one = np.zeros(n, dtype=np.int8), G.monomial(n, 0)
    rgsws = [G.rgsw(cl, one if b else zero) for b in bits]
    row = B.exps_from_switched(b2, a2, n, True)
    msg = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=n)]
    out = B.blind_rotate(ref, cl.k, cl.encrypt_poly_ntt(msg), row, rgsws, True)
    want = [centred(v, 1 << 80) for v in B.rotated(msg, B.phi_tilde(row, bits, n), 1 << 80)]
    worst = ckks_rel_error(cl, out, want, msg)
    print("ckks restatement blind rotation, 512 steps: relative error 2^%.1f (%r)" % (np.log2(worst), worst))
    assert worst == B.CKKS_REL_MEASURED, worst  # (the recorded figure IS this measurement)
    assert B.CKKS_REL_BOUND == B.CKKS_REL_MEASURED * 2.0 ** 10


# ---------------------------------------------------------------- the entries on host-only contexts
def test_entries_on_host_only_context():
    """the header's order: E_POINTER; then the E_INVALIDARG checks that need no handle (the level, n_ct, the mode, alignment,
    overlap), which hold for an empty call too; then the host-only context. An RGSW handle cannot exist without a device: the
    pointer handed in is never followed here, and the check that reads it is in tests/test_tfhe_blind_rotate_gpu.py."""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    parity = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, device=-1)
    strict = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    ckks_parity = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, mode=S.MODE_PARITY, device=-1)
    L = S.lib()
    big = np.zeros(1 << 16, dtype=np.uint64)
    base = big.ctypes.data
    base += (-base) % 16
    a, ex, out = base, base + (1 << 15), base + (1 << 17)  # disjoint for count = 2, k = 2
    fake = base + (1 << 18)
    lst = (C.c_void_p * 2)(fake, fake)
    holed = (C.c_void_p * 2)(fake, None)

    def mono(h, k=2, ct=a, n_ct=1, count=2, e=ex, stride=1, o=out):
        return L.sealhip_evaluator_multiply_monomial(h, k, ct, n_ct, count, e, stride, 1, o)

    def rot(h, k=2, ct=a, n_ct=1, count=2, e=ex, steps=2, gs=lst, o=out):
        return L.sealhip_evaluator_blind_rotate(h, k, ct, n_ct, count, e, steps, gs, o)

    ok = (strict.handle, ckks.handle, ckks_parity.handle)
    every = ok + (parity.handle,)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG)
    for h in every:
        for fn in (mono, rot):
            for kw in ({"ct": None}, {"e": None}, {"o": None}):
                with pytest.raises(TypeError):
                    S._check(fn(h, k=9, **kw))
        for kw in ({"gs": None}, {"gs": holed}):
            with pytest.raises(TypeError):
                S._check(rot(h, k=9, **kw))
    for fn in (mono, rot):
        with pytest.raises(TypeError):
            S._check(fn(None))
    # 2. invalid arguments, also for an empty call, in the documented order (each call also breaks every LATER rule)
    for fn in (mono, rot):
        for h in every:
            for count in (2, 0):
                for k in (0, 3, 4):
                    with pytest.raises(ValueError, match="level k out of range"):
                        S._check(fn(h, k=k, count=count, n_ct=5, o=a + 8))
                with pytest.raises(ValueError, match="1 .* or count"):
                    S._check(fn(h, count=count, n_ct=5, o=a + 8))
        for count, n_ct in ((2, 1), (2, 2), (0, 0), (0, 1)):
            with pytest.raises(ValueError, match="STRICT"):  # (the mode before alignment and overlap)
                S._check(fn(parity.handle, count=count, n_ct=n_ct, o=a + 8))
        for h in ok:
            for count, n_ct in ((2, 1), (0, 0)):
                with pytest.raises(ValueError, match="16-byte aligned"):
                    S._check(fn(h, count=count, n_ct=n_ct, o=a + 8))
                with pytest.raises(ValueError, match="16-byte aligned"):
                    S._check(fn(h, count=count, n_ct=n_ct, ct=a + 8, o=a))
                with pytest.raises(ValueError, match="4-byte aligned"):
                    S._check(fn(h, count=count, n_ct=n_ct, e=ex + 2, o=a))
            with pytest.raises(ValueError, match="overlap"):
                S._check(fn(h, o=a))
            with pytest.raises(ValueError, match="overlap"):
                S._check(fn(h, n_ct=2, o=a + 8 * 2 * 2 * n))  # (the second operand)
            with pytest.raises(ValueError, match="overlap"):
                S._check(fn(h, o=ex - 16))  # (out reaches over exps)
            with pytest.raises(ValueError, match="overlap"):
                S._check(fn(h, e=out + 8 * 2 * 2 * 2 * n - 4))  # (the first exponent is out's last half word)
    # 3. a valid call, with work to do or without, is refused as host-only
    for h in ok:
        for fn in (mono, rot):
            for count, n_ct in ((2, 1), (2, 2), (0, 0), (0, 1)):
                with pytest.raises(S.LogicError, match="host-only"):
                    S._check(fn(h, count=count, n_ct=n_ct))
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(rot(h, steps=0, gs=None))


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    from support import compile_cpp, run_exe

    exe = compile_cpp(tmp_path, "host_adapter_blind_rotate_check.cpp", link_sealhip=True)
    assert "host-only blind rotation checks ok" in run_exe(exe, "host", timeout=120)


def test_mod_switch_and_key_entries_on_host_only_context():
    import sealhip as S

    mods = O.coeff_modulus_create(256, [30, 40, 50, 60])
    ctx = S.Context(S.SCHEME_CKKS, 8, mods, 1, 0, device=-1)
    L = S.lib()
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    p += (-p) % 16
    a, b, ex = p, p + 8 * 1024, p + 8 * 2048

    def sw(h=ctx.handle, la=a, lb=b, count=2, ternary=0, o=ex):
        return L.sealhip_lwe_mod_switch(h, la, lb, count, ternary, 3, o)

    for kw in ({"h": None}, {"la": None}, {"lb": None}, {"o": None}):
        with pytest.raises(TypeError):
            S._check(sw(**dict({"o": ex + 2}, **kw)))  # (a misaligned exps_out would be E_INVALIDARG)
    for count in (2, 0):
        with pytest.raises(ValueError, match="aligned"):
            S._check(sw(la=a + 8, count=count))
        with pytest.raises(ValueError, match="aligned"):
            S._check(sw(lb=b + 4, count=count))
        with pytest.raises(ValueError, match="aligned"):
            S._check(sw(o=ex + 2, count=count))
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(sw(count=count))
    with pytest.raises(ValueError, match="overlap"):
        S._check(sw(o=a + 8 * 511))  # (the second sample's last word)
    with pytest.raises(ValueError, match="overlap"):
        S._check(sw(lb=ex + 4 * (2 * 257 - 1) - 4))  # (exps' last word, 8-byte aligned)
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(sw(ternary=1))

    def gen(h=ctx.handle, sk=p, s=p, n_lwe=1, ternary=1, level=3, seeds=p, noise=p, out=True):
        handles = (C.c_void_p * 2)(1, 2)
        return L.sealhip_generate_blind_rotation_keys(h, sk, s, n_lwe, ternary, level, seeds, noise, handles if out else None), list(handles)

    for kw in ({"h": None}, {"sk": None}, {"s": None}, {"seeds": None}, {"noise": None}, {"out": False}):
        with pytest.raises(TypeError):
            S._check(gen(level=9, **kw)[0])
    for level in (0, 4):
        hr, handles = gen(level=level)
        with pytest.raises(ValueError, match="level k out of range"):
            S._check(hr)
        assert handles == [None, None]
    for n_lwe in (1, 0):
        hr, handles = gen(n_lwe=n_lwe)
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(hr)
        assert handles == ([None, None] if n_lwe else [1, 2])
    hr, handles = gen(ternary=0)
    assert handles == [None, 2]  # (a binary secret of one coefficient makes one key)
