"""CPU restatement of the RGSW entries over the oracle. It defines the words of
sealhip_evaluator_external_product, _cmux and _select.

An RGSW encryption of a small polynomial m is two ordinary key-switch keys, K_b with new key m and K_a with new key m s.
    external product   the oracle's ref_switch_key_partial of c_0 with K_b and of c_1 with K_a over all digits, the word-wise
                       sum of the two canonical partials (below 2p < 2^63), and ref_switch_key_finish into a copy of base
    cmux               external_product(ct1 - ct0, base = ct0)
    select             l levels of cmux over adjacent pairs, bit t of the index (least significant first) at level t
The phase check is in Python integers: the result's phase is m * phase(ct) (+ phase(base)) up to a bounded error."""
import ctypes as C

import numpy as np

import oracle_lib as O

# The largest relative error of the restatement's CKKS runs at the moduli of CASES_16 (scale 2^40, log N = 4), measured on
# the CPU by tests/test_rgsw_host.py on clients of their own (fixed seeds, so the figures do not depend on the order of the
# tests): 2^-36.1 of the largest message coefficient for the external product by X^3 (test_restatement_ckks_error) and
# 2^-34.7 for the select tree over 8 leaves (test_tree_picks_each_of_its_8_leaves). The worst is recorded as measured, not
# rounded, and that test pins it. The device tests allow 2^10 times that, the room sections 27 and 28 gave their own.
CKKS_REL_MEASURED = 3.6675231987064643e-11  # 2^-34.7
CKKS_REL_BOUND = CKKS_REL_MEASURED * 2.0 ** 10


def small_to_ntt(ref, coeffs):
    """a polynomial with small signed coefficients, lifted over every key prime (-v -> q_j - v) and transformed: (n_key, N)"""
    s = np.ascontiguousarray(np.asarray(coeffs, dtype=np.int8))
    assert s.shape == (ref.n,)
    out = np.zeros((ref.n_key, ref.n), dtype=np.uint64)
    O.lib().ref_small_poly_to_rns(C.byref(ref.c), s.ctypes.data, ref.n_key, 1, O.ptr(out))
    return out


def times_secret(ref, m_ntt, sk):
    """m (.) s row by row over the key primes"""
    out = np.zeros_like(m_ntt)
    for r in range(ref.n_key):
        O.lib().ref_dyadic_product_coeffmod(O.ptr(np.ascontiguousarray(m_ntt[r])), O.ptr(np.ascontiguousarray(sk[r])), ref.n,
                                            C.byref(ref.c.key_mod[r]), O.ptr(out[r]))
    return out


def rgsw(cl, coeffs):
    """(K_b, K_a) under the client's secret: Client.kswitch_key(m) and Client.kswitch_key(m (.) sk)"""
    m = small_to_ntt(cl.ref, coeffs)
    return cl.kswitch_key(m), cl.kswitch_key(times_secret(cl.ref, m, cl.sk))


def partial(ref, k, target, key):
    """ref_switch_key_partial over all digits of the level: (2, k + nsp, N), canonical"""
    nd = (k + ref.nsp - 1) // ref.nsp
    acc = np.zeros((2, k + ref.nsp, ref.n), dtype=np.uint64)
    assert O.lib().ref_switch_key_partial(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(target, dtype=np.uint64)),
                                          O.ptr(np.ascontiguousarray(key, dtype=np.uint64)), 0, nd, O.ptr(acc)) == 0
    return acc


def external_product(ref, k, ct, g, base=None):
    """base + ct (x) g for one ciphertext (2, k, N); g = (K_b, K_a); base None is zero"""
    total = partial(ref, k, ct[0], g[0]) + partial(ref, k, ct[1], g[1])  # (each word below p < 2^62: no wrap)
    out = np.zeros((2, k, ref.n), dtype=np.uint64) if base is None else np.ascontiguousarray(base, dtype=np.uint64).copy()
    assert O.lib().ref_switch_key_finish(C.byref(ref.c), k, O.ptr(out), O.ptr(np.ascontiguousarray(total))) == 0
    return out


def sub(mods, k, a, b):
    """a - b row by row, canonical: (.., k, N)"""
    out = np.empty_like(a)
    for r in range(k):
        p = np.uint64(mods[r])
        x, y = a[..., r, :], b[..., r, :]
        out[..., r, :] = np.where(x >= y, x - y, x + (p - y))
    return out


def cmux(ref, mods, k, ct0, ct1, g):
    return external_product(ref, k, sub(mods, k, ct1, ct0), g, base=ct0)


def select(ref, mods, k, cts, bits):
    """cts (2^l, 2, k, N); bits[t] = (K_b, K_a) of bit t: the CMux tree, level t pairing W[2i] with W[2i+1]"""
    work = [np.ascontiguousarray(c) for c in cts]
    assert len(work) == 1 << len(bits)
    for g in bits:
        work = [cmux(ref, mods, k, work[2 * i], work[2 * i + 1], g) for i in range(len(work) // 2)]
    return work[0]


# ---------------------------------------------------------------- the phase, in Python integers
def negacyclic(a, b, q):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < n:
                    out[i + j] += x * y
                else:
                    out[i + j - n] -= x * y
    return [v % q for v in out]


def centered(v, q):
    return [x - q if x > q // 2 else x for x in (y % q for y in v)]


def crt_rows(rows, mods):
    """(k, N) coefficient-form rows -> integers modulo q = prod mods"""
    q = 1
    for p in mods:
        q *= p
    out = [0] * rows.shape[1]
    for r, p in enumerate(mods):
        qr = q // p
        w = qr * pow(qr % p, -1, p)
        for i in range(rows.shape[1]):
            out[i] = (out[i] + int(rows[r, i]) * w) % q
    return out, q


def phase(cl, ct, ntt_form):
    """c_0 + c_1 s modulo q of the ciphertext's k primes, centred; (coefficients, q)"""
    k = ct.shape[1]
    polys = []
    for j in range(2):
        rows = np.ascontiguousarray(ct[j]).copy()
        if ntt_form:
            for r in range(k):
                O.lib().ref_ntt_inverse(O.ptr(rows[r]), C.byref(cl.ref.c.key_tables[r]))
        polys.append(crt_rows(rows, cl.mods[:k]))
    q = polys[0][1]
    s = [int(v) % q for v in cl.s]
    c1s = negacyclic(polys[1][0], s, q)
    return centered([a + b for a, b in zip(polys[0][0], c1s)], q), q


def phase_error(cl, out, ct, coeffs, ntt_form, base=None):
    """max |phase(out) - (m * phase(ct) + phase(base))| over the coefficients, centred modulo q"""
    got, q = phase(cl, out, ntt_form)
    src, _ = phase(cl, ct, ntt_form)
    want = negacyclic([int(v) % q for v in coeffs], [v % q for v in src], q)
    if base is not None:
        want = [a + b for a, b in zip(want, phase(cl, base, ntt_form)[0])]
    return max(abs(v) for v in centered([a - b for a, b in zip(got, want)], q))


def monomial(n, power, sign=1):
    m = np.zeros(n, dtype=np.int8)
    m[power] = sign
    return m
