"""CPU restatement of the blind-rotation entries over the oracle, on top of tests/rgsw_ref.py. It
defines the words of sealhip_evaluator_multiply_monomial, sealhip_lwe_mod_switch and sealhip_evaluator_blind_rotate.

    monomial product   in Python integers. Coefficient form: (X^e c)[x] = sgn c[x - e'] for x >= e', -sgn c[N + x - e'] below
                       (e' = e mod N, sgn = -1 for e >= N). NTT form: position c of row r holds the value at
                       psi_r^(2 brev(c) + 1), so the factor is psi_r^(e (2 brev(c) + 1) mod 2N); psi_r is read off the oracle's
                       own transform (position 0 of NTT(X)), and tests/test_blind_rotate_host.py holds the product to the
                       oracle's transform of the one-hot row followed by its dyadic product
    ms(x)              floor((2N x + floor(q / 2)) / q) mod 2N
    exps rows          blind_rotate's layout from mod-switched samples, binary and ternary
    blind_rotate       acc = X^(e_0) tv; acc = external_product((X^(e_t) - 1) acc, rgsw[t - 1], base = acc)"""
import ctypes as C

import numpy as np

import oracle_lib as O
import rgsw_ref as G

# The largest relative error of the restatement's CKKS run at the shape of the device's semantic check (log N = 8, the
# moduli of CKKS_256 below, scale 2^40, a ternary secret, n_steps = 2N = 512 exact-exponent steps), measured on the CPU by
# tests/test_blind_rotate_host.py::test_restatement_ckks_error_at_the_device_shape on a client of its own (fixed seeds).
# Recorded as measured; that test pins it. The device test allows 2^10 times that, the room sections 27 to 29 gave.
CKKS_256 = (2, [40] * 3 + [41], 1, 0)
CKKS_REL_MEASURED = 2.2180926464561405e-09  # 2^-28.7
CKKS_REL_BOUND = CKKS_REL_MEASURED * 2.0 ** 10


# The oracle's forward transform is asked for Harvey's correction in every layer: without it (the fork's PARITY quirk) the
# lazy words of a 61-bit prime wrap 64 bits from log N = 8 on, and the transform of a one-hot row is not the evaluation map.
STRICT = 1


def psi_of(ref, r):
    """psi_r as the oracle's transform has it: NTT(X)[0] is the value of X at psi^(2 brev(0) + 1) = psi"""
    row = np.zeros(ref.n, dtype=np.uint64)
    row[1] = 1
    O.lib().ref_ntt_forward(O.ptr(row), C.byref(ref.c.key_tables[r]), STRICT)
    return int(row[0])


def monomial_coeff(row, e, p, minus_one=False):
    """X^e row (- row) in coefficient form, one row of canonical residues modulo p"""
    n = len(row)
    e %= 2 * n
    s, sgn = e % n, -1 if e >= n else 1
    out = []
    for x in range(n):
        v = sgn * int(row[x - s]) if x >= s else -sgn * int(row[n + x - s])
        out.append((v - (int(row[x]) if minus_one else 0)) % p)
    return np.array(out, dtype=np.uint64)


def monomial_factors(n, e, p, psi):
    """NTT(X^e) modulo p in the transform's order: psi^(e (2 brev(c) + 1) mod 2N)"""
    logn = n.bit_length() - 1
    key = (n, p, psi)
    if key not in _POWERS:
        pw = [1]
        for _ in range(2 * n - 1):
            pw.append(pw[-1] * psi % p)
        _POWERS[key] = (pw, [2 * O.bitrev(c, logn) + 1 for c in range(n)])
    pw, odd = _POWERS[key]
    return [pw[(e * o) % (2 * n)] for o in odd]


_POWERS = {}


def monomial_ntt(row, e, p, psi, minus_one=False):
    """NTT(X^e) (.) row (- row) for one NTT-form row"""
    n = len(row)
    f = monomial_factors(n, e % (2 * n), p, psi)
    return np.array([(int(v) * (w - (1 if minus_one else 0))) % p for v, w in zip(row, f)], dtype=np.uint64)


def multiply_monomial(ref, k, ct, e, ntt_form, minus_one=False):
    """one size-2 ciphertext (2, k, N) at level k"""
    out = np.empty_like(ct)
    for r in range(k):
        p = ref.key_moduli[r]
        psi = psi_of(ref, r) if ntt_form else None
        for j in range(2):
            out[j, r] = monomial_ntt(ct[j, r], e, p, psi, minus_one) if ntt_form else monomial_coeff(ct[j, r], e, p, minus_one)
    return out


def ms(x, q, n):
    """the modulus switch of one word from q to 2N, rounded to nearest; a value that rounds to 2N wraps to 0"""
    return ((2 * n * int(x) + q // 2) // q) % (2 * n)


def exps_from_switched(b2, a2, n, ternary, b_offset=0):
    """one row of blind_rotate's exps from a sample already modulo 2N: b2 and a2[n_lwe]"""
    row = [(-(int(b2) + b_offset)) % (2 * n)]
    for a in a2:
        row.append((-int(a)) % (2 * n))
        if ternary:
            row.append(int(a) % (2 * n))
    return row


def exps_rows(lwe_a, lwe_b, q, n, ternary, b_offset=0):
    """sealhip_lwe_mod_switch: lwe_a (n_samples, N), lwe_b (n_samples,) modulo q -> (n_samples, 1 + n_steps) uint32"""
    return np.array([exps_from_switched(ms(b, q, n), [ms(x, q, n) for x in a], n, ternary, b_offset)
                     for a, b in zip(lwe_a, lwe_b)], dtype=np.uint32)


def indicators(secret, ternary):
    """the bits the blind-rotation keys encrypt, in step order: [s_j = 1] (then [s_j = -1] for a ternary secret)"""
    bits = []
    for s in secret:
        bits.append(1 if s == 1 else 0)
        if ternary:
            bits.append(1 if s == -1 else 0)
    return bits


def phi_tilde(row, bits, n):
    """the exponent the rotation applies, negated: out = X^(-phi~) tv"""
    return (-(int(row[0]) + sum(int(e) for e, b in zip(row[1:], bits) if b))) % (2 * n)


def blind_rotate(ref, k, tv, row, rgsws, ntt_form):
    """one item: tv (2, k, N), row = exps[i] (1 + n_steps), rgsws[t] = (K_b, K_a)"""
    acc = multiply_monomial(ref, k, tv, int(row[0]), ntt_form)
    for e, g in zip(row[1:], rgsws):
        acc = G.external_product(ref, k, multiply_monomial(ref, k, acc, int(e), ntt_form, minus_one=True), g, base=acc)
    return acc


def lut_test_vector(f, t, n):
    """tv[j] = f(floor(j t / 2N)), j < N (the library's sealhip.lut_test_vector, restated)"""
    return [f((j * t) // (2 * n)) for j in range(n)]


def rotated(tv, phi, q):
    """X^(-phi) tv in integers modulo q (coefficient form): what the rotation's output decrypts to"""
    n = len(tv)
    e = (-phi) % (2 * n)
    s, sgn = e % n, -1 if e >= n else 1
    return [(sgn * int(tv[x - s]) if x >= s else -sgn * int(tv[n + x - s])) % q for x in range(n)]
