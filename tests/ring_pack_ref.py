"""Ring packing restated on the CPU (include/sealhip.h, "Ring packing"): the LWE sample of one
coefficient, its embedding, the monomial product and the merge / trace steps in numpy and Python integers; the automorphism
with its key switch and the ciphertext sums are the oracle's (ref_apply_galois_inplace, ref_evaluator_add / _sub), the
transforms of the CKKS form the oracle's too. The device's fused step reorders exact modular sums only, so its words equal
this composition bit for bit. `pack_keyless` is the same tree on plaintext polynomials, with no keys at all."""
import ctypes as C

import numpy as np

import oracle_lib as O


def galois_elts(logn, n, trace):
    """the elements 2^t + 1 the pack of n = 2^l samples needs, ascending"""
    l = n.bit_length() - 1
    return [(1 << t) + 1 for t in range(1, (logn if trace else l) + 1)]


def neg(v, p):
    """-v on canonical residues: p - v, and 0 stays 0"""
    v = np.asarray(v, dtype=np.uint64)
    return np.where(v == 0, np.uint64(0), np.uint64(p) - v).astype(np.uint64)


def scale(v, w, p):
    """w * v mod p, exactly (Python integers)"""
    return np.array([int(x) * w % p for x in np.asarray(v).ravel()], dtype=np.uint64).reshape(np.shape(v))


def weights(mods, k, n, big_n, trace, normalize):
    """w_r: 1, or the inverse of the factor the steps put on the phase (n; N with the trace)"""
    return [pow((big_n if trace else n) % mods[r], -1, mods[r]) if normalize else 1 for r in range(k)]


def extract(ct, mods, j):
    """(a[k][N], b[k]) of coefficient j of the coefficient-form ciphertext ct[2][k][N]"""
    k, n = ct.shape[1], ct.shape[2]
    i = np.arange(n)
    a = np.empty((k, n), dtype=np.uint64)
    for r in range(k):
        row = ct[1, r][(j - i) % n]
        a[r] = np.where(i > j, neg(row, mods[r]), row)
    return a, ct[0, :, j].copy()


def embed(a, b, mods, w):
    """coefficient-form ciphertext [2][k][N] of the sample (a[k][N], b[k]) scaled by w[r]"""
    k, n = a.shape
    ct = np.zeros((2, k, n), dtype=np.uint64)
    for r in range(k):
        p = mods[r]
        ct[0, r, 0] = int(b[r]) * w[r] % p
        c1 = np.empty(n, dtype=np.uint64)
        c1[0] = a[r, 0]
        c1[1:] = neg(a[r, :0:-1], p)  # c_1[N - i] = -a[i]
        ct[1, r] = scale(c1, w[r], p)
    return ct


def mul_monomial(rows, s, mods):
    """X^s times every row of rows[..][k][N], coefficient form, 0 <= s < N"""
    n = rows.shape[-1]
    out = np.empty_like(rows)
    for r in range(rows.shape[-2]):
        out[..., r, s:] = rows[..., r, : n - s]
        out[..., r, :s] = neg(rows[..., r, n - s:], mods[r]) if s else rows[..., r, :0]
    return out


def transform(ref, rows, inverse=False):
    """the oracle's canonical transforms over rows[..][k][N] (row r under prime r), the forward one in the context's mode
    (the fork's lazy butterflies, PARITY, are not a transform for primes near 2^60 on long rings)"""
    out = np.ascontiguousarray(rows, dtype=np.uint64).copy()
    flat = out.reshape(-1, out.shape[-2], out.shape[-1])
    L = O.lib()
    strict = int(ref.c.mode)
    for x in flat:
        for r in range(x.shape[0]):
            if inverse:
                L.ref_ntt_inverse(O.ptr(x[r]), ref.tables(r))
            else:
                L.ref_ntt_forward(O.ptr(x[r]), ref.tables(r), strict)
    return out


def extract_samples(ref, mods, ct, indices):
    """lwe_a[count][n_idx][k][N], lwe_b[count][n_idx][k] of ct[count][2][k][N] in the scheme's form"""
    count, _, k, n = ct.shape
    coeff = transform(ref, ct, inverse=True) if ref.scheme == 2 else ct
    la = np.empty((count, len(indices), k, n), dtype=np.uint64)
    lb = np.empty((count, len(indices), k), dtype=np.uint64)
    for c in range(count):
        for s, j in enumerate(indices):
            la[c, s], lb[c, s] = extract(coeff[c], mods, j)
    return la, lb


def _galois_step(ref, k, sums, diff, g, key):
    """sums + apply_galois(diff, g): both [2][k][N] in the scheme's form"""
    L = O.lib()
    d = np.ascontiguousarray(diff).copy()
    assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(d), g, O.ptr(key)) == 0
    out = np.zeros_like(d)
    L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(sums)), 2, O.ptr(d), 2, O.ptr(out))
    return out


def pack(ref, mods, k, lwe_a, lwe_b, keys, trace=False, normalize=False):
    """ct[2][k][N] in the scheme's form: the pack of the samples lwe_a[n][k][N], lwe_b[n][k] of ONE item; keys: element ->
    host key"""
    L = O.lib()
    n, big_n, logn = lwe_a.shape[0], ref.n, ref.logn
    ckks = ref.scheme == 2
    w = weights(mods, k, n, big_n, trace, normalize)
    W = [embed(lwe_a[j], lwe_b[j], mods, w) for j in range(n)]
    if ckks:
        W = [transform(ref, x) for x in W]
    l = n.bit_length() - 1
    for t in range(1, l + 1):
        half, s, g = 1 << (l - t), big_n >> t, (1 << t) + 1
        if ckks:
            one_hot = np.zeros((k, big_n), dtype=np.uint64)
            one_hot[:, s] = 1
            mono = transform(ref, one_hot)
        nxt = []
        for j in range(half):
            E, B = W[j], W[j + half]
            if ckks:
                odd = np.empty_like(B)
                for r in range(k):
                    prod = [int(x) * int(m) % mods[r] for x, m in zip(B[:, r].ravel(), np.tile(mono[r], 2))]
                    odd[:, r] = np.array(prod, dtype=np.uint64).reshape(2, big_n)
            else:
                odd = mul_monomial(B, s, mods)
            sums, diff = np.zeros_like(E), np.zeros_like(E)
            L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(E), 2, O.ptr(odd), 2, O.ptr(sums))
            L.ref_evaluator_sub(C.byref(ref.c), k, O.ptr(E), 2, O.ptr(odd), 2, O.ptr(diff))
            nxt.append(_galois_step(ref, k, sums, diff, g, keys[g]))
        W = nxt
    out = np.ascontiguousarray(W[0])
    if trace:
        for t in range(l + 1, logn + 1):
            g = (1 << t) + 1
            out = _galois_step(ref, k, out, out, g, keys[g])
    return out


def pack_batch(ref, mods, k, lwe_a, lwe_b, keys, trace=False, normalize=False):
    """[count][2][k][N] for lwe_a[count][n][k][N], lwe_b[count][n][k]"""
    return np.stack([pack(ref, mods, k, lwe_a[c], lwe_b[c], keys, trace, normalize) for c in range(lwe_a.shape[0])])


# ---------------------------------------------------------------- the same tree without keys, on plaintext polynomials
def galois_plain(poly, g, q):
    """x -> x^g on a polynomial with coefficients mod q (Python integers)"""
    n = len(poly)
    out = [0] * n
    for i, v in enumerate(poly):
        j = (i * g) % (2 * n)
        out[j % n] = (-v) % q if j >= n else v % q
    return out


def pack_keyless(values, logn, q, trace=False):
    """the pack of the constants values[j] (as the phases of n samples): the polynomial whose coefficient (N / n) j is
    n * values[j] (N * values[j] and zero elsewhere with the trace)"""
    big_n, n = 1 << logn, len(values)
    W = [[v % q] + [0] * (big_n - 1) for v in values]
    return pack_keyless_polys(W, logn, q, trace)


def pack_keyless_polys(W, logn, q, trace=False):
    """... of n full polynomials: coefficient (N / n) j gets n (or N) times the constant coefficient of W[j]"""
    big_n, n = 1 << logn, len(W)
    l = n.bit_length() - 1
    for t in range(1, l + 1):
        half, s, g = 1 << (l - t), big_n >> t, (1 << t) + 1
        nxt = []
        for j in range(half):
            E, B = W[j], W[j + half]
            odd = [(-B[c - s + big_n]) % q if c < s else B[c - s] for c in range(big_n)]
            sums = [(a + b) % q for a, b in zip(E, odd)]
            rot = galois_plain([(a - b) % q for a, b in zip(E, odd)], g, q)
            nxt.append([(a + b) % q for a, b in zip(sums, rot)])
        W = nxt
    out = W[0]
    if trace:
        for t in range(l + 1, logn + 1):
            out = [(a + b) % q for a, b in zip(out, galois_plain(out, (1 << t) + 1, q))]
    return out


# ---------------------------------------------------------------- the semantic check of the CKKS form
# The restatement's own error under real keys at log N = 4, scale 2^40, 50-bit primes, relative to the largest message
# coefficient, is at most 2^-34.1 on the seeds of tests/test_ring_pack_host.py (which prints it):
# 2^-24 leaves 2^10 of room, on the CPU and on the device.
CKKS_REL_BOUND = 2.0 ** -24


def ckks_phase(cl, ct):
    """centred integer coefficients of c_0 + c_1 s for the NTT-form ct[2][k][N] under the O.Client cl"""
    k = ct.shape[1]
    dot = np.zeros((k, cl.n), dtype=np.uint64)
    O.lib().ref_dot_product_ct_sk(C.byref(cl.ref.c), k, O.ptr(np.ascontiguousarray(ct)), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
    return cl.centered_from_ntt_rows(dot)[0]
