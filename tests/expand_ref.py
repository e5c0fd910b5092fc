"""Oblivious expansion and the sums against plaintext rows restated on the CPU (include/sealhip.h,
"Oblivious expansion"). The tree is written over the oracle's ref_apply_galois_inplace and ref_evaluator_add and the
monomial product and transforms of tests/ring_pack_ref.py; the normalisation is in Python integers. The device's fused step
reorders exact modular sums only, so its words equal this composition bit for bit. `expand_keyless` is the same tree on
a plaintext polynomial, with no keys at all. `dot_plain` is multiply_plain_ntt per term and add left to right, and
`dot_plain_int` the same sums in Python integers."""
import ctypes as C

import numpy as np

import oracle_lib as O
import ring_pack_ref as R


def galois_elts(logn, n):
    """the elements N / 2^(t-1) + 1, t = 1 .. l, that the expansion into n = 2^l needs, ascending"""
    l = n.bit_length() - 1
    return sorted((1 << (logn - t + 1)) + 1 for t in range(1, l + 1))


def weights(mods, k, n, normalize):
    """w_r: 1, or the inverse of the factor n the steps put on the phase"""
    return [pow(n % mods[r], -1, mods[r]) if normalize else 1 for r in range(k)]


def mul_inverse_monomial(ref, mods, ct, s):
    """X^(-s) times ct[2][k][N] in the scheme's form, 0 < s < N: -X^(N - s) in coefficient form, the dyadic product with the
    transform of that monomial in NTT form"""
    k, big_n = ct.shape[1], ct.shape[2]
    if ref.scheme != 2:
        up = R.mul_monomial(ct, big_n - s, mods)
        return np.stack([np.stack([R.neg(up[j, r], mods[r]) for r in range(k)]) for j in range(2)])
    one_hot = np.zeros((k, big_n), dtype=np.uint64)
    for r in range(k):
        one_hot[r, big_n - s] = mods[r] - 1
    mono = R.transform(ref, one_hot)
    out = np.empty_like(ct)
    for r in range(k):
        prod = [int(x) * int(m) % mods[r] for x, m in zip(ct[:, r].ravel(), np.tile(mono[r], 2))]
        out[:, r] = np.array(prod, dtype=np.uint64).reshape(2, big_n)
    return out


def _plus_galois(ref, k, ct, g, key):
    """ct + apply_galois(ct, g): [2][k][N] in the scheme's form"""
    L = O.lib()
    d = np.ascontiguousarray(ct).copy()
    assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(d), g, O.ptr(key)) == 0
    out = np.zeros_like(d)
    L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(ct)), 2, O.ptr(d), 2, O.ptr(out))
    return out


def expand(ref, mods, k, ct, keys, n, normalize=False):
    """[n][2][k][N] in the scheme's form: the expansion of ONE ciphertext ct[2][k][N]; keys: element -> host key"""
    big_n = ref.n
    w = weights(mods, k, n, normalize)
    first = np.ascontiguousarray(ct, dtype=np.uint64).copy()
    for r in range(k):
        first[:, r] = R.scale(first[:, r], w[r], mods[r])
    W = [first]
    l = n.bit_length() - 1
    for t in range(1, l + 1):
        cur = 1 << (t - 1)
        g = big_n // cur + 1
        nxt = [None] * (2 * cur)
        for j in range(cur):
            E = W[j]
            odd = mul_inverse_monomial(ref, mods, E, cur)
            nxt[j] = _plus_galois(ref, k, E, g, keys[g])
            nxt[j + cur] = _plus_galois(ref, k, odd, g, keys[g])
        W = nxt
    return np.stack(W)


def expand_batch(ref, mods, k, ct, keys, n, normalize=False):
    """[count][n][2][k][N] for ct[count][2][k][N]"""
    return np.stack([expand(ref, mods, k, ct[c], keys, n, normalize) for c in range(ct.shape[0])])


# ---------------------------------------------------------------- the same tree without keys, on a plaintext polynomial
def expand_keyless(poly, logn, n, q):
    """the n polynomials the tree makes of `poly` (coefficients mod q): output i is n sum_u poly[i + n u] X^(n u)"""
    big_n = 1 << logn
    W = [[v % q for v in poly]]
    l = n.bit_length() - 1
    for t in range(1, l + 1):
        cur = 1 << (t - 1)
        g = big_n // cur + 1
        nxt = [None] * (2 * cur)
        for j in range(cur):
            E = W[j]
            odd = [E[x + cur] if x + cur < big_n else (-E[x + cur - big_n]) % q for x in range(big_n)]
            nxt[j] = [(a + b) % q for a, b in zip(E, R.galois_plain(E, g, q))]
            nxt[j + cur] = [(a + b) % q for a, b in zip(odd, R.galois_plain(odd, g, q))]
        W = nxt
    return W


def closed_form(poly, logn, n, q, i):
    """n sum_u poly[i + n u] X^(n u) mod q"""
    big_n = 1 << logn
    out = [0] * big_n
    for u in range(big_n // n):
        out[n * u] = n * poly[i + n * u] % q
    return out


# ---------------------------------------------------------------- sums against plaintext rows
def dot_plain(ref, k, cts, plain):
    """out[n_sums][count][size][k][N] for cts[count][n_terms][size][k][N] and plain[n_sums][n_terms][k][N], all in NTT form:
    multiply_plain_ntt per term and add left to right"""
    L = O.lib()
    count, n_terms, size = cts.shape[:3]
    n_sums = plain.shape[0]
    out = np.zeros((n_sums, count) + cts.shape[2:], dtype=np.uint64)
    for s in range(n_sums):
        for c in range(count):
            acc = None
            for i in range(n_terms):
                term = np.ascontiguousarray(cts[c, i]).copy()
                L.ref_multiply_plain_ntt(C.byref(ref.c), k, O.ptr(term), size, O.ptr(np.ascontiguousarray(plain[s, i])))
                if acc is None:
                    acc = term
                else:
                    nxt = np.zeros_like(acc)
                    L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(acc), size, O.ptr(term), size, O.ptr(nxt))
                    acc = nxt
            out[s, c] = acc
    return out


def dot_plain_int(mods, cts, plain):
    """the same sums as exact integers reduced once (object arrays of Python integers)"""
    count, n_terms, size, k, _ = cts.shape
    n_sums = plain.shape[0]
    x = cts.astype(object)
    p = plain.astype(object)
    out = np.zeros((n_sums, count) + cts.shape[2:], dtype=np.uint64)
    for s in range(n_sums):
        acc = (x * p[s][None, :, None]).sum(axis=1)  # [count][size][k][N]
        for r in range(k):
            out[s, :, :, r] = (acc[:, :, r] % mods[r]).astype(np.uint64)
    return out


# ---------------------------------------------------------------- the semantic check of the CKKS form
# The restatement's own error under real keys at log N = 4, scale 2^40, the 40-bit moduli of CASES_16, relative to the
# largest message coefficient, is at most 2^-33.3 on the seeds of tests/test_expand_host.py (n = 16; the test prints every
# n and holds them to the number below). The bound of the CPU and the device tests is 2^10 times
# that, the room section 27 gave its CKKS_REL_BOUND: 2^-23.2.
CKKS_REL_MEASURED = 2.0 ** -33.2
CKKS_REL_BOUND = CKKS_REL_MEASURED * 2.0 ** 10
