"""CPU restatement of polynomial evaluation on BFV ciphertexts (sealhip_evaluator_evaluate_polynomial),
composed only from the oracle's functions and dot_ct_ref: Paterson-Stockmeyer with the power basis built by ref_bfv_multiply +
ref_relinearize, the inner sums by ref_multiply_plain on one-coefficient plaintexts + ref_evaluator_add +
ref_multiply_add_plain_with_scaling_variant, and the outer sum by dot_ct_ref.bfv_dot_product (ONE floor, ONE relinearization).
Also the oracle composition that defines sealhip_evaluator_linear_combination's words, and the shape (d, m, g) of a call."""
import ctypes as C

import numpy as np

import dot_ct_ref as D
import oracle_lib as O


def shape(coeffs, n_baby=0):
    """(trimmed coefficients, d, m, g): trailing zeros trimmed, m = n_baby or ceil(sqrt(d + 1)), g = ceil((d + 1) / m)"""
    c = [int(v) for v in coeffs]
    while len(c) > 1 and c[-1] == 0:
        c.pop()
    d = len(c) - 1
    m = int(n_baby)
    if m == 0:
        m = 1
        while m * m < d + 1:
            m += 1
    g = (d + m) // m
    return c, d, m, g


def linear_combination(ref, k, terms, weights, constant=None):
    """terms[i]: [size][k][N]; weights [n_sums][n_terms][k] canonical residues; constant [n_sums][k] or None. Returns
    [n_sums][size][k][N]: ref_multiply_poly_scalar_coeffmod per term and row, ref_add_poly_coeffmod left to right, the constant
    added last to polynomial 0 (BFV: coefficient 0; CKKS: every coefficient)."""
    L = O.lib()
    n, size = ref.n, terms[0].shape[0]
    weights = np.asarray(weights, dtype=np.uint64)
    n_sums = weights.shape[0]
    out = np.zeros((n_sums, size, k, n), dtype=np.uint64)
    prod = np.zeros(n, dtype=np.uint64)
    for s in range(n_sums):
        for i, x in enumerate(terms):
            x = np.ascontiguousarray(x, dtype=np.uint64)
            for j in range(size):
                for r in range(k):
                    m = C.byref(ref.c.key_mod[r])
                    L.ref_multiply_poly_scalar_coeffmod(O.ptr(x[j, r]), n, int(weights[s, i, r]), m, O.ptr(prod))
                    L.ref_add_poly_coeffmod(O.ptr(out[s, j, r]), O.ptr(prod), n, m, O.ptr(out[s, j, r]))
        if constant is not None:
            for r in range(k):
                kv = np.zeros(n, dtype=np.uint64)
                if ref.scheme == 1:
                    kv[0] = int(constant[s][r])
                else:
                    kv[:] = int(constant[s][r])
                L.ref_add_poly_coeffmod(O.ptr(out[s, 0, r]), O.ptr(kv), n, C.byref(ref.c.key_mod[r]), O.ptr(out[s, 0, r]))
    return out


def bfv_weight(c, t, q):
    """w(c)[r] = (c - t [c >= (t + 1) / 2]) mod q_r: what multiply_plain multiplies by for a one-coefficient plaintext"""
    c, t = int(c), int(t)
    return [(c - (t if c >= (t + 1) // 2 else 0)) % int(p) for p in q]


def bfv_constant(ref, k, c):
    """K(c)[r]: the word ref_multiply_add_plain_with_scaling_variant adds at coefficient 0 for the plaintext c"""
    plain = np.zeros(ref.n, dtype=np.uint64)
    plain[0] = int(c)
    c0 = np.zeros((k, ref.n), dtype=np.uint64)
    O.lib().ref_multiply_add_plain_with_scaling_variant(C.byref(ref.c), k, O.ptr(plain), 0, O.ptr(c0))
    assert not c0[:, 1:].any()
    return [int(v) for v in c0[:, 0]]


def _product(ref, k, a, b, relin_key):
    L = O.lib()
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    wide = np.zeros((3, k, ref.n), dtype=np.uint64)
    assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a), 2, O.ptr(b), 2, O.ptr(wide)) == 0
    key = np.ascontiguousarray(relin_key, dtype=np.uint64)
    keys = (C.c_void_p * 1)(key.ctypes.data)
    assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(wide), 3, keys) == 0
    return np.ascontiguousarray(wide[:2])


def _add(ref, k, a, b):
    out = np.zeros_like(a)
    O.lib().ref_evaluator_add(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(a)), 2, O.ptr(np.ascontiguousarray(b)), 2, O.ptr(out))
    return out


def inner_sum(ref, k, baby, coeffs):
    """coeffs[0] + sum_{i >= 1} coeffs[i] * baby[i] with one-coefficient plaintexts; zero coefficients are skipped"""
    L = O.lib()
    n = ref.n
    acc = np.zeros((2, k, n), dtype=np.uint64)
    for i in range(1, len(coeffs)):
        if coeffs[i] == 0:
            continue
        plain = np.zeros(n, dtype=np.uint64)
        plain[0] = coeffs[i]
        term = np.ascontiguousarray(baby[i], dtype=np.uint64).copy()
        assert L.ref_multiply_plain(C.byref(ref.c), k, O.ptr(term), 2, O.ptr(plain)) == 0
        acc = _add(ref, k, acc, term)
    if coeffs[0]:
        plain = np.zeros(n, dtype=np.uint64)
        plain[0] = coeffs[0]
        L.ref_multiply_add_plain_with_scaling_variant(C.byref(ref.c), k, O.ptr(plain), 0, O.ptr(acc[0]))
    return acc


def power_basis(ref, k, ct, d, m, g, needed_giants, relin_key):
    """baby[e] for 1 <= e <= min(m, d) and giant[j] for the needed 1 <= j < g (memoised, halves first)"""
    baby = {1: np.ascontiguousarray(ct, dtype=np.uint64)}
    for e in range(2, min(m, d) + 1):
        baby[e] = _product(ref, k, baby[(e + 1) // 2], baby[e // 2], relin_key)
    giant = {}
    if g > 1:
        giant[1] = baby[m]

    def build(j):
        if j not in giant:
            build((j + 1) // 2)
            build(j // 2)
            giant[j] = _product(ref, k, giant[(j + 1) // 2], giant[j // 2], relin_key)
        return giant[j]

    for j in sorted(needed_giants):
        build(j)
    return baby, giant


def evaluate_polynomial(ref, k, ct, coeffs, relin_key=None, n_baby=0):
    """ct: [2][k][N] coefficient form; coeffs: integers below t, lowest degree first. Returns [2][k][N]."""
    c, d, m, g = shape(coeffs, n_baby)
    assert d >= 1 and (n_baby == 0 or 2 <= n_baby <= d + 1)
    padded = c + [0] * (g * m - len(c))
    chunks = [padded[j * m:(j + 1) * m] for j in range(g)]
    outer = [j for j in range(1, g) if any(chunks[j])]
    baby, giant = power_basis(ref, k, ct, d, m, g, outer, relin_key)
    inner = [inner_sum(ref, k, baby, ch) for ch in chunks]  # (coefficients beyond d are zero and are skipped)
    if not outer:
        return inner[0]
    dot = D.bfv_dot_product(ref, k, [giant[j] for j in outer], [inner[j] for j in outer], relin_key)
    return _add(ref, k, inner[0], dot)


def composition(ref, k, ct, coeffs, relin_key, n_baby=0):
    """the same power basis and inner sums, the outer sum by multiply + relinearize + add per giant step"""
    c, d, m, g = shape(coeffs, n_baby)
    padded = c + [0] * (g * m - len(c))
    chunks = [padded[j * m:(j + 1) * m] for j in range(g)]
    outer = [j for j in range(1, g) if any(chunks[j])]
    baby, giant = power_basis(ref, k, ct, d, m, g, outer, relin_key)
    acc = inner_sum(ref, k, baby, chunks[0])
    for j in outer:
        acc = _add(ref, k, acc, _product(ref, k, giant[j], inner_sum(ref, k, baby, chunks[j]), relin_key))
    return acc
