"""CPU restatement of polynomial evaluation on CKKS ciphertexts with planned levels and scales
(sealhip_evaluator_polynomial_plan_ckks / _evaluate_polynomial_ckks).

plan() is gemini-seal_amd/csrc/poly_plan.hpp in Python: the same IEEE double operations in the same order (Python floats are
doubles, round(float) rounds half to even, int(float) is exact), so plan, scales and tables are equal bit for bit.
evaluate() runs that plan with ks_rescale_ref (dot_product_rescale, relinearize_rescale, rescale), dot_ct_ref.ckks_dot_product,
poly_eval_ref.linear_combination and row slicing only: a term at a higher level is its first rows, a size-2 term in a size-3 sum
is padded with a zero polynomial. composition() is the same plan with every merged step replaced by its unmerged pair
(dot_product with keys, then rescale): what the call's error is measured against."""
import numpy as np

import dot_ct_ref as DC
import ks_rescale_ref as KR
import poly_eval_ref as P


def delta(e):
    """ceil(log2 e)"""
    b = 0
    while (1 << b) < e:
        b += 1
    return b


def rint(x):
    """round half to even, exactly, as a Python integer (a double at or above 2^53 is an integer already)"""
    return int(round(x)) if abs(x) < 2.0 ** 53 else int(x)


def residues(x, q):
    """rint(x) reduced per prime: negatives become q_r - (|I| mod q_r), or 0 when q_r divides I"""
    v = rint(x)
    return [v % int(p) for p in q]


def divide_by_tm(a, m):
    """a / T_m in the Chebyshev basis; returns the quotient and leaves the remainder in a[:m]"""
    n = len(a) - 1
    quot = [0.0] * (n - m + 1)
    for i in range(n, m, -1):
        twice = a[i] + a[i]
        quot[i - m] = quot[i - m] + twice
        back = abs(i - 2 * m)
        a[back] = a[back] - a[i]
        a[i] = 0.0
    quot[0] = quot[0] + a[m]
    a[m] = 0.0
    return quot


def chunks_of(c, d, m, g, basis):
    if basis == 0:
        padded = list(c) + [0.0] * (g * m - len(c))
        return [padded[j * m:(j + 1) * m] for j in range(g)]
    out, cur = [], list(c)
    while len(cur) > m:
        quot = divide_by_tm(cur, m)
        out.append(cur[:m])
        cur = quot
    out.append(cur + [0.0] * (m - len(cur)))
    assert len(out) == g
    return out


def plan(q, k, scale, coeffs, basis=0, n_baby=0, scale_out=0.0):
    """q: the data primes of the first level. Returns a dict with the shape, the levels and scales of every element, the
    chunks, and the tables W [g][m - 1][L_in], K [g][L_in] (uint64; rows of sums that are not formed stay zero)."""
    q = [int(p) for p in q]
    c = [float(v) for v in coeffs]
    while len(c) > 1 and c[-1] == 0:
        c.pop()
    d = len(c) - 1
    assert d >= 1 and basis in (0, 1) and (n_baby == 0 or 2 <= n_baby <= d + 1)
    m = int(n_baby)
    if m == 0:
        m = 1
        while m * m < d + 1:
            m += 1
    g = (d + m) // m
    mi, nb = m - 1, min(m, d)
    scale, scale_out = float(scale), float(scale_out) if scale_out else float(scale)
    chunks = chunks_of(c, d, m, g, basis)
    J = [j for j in range(1, g) if any(v != 0 for v in chunks[j])]
    needed = set(J)
    for j in range(g - 1, 1, -1):
        if j in needed:
            needed.update(((j + 1) // 2, j // 2))
    lev = {e: k - delta(e) for e in range(1, nb + 1)}
    glev = {j: k - delta(m) - delta(j) for j in range(1, g) if j in needed}
    L_in = k - delta(mi)
    L_I = L_in - 1
    L_out = min([L_I] + [glev[j] for j in J])
    out_level = L_out - 1 if J else L_I
    if out_level < 1:
        raise ValueError("end of modulus switching chain reached")
    dbl = lambda row: float(q[row])
    sc, sub = {1: scale}, {}
    for e in range(2, nb + 1):
        hi, lo = (e + 1) // 2, e // 2
        L = lev[hi]
        prod = sc[hi] * sc[lo]
        sc[e] = prod / dbl(L - 1)
        if basis == 1:
            sub[e] = float(round(prod if hi == lo else prod / sc[1]))
    gsc = {}
    if g > 1:
        gsc[1] = sc[m]
    for j in range(2, g):
        if j in needed:
            hi, lo = (j + 1) // 2, j // 2
            gsc[j] = gsc[hi] * gsc[lo] / dbl(glev[hi] - 1)
    tau = {0: scale_out}
    sigma = 0.0
    if J:
        sigma = scale_out * dbl(L_out - 1)
        for j in J:
            tau[j] = sigma / gsc[j]
    W = np.zeros((g, mi, L_in), dtype=np.uint64)
    K = np.zeros((g, L_in), dtype=np.uint64)
    for j in [0] + J:
        up = tau[j] * dbl(L_in - 1)
        for i in range(1, mi + 1):
            W[j, i - 1] = residues(chunks[j][i] * (up / sc[i]), q[:L_in])
        K[j] = residues(chunks[j][0] * up, q[:L_in])
    n_products = (nb - 1) + len([j for j in needed if j >= 2]) + (1 if J else 0)
    return dict(d=d, m=m, g=g, mi=mi, nb=nb, basis=basis, k=k, q=q, chunks=chunks, J=J, needed=sorted(needed), lev=lev, sc=sc,
                sub=sub, glev=glev, gsc=gsc, L_in=L_in, L_I=L_I, L_out=L_out, out_level=out_level, out_scale=scale_out,
                sigma=sigma, tau=tau, W=W, K=K, n_products=n_products)


def _rows(x, L):
    """the ciphertext at level L: its first L rows"""
    return np.ascontiguousarray(np.asarray(x)[:, :L])


def _pad(x, size):
    out = np.zeros((size,) + x.shape[1:], dtype=np.uint64)
    out[:x.shape[0]] = x
    return out


def _mul_rescale(ref, L, a, b, key, merged):
    if merged:
        return KR.dot_product_rescale(ref, L, [a], [b], key)
    return KR.rescale(ref, L, DC.ckks_dot_product(ref, L, [a], [b], key))


def run(ref, pl, ct, relin_key, merged=True):
    """ct: [2][k][N] NTT form. Returns [2][out_level][N]."""
    q, k, basis = pl["q"], pl["k"], pl["basis"]
    E = {1: np.ascontiguousarray(ct, dtype=np.uint64)}
    for e in range(2, pl["nb"] + 1):
        hi, lo = (e + 1) // 2, e // 2
        L = pl["lev"][hi]
        a, b = _rows(E[hi], L), _rows(E[lo], L)
        if basis == 0:
            E[e] = _mul_rescale(ref, L, a, b, relin_key, merged)
            continue
        prod = DC.ckks_dot_product(ref, L, [a], [b], None)
        two = [2 % p for p in q[:L]]
        neg = residues(-pl["sub"][e], q[:L])
        if hi == lo:
            R = P.linear_combination(ref, L, [prod], [[two]], [neg])[0]
        else:
            R = P.linear_combination(ref, L, [prod, _pad(_rows(E[1], L), 3)], [[two, neg]])[0]
        if merged:
            E[e] = KR.relinearize_rescale(ref, L, R, relin_key)
        else:
            E[e] = KR.rescale(ref, L, DC._relin(ref, L, R, relin_key))
    Y = {}
    if pl["g"] > 1:
        Y[1] = E[pl["m"]]
    for j in pl["needed"]:
        if j >= 2:
            hi, lo = (j + 1) // 2, j // 2
            L = min(pl["glev"][hi], pl["glev"][lo])
            Y[j] = _mul_rescale(ref, L, _rows(Y[hi], L), _rows(Y[lo], L), relin_key, merged)
    L_in, J = pl["L_in"], pl["J"]
    formed = [0] + J
    sums = P.linear_combination(ref, L_in, [_rows(E[i], L_in) for i in range(1, pl["mi"] + 1)], pl["W"][formed], pl["K"][formed])
    I = {j: KR.rescale(ref, L_in, sums[s]) for s, j in enumerate(formed)}
    if not J:
        return I[0]
    Lo, out_level = pl["L_out"], pl["out_level"]
    ya, ib = [_rows(Y[j], Lo) for j in J], [_rows(I[j], Lo) for j in J]
    if merged:
        D = KR.dot_product_rescale(ref, Lo, ya, ib, relin_key)
    else:
        D = KR.rescale(ref, Lo, DC.ckks_dot_product(ref, Lo, ya, ib, relin_key))
    ones = [[[1] * out_level, [1] * out_level]]
    return P.linear_combination(ref, out_level, [D, _rows(I[0], out_level)], ones)[0]


def evaluate(ref, k, ct, scale, coeffs, relin_key=None, basis=0, n_baby=0, scale_out=0.0):
    """(plan, words): the definition of sealhip_evaluator_evaluate_polynomial_ckks's output"""
    pl = plan(ref.key_moduli[:ref.k_first], k, scale, coeffs, basis, n_baby, scale_out)
    return pl, run(ref, pl, ct, relin_key, True)


def composition(ref, k, ct, scale, coeffs, relin_key=None, basis=0, n_baby=0, scale_out=0.0):
    """the same plan, every merged step as its unmerged pair"""
    pl = plan(ref.key_moduli[:ref.k_first], k, scale, coeffs, basis, n_baby, scale_out)
    return pl, run(ref, pl, ct, relin_key, False)


def float_value(coeffs, basis, x):
    """p(x) in floating point for a scalar or an array"""
    if basis == 0:
        return np.polynomial.polynomial.polyval(x, coeffs)
    return np.polynomial.chebyshev.chebval(x, coeffs)
