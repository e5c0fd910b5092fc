"""numpy restatement of the matrix-vector product from a caller's matrix: the occupancy scan, the
plan and the grid of pre-rotated diagonals, written from the definition in include/sealhip.h and not from the library's code.

n slots, M a d x d complex matrix, d a power of two <= n. Diagonal c is u_c[p] = M[p mod d][(p + c) mod d], p < n, and
    out[p] = sum_{c in D} u_c[p] z[(p + c) mod n].
rot(v, s)[p] = v[(p + s) mod n] is what a rotation by step s does to the slots."""
import numpy as np


def diagonal(M, n, c):
    """u_c as n values"""
    d = M.shape[0]
    p = np.arange(n)
    return M[p % d, (p + c) % d]


def occupancy(M):
    """(d flags: the diagonal holds a non-zero entry, re or im; whether every entry is finite). -0.0 is zero."""
    d = M.shape[0]
    i = np.arange(d)
    occ = np.array([1 if np.any((M[i, (i + c) % d].real != 0) | (M[i, (i + c) % d].imag != 0)) else 0 for c in range(d)],
                   dtype=np.uint8)
    return occ, bool(np.all(np.isfinite(M.real)) and np.all(np.isfinite(M.imag)))


def steps_for(mask, n1):
    D = [c for c in range(len(mask)) if mask[c]]
    return sorted({c % n1 for c in D}), sorted({c - c % n1 for c in D})


def default_n1(mask):
    """the power of two minimising nb + 2 ng over the non-zero steps, ties to the larger"""
    best, best_cost, n1 = 1, None, 1
    while n1 <= len(mask):
        baby, giant = steps_for(mask, n1)
        cost = sum(1 for b in baby if b) + 2 * sum(1 for g in giant if g)
        if best_cost is None or cost <= best_cost:
            best, best_cost = n1, cost
        n1 *= 2
    return best


def plan(n, d, mask=None, n1=0):
    """dict: d, n_diagonals, n1, n_baby, n_giant, baby_steps, giant_steps, key_steps"""
    mask = np.ones(d, dtype=np.uint8) if mask is None else (np.asarray(mask) != 0).astype(np.uint8)
    assert d >= 1 and d & (d - 1) == 0 and d <= n and mask.size == d and mask.any()
    n1 = n1 or default_n1(mask)
    assert n1 & (n1 - 1) == 0 and n1 <= d
    baby, giant = steps_for(mask, n1)
    return {"d": d, "n_diagonals": int(mask.sum()), "n1": n1, "n_baby": len(baby), "n_giant": len(giant), "baby_steps": baby,
            "giant_steps": giant, "key_steps": sorted({s for s in baby + giant if s}), "mask": mask}


def values(M, n, mask=None, n1=0, gain=1.0):
    """values[gi][bi][p] = gain * u_(g+b)[(p - g) mod n], zero where g + b is not in D; re and im are multiplied by the
    real gain separately (a complex product with gain + 0j would add signed zeros and spoil infinities)"""
    d = M.shape[0]
    pl = plan(n, d, mask, n1)
    out = np.zeros((pl["n_giant"], pl["n_baby"], n), dtype=np.complex128)
    p = np.arange(n)
    for gi, g in enumerate(pl["giant_steps"]):
        for bi, b in enumerate(pl["baby_steps"]):
            if pl["mask"][g + b]:
                u = diagonal(M, n, g + b)[(p - g) % n]
                out[gi, bi].real = u.real * gain
                out[gi, bi].imag = u.imag * gain
    return out, pl


def rot(v, s):
    return np.roll(v, -s)


def apply_definition(M, z, mask=None):
    """out[p] = sum_{c in D} u_c[p] z[(p + c) mod n]"""
    n, d = len(z), M.shape[0]
    mask = np.ones(d, dtype=np.uint8) if mask is None else mask
    out = np.zeros(n, dtype=np.complex128)
    for c in range(d):
        if mask[c]:
            out += diagonal(M, n, c) * rot(z, c)
    return out


def apply_grid(W, baby, giant, z):
    """sum_g rot(sum_b W[g][b] * rot(z, b), g): what the BSGS entry computes on the slots"""
    out = np.zeros(len(z), dtype=np.complex128)
    for gi, g in enumerate(giant):
        inner = np.zeros(len(z), dtype=np.complex128)
        for bi, b in enumerate(baby):
            inner += W[gi, bi] * rot(z, b)
        out += rot(inner, g)
    return out


def masks(d, rng, n_random):
    """the named masks of the tests, then n_random seeded ones (never empty)"""
    out = [np.ones(d, dtype=np.uint8)]
    one = np.zeros(d, dtype=np.uint8)
    one[0] = 1
    out.append(one)
    if d > 1:
        single = np.zeros(d, dtype=np.uint8)
        single[d - 1 if d < 4 else d // 2 + 1] = 1
        band = np.zeros(d, dtype=np.uint8)
        band[[0, 1, d - 1]] = 1
        other = (np.arange(d) % 2 == 0).astype(np.uint8)
        out += [single, band, other]
    for _ in range(n_random):
        m = (rng.random(d) < rng.random()).astype(np.uint8)
        if not m.any():
            m[rng.integers(0, d)] = 1
        out.append(m)
    return out


def masked_matrix(d, mask, rng):
    """a random complex d x d matrix whose non-zero diagonals are exactly those of mask"""
    M = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    i = np.arange(d)
    for c in range(d):
        if not mask[c]:
            M[i, (i + c) % d] = 0
    return M
