"""numpy restatement of the homomorphic DFT's matrices (include/sealhip.h), from the LAYERS: a stage is
built by applying its butterfly layers to the identity, O(r n^2); nothing here uses the closed form of the product that the
generator kernel evaluates. n = N/2 slots, L = log2 n, zeta = exp(i pi / N)."""
import numpy as np

C2S, S2C = 0, 1


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def bitrev_perm(n):
    bits = n.bit_length() - 1
    return np.array([bitrev(j, bits) for j in range(n)])


def pow5(n_ring):
    """5^j mod 2N for j < N/2"""
    out, pos = [], 1
    for _ in range(n_ring // 2):
        out.append(pos)
        pos = pos * 5 % (2 * n_ring)
    return out


def embedding(n_ring):
    """U[j][t] = zeta^((5^j mod 2N) t): slot values z = U w of w_t = m_t + i m_(t + n)"""
    n = n_ring // 2
    e = np.outer(np.array(pow5(n_ring), dtype=np.int64), np.arange(n, dtype=np.int64)) % (2 * n_ring)
    return np.exp(1j * np.pi * e / n_ring)


def layer(n, s):
    """F_s as a matrix: on every aligned block of 2^s, a = v[b+j], c = v[b+j+h] omega_(s,j): a + c, a - c"""
    ln, h = 1 << s, 1 << (s - 1)
    omega = [np.exp(2j * np.pi * (pow(5, j, 4 * ln)) / (4 * ln)) for j in range(h)]
    F = np.zeros((n, n), dtype=np.complex128)
    for b in range(0, n, ln):
        for j in range(h):
            F[b + j, b + j] = 1
            F[b + j, b + j + h] = omega[j]
            F[b + j + h, b + j] = 1
            F[b + j + h, b + j + h] = -omega[j]
    return F


def apply_layer(v, s, inverse=False):
    """F_s v (or F_s^-1 v = F_s^H v / 2) on the columns of v, by the butterflies"""
    n = v.shape[0]
    ln, h = 1 << s, 1 << (s - 1)
    omega = np.array([np.exp(2j * np.pi * (pow(5, j, 4 * ln)) / (4 * ln)) for j in range(h)])
    out = np.empty_like(v)
    for b in range(0, n, ln):
        top, bot = v[b:b + h], v[b + h:b + ln]
        w = omega.reshape((h,) + (1,) * (v.ndim - 1))
        if inverse:
            out[b:b + h] = (top + bot) / 2
            out[b + h:b + ln] = (top - bot) * np.conj(w) / 2
        else:
            c = bot * w
            out[b:b + h] = top + c
            out[b + h:b + ln] = top - c
    return out


def stage_layout(n_ring, direction, counts):
    """[(s0, r)] of the stages in application order: CoeffToSlot starts with the top layers, SlotToCoeff with the bottom"""
    L = (n_ring // 2).bit_length() - 1
    assert sum(counts) == L and all(c > 0 for c in counts)
    out, done = [], 0
    for r in counts:
        out.append((done + 1, r) if direction == S2C else (L - done - r + 1, r))
        done += r
    return out


def stage_matrix(n_ring, direction, s0, r):
    """The stage's matrix from its layers applied to the identity: F_(s0+r-1) ... F_s0 (SlotToCoeff) or
    F_s0^-1 ... F_(s0+r-1)^-1 (CoeffToSlot)"""
    n = n_ring // 2
    M = np.eye(n, dtype=np.complex128)
    order = range(s0, s0 + r) if direction == S2C else range(s0 + r - 1, s0 - 1, -1)
    for s in order:
        M = apply_layer(M, s, inverse=direction == C2S)
    return M


def default_n_baby(r):
    return 1 << ((r + 2) // 2)


def read_diagonals(M, s0, r):
    """{signed c: diag_c} of the non-zero generalized diagonals: diag_c[i] = M[i][i + c h0] taken over the integers (no
    wrap-around), read off the matrix. Also checks that nothing non-zero lies elsewhere."""
    n, h0 = M.shape[0], 1 << (s0 - 1)
    out, seen = {}, np.zeros_like(M, dtype=bool)
    for c in range(-(n // h0) + 1, n // h0):
        d = np.zeros(n, dtype=np.complex128)
        idx = np.arange(n)
        col = idx + c * h0
        ok = (col >= 0) & (col < n)
        d[ok] = M[idx[ok], col[ok]]
        seen[idx[ok], col[ok]] = True
        if np.any(d != 0):
            out[c] = d
    assert not np.any(M[~seen] != 0), "a non-zero off the h0-spaced diagonals"
    return out


def bsgs_grid(M, s0, r, n_baby=None):
    """(W[g][b], baby steps, giant steps) read off the matrix M of a stage: rotations are taken modulo n, so the diagonal of
    rotation t is d_t[i] = M[i][(i + t) mod n]; the grid holds the rotations t = (c_g n_baby + b) h0 mod n with c_g running
    over [-n_giant/2, n_giant/2) (or [0, n_giant) when the stage spans the whole vector), W[g][b] = d_t rotated by minus the
    giant step. Asserts that every non-zero of M is covered exactly once."""
    n, h0 = M.shape[0], 1 << (s0 - 1)
    folded = (h0 << r) == n
    n_baby = n_baby or default_n_baby(r)
    n_diag = (1 << r) if folded else (2 << r)
    n_giant = n_diag // n_baby
    idx = np.arange(n)
    W = np.zeros((n_giant, n_baby, n), dtype=np.complex128)
    baby = [b * h0 for b in range(n_baby)]
    giant, covered = [], np.zeros((n, n), dtype=int)
    for g in range(n_giant):
        cg = g if folded else g - n_giant // 2
        G = (cg * n_baby * h0) % n
        giant.append(G)
        for b in range(n_baby):
            t = (G + baby[b]) % n
            d = M[idx, (idx + t) % n]
            covered[idx, (idx + t) % n] += 1
            W[g, b] = d[(idx - G) % n]  # rot_(-G): slot p holds d[p - G]
    assert np.all(covered[M != 0] == 1), "a non-zero is covered by no cell, or by two"
    return W, baby, giant


def rot(v, s):
    """rotate_vector by s: slot j + s moves to slot j"""
    return np.roll(v, -s, axis=-1)


def bsgs_apply(W, baby, giant, v):
    """sum_g rot_g( sum_b W[g][b] (.) rot_b v )"""
    out = np.zeros_like(v, dtype=np.complex128)
    for g, G in enumerate(giant):
        inner = sum(W[g, b] * rot(v, B) for b, B in enumerate(baby))
        out = out + rot(inner, G)
    return out


def stage_gain(direction, t, n_stages, gain=1.0):
    """the real factor on stage t beyond its matrix: 1/2 (the split) and gain on the last CoeffToSlot stage, gain on the first
    SlotToCoeff stage"""
    if direction == C2S:
        return 0.5 * gain if t == n_stages - 1 else 1.0
    return gain if t == 0 else 1.0


def stage_values(n_ring, direction, counts, t, n_baby=None, gain=1.0):
    """what sealhip_dft_stage_values returns for stage t: the grid of the stage's matrix times its gain"""
    s0, r = stage_layout(n_ring, direction, counts)[t]
    W, _, _ = bsgs_grid(stage_matrix(n_ring, direction, s0, r), s0, r, n_baby[t] if n_baby else None)
    return W * stage_gain(direction, t, len(counts), gain)


def compositions(total, max_parts):
    """every ordered split of `total` into 1 .. max_parts positive parts"""
    def rec(left, parts):
        if left == 0:
            yield list(parts)
            return
        if len(parts) == max_parts:
            return
        for first in range(1, left + 1):
            yield from rec(left - first, parts + [first])
    return list(rec(total, []))
