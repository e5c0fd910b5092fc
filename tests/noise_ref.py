"""Decryptor::invariant_noise_budget (decryptor.cpp:269-325) restated with Python integers, and ciphertexts with a planted
budget, for tests/test_decryptor_host.py and tests/test_gpu_decryptor.py.

The restatement, from the dot product v = c_0 + c_1 s + ... (k x N canonical residues, coefficient form):
  1. w = t v mod q_i;  2. W = CRT(w) in [0, Q);  3. |W| = Q - W if W >= (Q + 1) / 2, else W;  4. norm = max |W|;
  5. budget = max(0, bits(Q) - bits(norm) - 1).

Planting: for signed targets X_c with |X_c| <= (Q - 1) / 2, a dot product v = X t^{-1} mod Q gives t v = X (mod Q), so the
norm is max |X_c| and the budget follows from it alone. Small targets are reduced per row with the oracle's
multiply_poly_scalar_coeffmod; the few large ones are done one by one with Python integers."""
import ctypes as C

import numpy as np

import oracle_lib as O


def prod(mods):
    q = 1
    for p in mods:
        q *= int(p)
    return q


def budget_from_norm(norm, q):
    return max(0, q.bit_length() - int(norm).bit_length() - 1)


def ref_noise_budget(v, mods, t):
    """the five steps on one dot product v (k x N), exact"""
    mods = [int(p) for p in mods]
    q = prod(mods)
    acc = np.zeros(v.shape[1], dtype=object)
    for r, p in enumerate(mods):
        punct = q // p
        inv = pow(punct % p, -1, p)
        w = (v[r].astype(object) * (t % p)) % p  # multiply_poly_scalar_coeffmod
        acc = (acc + (w * inv % p) * punct) % q  # compose_array
    half = (q + 1) >> 1
    centred = np.where(acc >= half, q - acc, acc)
    return budget_from_norm(max(centred) if len(centred) else 0, q)


def planted_rows(x_small, big, mods, t):
    """k x N residues of X t^{-1} mod Q: x_small a signed int64 array (|x| < 2^62), big {coefficient: Python int} overrides"""
    L = O.lib()
    mods = [int(p) for p in mods]
    q = prod(mods)
    n = len(x_small)
    rows = np.zeros((len(mods), n), dtype=np.uint64)
    x = np.asarray(x_small, dtype=np.int64)
    for r, p in enumerate(mods):
        red = np.ascontiguousarray((x % np.int64(p)).astype(np.uint64))
        mod = O.modulus(p)
        L.ref_multiply_poly_scalar_coeffmod(O.ptr(red), n, pow(t % p, -1, p), C.byref(mod), O.ptr(rows[r]))
    tinv = pow(t, -1, q)
    for c, val in big.items():
        w = (int(val) * tinv) % q
        for r, p in enumerate(mods):
            rows[r, c] = w % p
    return rows


def planted_budget(x_small, big, mods):
    q = prod(mods)
    norm = int(np.abs(np.asarray(x_small, dtype=np.int64)).max()) if len(x_small) else 0
    for val in big.values():
        norm = max(norm, abs(int(val)))
    return budget_from_norm(norm, q)


def random_sk_powers(mods, logn, count, rng):
    """s, s^2, ... (NTT form, rows of the given primes) for a uniformly random NTT-form s"""
    L = O.lib()
    n = 1 << logn
    sk = np.stack([rng.integers(0, int(p), size=n, dtype=np.uint64) for p in mods])
    out = np.zeros((count, len(mods), n), dtype=np.uint64)
    cur = sk.copy()
    for i in range(count):
        out[i] = cur
        nxt = np.zeros_like(cur)
        for r, p in enumerate(mods):
            mod = O.modulus(int(p))
            L.ref_dyadic_product_coeffmod(O.ptr(cur[r]), O.ptr(sk[r]), n, C.byref(mod), O.ptr(nxt[r]))
        cur = nxt
    return out


def ciphertext_with_dot(rows, size, pw, mods, logn, rng, tables=None):
    """size x k x N ciphertext (coefficient form) with random c_1.. and c_0 chosen so that its dot product with the key
    powers pw (NTT form, key-level rows) is `rows`"""
    L = O.lib()
    k, n = rows.shape
    mods = [int(p) for p in mods[:k]]
    ct = np.zeros((size, k, n), dtype=np.uint64)
    ct[0] = rows
    tables = tables or [O.Tables(logn, p) for p in mods]
    for j in range(1, size):
        for r, p in enumerate(mods):
            ct[j, r] = rng.integers(0, p, size=n, dtype=np.uint64)
            mod = O.modulus(p)
            row = ct[j, r].copy()
            L.ref_ntt_forward(O.ptr(row), C.byref(tables[r].t), 0)
            L.ref_dyadic_product_coeffmod(O.ptr(row), O.ptr(pw[j - 1, r]), n, C.byref(mod), O.ptr(row))
            L.ref_ntt_inverse(O.ptr(row), C.byref(tables[r].t))
            L.ref_sub_poly_coeffmod(O.ptr(ct[0, r]), O.ptr(row), n, C.byref(mod), O.ptr(ct[0, r]))
    return ct

