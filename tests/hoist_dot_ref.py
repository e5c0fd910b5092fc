"""CPU restatement of the plaintext-weighted sum of rotations, from functions the oracle already has.

out_s = finish( base_s, acc_s ) with
    acc_s  = sum_{i : g_i != 1} W[s][i] (.) prod_{g_i}      on the k + nsp extended rows, row r modulo key prime rp(r),
    base_s = ( sum_i W[s][i] (.) sigma_{g_i}(C_0), sum_{i : g_i = 1} W[s][i] (.) C_1 )   on the k ciphertext rows,
prod_g the hoisted rotation's inner product (tests/hoist_ref.py: the key permuted with g^-1, ref_switch_key_partial, the rows
permuted with g) and C the NTT form of the ciphertext's components. Every sum is canonical, so the order of the terms does
not matter. This -- not apply_galois_many + multiply_plain_ntt + add -- is what the device result equals."""
import ctypes as C

import numpy as np

import hoist_ref as H
import oracle_lib as O


def row_prime(ref, k, r):
    """the key prime of extended row r at level k (KsDev::row_prime)"""
    return r if r < k else ref.n_key - ref.nsp + (r - k)


def _mul_add(ref, prime, w, x, into):
    """into += w (.) x modulo key prime `prime`, in place"""
    L = O.lib()
    mod = C.byref(ref.c.key_mod[prime])
    t = np.zeros(ref.n, dtype=np.uint64)
    L.ref_dyadic_product_coeffmod(O.ptr(np.ascontiguousarray(w)), O.ptr(np.ascontiguousarray(x)), ref.n, mod, O.ptr(t))
    L.ref_add_poly_coeffmod(O.ptr(into), O.ptr(t), ref.n, mod, O.ptr(into))


def ntt_form(ref, k, ct):
    """C of section 16: the components themselves for CKKS, their canonical forward transform for BFV"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    if ref.scheme == 2:
        return ct
    out = ct.copy()
    for l in range(2):
        for r in range(k):
            O.lib().ref_ntt_forward(O.ptr(out[l, r]), ref.tables(r), 1)
    return out


def products(ref, k, ct, elts, keys, keys_inv=None):
    """prod_g of every element g != 1 (None for the identity): (2, k + nsp, N) canonical words"""
    L = O.lib()
    nd = (k + ref.nsp - 1) // ref.nsp
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    out = []
    for i, g in enumerate(elts):
        if g == 1:
            out.append(None)
            continue
        kinv = keys_inv[i] if keys_inv is not None else H.hoisted_key(ref, keys[i], g)
        partial = np.zeros((2, k + ref.nsp, ref.n), dtype=np.uint64)
        assert L.ref_switch_key_partial(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(ct[1])), O.ptr(kinv), 0, nd,
                                        O.ptr(partial)) == 0
        out.append(H.permute_rows_ntt(partial, ref.logn, g))
    return out


def dot_plain_one(ref, k, ct, elts, keys, plains, keys_inv=None):
    """ct: (2, k, N); plains: (n_sums, n_elts, n_key, N) in key-level NTT form. Returns (n_sums, 2, k, N)."""
    L = O.lib()
    n, rows = ref.n, k + ref.nsp
    prods = products(ref, k, ct, elts, keys, keys_inv)
    cn = ntt_form(ref, k, ct)
    sig0 = [cn[0] if g == 1 else H.permute_rows_ntt(cn[0], ref.logn, g) for g in elts]
    out = np.zeros((plains.shape[0], 2, k, n), dtype=np.uint64)
    for s in range(plains.shape[0]):
        base = np.zeros((2, k, n), dtype=np.uint64)
        acc = np.zeros((2, rows, n), dtype=np.uint64)
        for i, g in enumerate(elts):
            for r in range(k):
                _mul_add(ref, r, plains[s, i, r], sig0[i][r], base[0, r])
                if g == 1:
                    _mul_add(ref, r, plains[s, i, r], cn[1, r], base[1, r])
            if g != 1:
                for l in range(2):
                    for r in range(rows):
                        rp = row_prime(ref, k, r)
                        _mul_add(ref, rp, plains[s, i, rp], prods[i][l, r], acc[l, r])
        if ref.scheme != 2:
            for l in range(2):
                for r in range(k):
                    L.ref_ntt_inverse(O.ptr(base[l, r]), ref.tables(r))
        if any(g != 1 for g in elts):
            assert L.ref_switch_key_finish(C.byref(ref.c), k, O.ptr(base), O.ptr(acc)) == 0
        out[s] = base
    return out


def dot_plain(ref, k, cts, elts, keys, plains, items=None):
    """cts: (count, 2, k, N) -> (n_sums, count, 2, k, N), the layout of sealhip_evaluator_apply_galois_dot_plain; only the
    ciphertexts of `items` are computed when given (the others stay zero)"""
    keys_inv = [None if g == 1 else H.hoisted_key(ref, key, g) for g, key in zip(elts, keys)]
    out = np.zeros((plains.shape[0],) + cts.shape, dtype=np.uint64)
    for c in (range(cts.shape[0]) if items is None else items):
        out[:, c] = dot_plain_one(ref, k, cts[c], elts, keys, plains, keys_inv)
    return out


def composed_one(ref, k, ct, elts, keys, plains_s):
    """the composition the fused operation replaces: the hoisted rotation per element, the plaintext product with the
    plaintext's leading k rows, the add. CKKS (NTT-form ciphertexts) multiplies directly; BFV goes through the transform.
    plains_s: (n_elts, n_key, N). Returns (2, k, N)."""
    L = O.lib()
    total = np.zeros((2, k, ref.n), dtype=np.uint64)
    for i, g in enumerate(elts):
        rot = np.ascontiguousarray(ct, dtype=np.uint64).copy() if g == 1 else H.hoisted_rotation(ref, k, ct, g, keys[i])
        if ref.scheme != 2:
            rot = ntt_form(ref, k, rot)
        term = np.zeros_like(total)
        for l in range(2):
            for r in range(k):
                _mul_add(ref, r, plains_s[i, r], rot[l, r], term[l, r])
        if ref.scheme != 2:
            for l in range(2):
                for r in range(k):
                    L.ref_ntt_inverse(O.ptr(term[l, r]), ref.tables(r))
        for l in range(2):
            for r in range(k):
                L.ref_add_poly_coeffmod(O.ptr(total[l, r]), O.ptr(term[l, r]), ref.n, C.byref(ref.c.key_mod[r]),
                                        O.ptr(total[l, r]))
    return total


def lift_plain(ref, coeffs):
    """an integer polynomial (centred coefficients) in key-level NTT form: (n_key, N)"""
    out = np.zeros((ref.n_key, ref.n), dtype=np.uint64)
    for r, p in enumerate(ref.key_moduli):
        out[r] = np.array([int(v) % p for v in coeffs], dtype=np.uint64)
        O.lib().ref_ntt_forward(O.ptr(out[r]), ref.tables(r), 1)
    return out
