"""CPU restatement of the key switch's mod-down merged with the CKKS rescale, from functions the
oracle and the other restatements already have.

    out = floor( (P * base + acc + half) / D )  row by row,  D = P * q_{k-1},  half = floor(D / 2)

base: (2, k, N) NTT form; acc: (2, k + nsp, N) NTT form, row r modulo key prime rp(r) -- the two operands of
ref_switch_key_finish. Per component and coefficient:
1. the dropped rows in coefficient form: y_l = intt((acc[k-1] + (P mod l) * base[k-1]) mod l), y_{p_j} = intt(acc[k+j]);
2. z_d = ((y_d + half) mod d) * ((D/d)^-1 mod d) mod d for d in Dset = (l, p_0, .., p_{nsp-1});
3. v = ( sum_d floor(z_d * C_d / 2^64) ) >> 64 with C_d = floor(2^128 / d): the integer formula defines the words;
4. temp_r = ( sum_d z_d * ((D/d) mod q_r) - v * (D mod q_r) - (half mod q_r) ) mod q_r, then the exact forward transform;
5. out[r] = ( acc[r] + (P mod q_r) * base[r] - temp_r ) * (D^-1 mod q_r) mod q_r, for r < k - 1.
The per-operation restatements apply finish_rescale where the unmerged ones apply ref_switch_key_finish. This -- not the
unmerged operation followed by ref_mod_switch_scale_to_next -- is what the device result equals."""
import ctypes as C

import numpy as np

import dot_ct_ref as DC
import hoist_bsgs_ref as BS
import hoist_dot_ref as HD
import hoist_ref as H
import oracle_lib as O


def dropped_set(ref, k):
    """(Dset, P, D, half) at level k, Python integers"""
    q = ref.key_moduli
    sp = [int(q[ref.n_key - ref.nsp + j]) for j in range(ref.nsp)]
    P = 1
    for p in sp:
        P *= p
    D = P * int(q[k - 1])
    return [int(q[k - 1])] + sp, P, D, D // 2


def quotient(z, dset):
    """step 3 for one coefficient (or an object array of coefficients per prime): z[i] canonical modulo dset[i]"""
    total = 0
    for zi, d in zip(z, dset):
        total = total + ((zi * ((1 << 128) // d)) >> 64)
    return total >> 64


def scaled_residues(y, dset, D, half):
    """step 2: y[i] canonical modulo dset[i]"""
    return [((yi + half) % d) * pow((D // d) % d, -1, d) % d for yi, d in zip(y, dset)]


def convert(z, v, dset, D, half, qr):
    """step 4 before the transform"""
    t = -v * (D % qr) - (half % qr)
    for zi, d in zip(z, dset):
        t = t + zi * ((D // d) % qr)
    return t % qr


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=object).astype(np.uint64))


def finish_rescale(ref, k, base, acc=None):
    """base: (2, k, N); acc: (2, k + nsp, N) or None (no key-switch term was formed). Returns (2, k - 1, N)."""
    assert ref.scheme == 2 and 2 <= k <= ref.k_first
    L = O.lib()
    n, nsp = ref.n, ref.nsp
    q = [int(p) for p in ref.key_moduli]
    dset, P, D, half = dropped_set(ref, k)
    l = dset[0]
    base = np.ascontiguousarray(base, dtype=np.uint64)
    acc = np.zeros((2, k + nsp, n), dtype=np.uint64) if acc is None else np.ascontiguousarray(acc, dtype=np.uint64)
    out = np.zeros((2, k - 1, n), dtype=np.uint64)
    for c2 in range(2):
        y = []
        row = _u64((_obj(acc[c2, k - 1]) + (P % l) * _obj(base[c2, k - 1])) % l)
        L.ref_ntt_inverse(O.ptr(row), ref.tables(k - 1))
        y.append(_obj(row))
        for j in range(nsp):
            row = acc[c2, k + j].copy()
            L.ref_ntt_inverse(O.ptr(row), ref.tables(ref.n_key - nsp + j))
            y.append(_obj(row))
        z = scaled_residues(y, dset, D, half)
        v = quotient(z, dset)
        for r in range(k - 1):
            temp = _u64(convert(z, v, dset, D, half, q[r]))
            L.ref_ntt_forward(O.ptr(temp), ref.tables(r), 1)
            w = (_obj(acc[c2, r]) + (P % q[r]) * _obj(base[c2, r]) - _obj(temp)) * pow(D % q[r], -1, q[r]) % q[r]
            out[c2, r] = _u64(w)
    return out


def key_switch_acc(ref, k, target, key):
    """ref_switch_key_partial of one polynomial (k, N) over all digits: (2, k + nsp, N)"""
    nd = (k + ref.nsp - 1) // ref.nsp
    acc = np.zeros((2, k + ref.nsp, ref.n), dtype=np.uint64)
    key = np.ascontiguousarray(key, dtype=np.uint64)
    assert O.lib().ref_switch_key_partial(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(target, dtype=np.uint64)), O.ptr(key), 0,
                                          nd, O.ptr(acc)) == 0
    return acc


def relinearize_rescale(ref, k, ct3, relin_key):
    """ct3: (3, k, N) -> (2, k - 1, N)"""
    ct3 = np.ascontiguousarray(ct3, dtype=np.uint64)
    return finish_rescale(ref, k, ct3[:2], key_switch_acc(ref, k, ct3[2], relin_key))


def dot_product_rescale(ref, k, a_terms, b_terms, relin_key):
    return relinearize_rescale(ref, k, DC.ckks_dot_product(ref, k, a_terms, b_terms, None), relin_key)


def dot_plain_rescale_one(ref, k, ct, elts, keys, plains, keys_inv=None):
    """ct: (2, k, N); plains: (n_sums, n_elts, n_key, N). Returns (n_sums, 2, k - 1, N)."""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    prods = HD.products(ref, k, ct, elts, keys, keys_inv)
    cn = HD.ntt_form(ref, k, ct)
    sig0 = [cn[0] if g == 1 else H.permute_rows_ntt(cn[0], ref.logn, g) for g in elts]
    out = np.zeros((plains.shape[0], 2, k - 1, ref.n), dtype=np.uint64)
    for s in range(plains.shape[0]):
        base, acc = BS.inner_parts(ref, k, elts, plains[s], prods, cn, sig0)
        out[s] = finish_rescale(ref, k, base, acc)
    return out


def dot_plain_rescale(ref, k, cts, elts, keys, plains):
    """cts: (count, 2, k, N) -> (n_sums, count, 2, k - 1, N)"""
    keys_inv = [None if g == 1 else H.hoisted_key(ref, key, g) for g, key in zip(elts, keys)]
    out = np.zeros((plains.shape[0], cts.shape[0], 2, k - 1, ref.n), dtype=np.uint64)
    for c in range(cts.shape[0]):
        out[:, c] = dot_plain_rescale_one(ref, k, cts[c], elts, keys, plains, keys_inv)
    return out


def bsgs_plain_rescale_one(ref, k, ct, baby, baby_keys, giant, giant_keys, plains, baby_inv=None, giant_inv=None):
    """steps 1-3 of tests/hoist_bsgs_ref.py as they are (CKKS), then finish_rescale(BASE, ACC). Returns (2, k - 1, N)."""
    L = O.lib()
    n, rows = ref.n, k + ref.nsp
    q_primes = list(range(k))
    e_primes = [HD.row_prime(ref, k, r) for r in range(rows)]
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    prods = HD.products(ref, k, ct, baby, baby_keys, baby_inv)
    cn = HD.ntt_form(ref, k, ct)
    sig0 = [cn[0] if g == 1 else H.permute_rows_ntt(cn[0], ref.logn, g) for g in baby]
    BASE = np.zeros((2, k, n), dtype=np.uint64)
    ACC = np.zeros((2, rows, n), dtype=np.uint64)
    formed = False
    for j, h in enumerate(giant):
        base, acc = BS.inner_parts(ref, k, baby, plains[j], prods, cn, sig0)
        if h == 1:
            for c2 in range(2):
                BS._add_rows(ref, q_primes, BASE[c2], base[c2])
                if acc is not None:
                    BS._add_rows(ref, e_primes, ACC[c2], acc[c2])
            formed = formed or acc is not None
            continue
        target = np.zeros((2, k, n), dtype=np.uint64)
        target[1] = base[1]
        if acc is not None:
            half = np.zeros((2, rows, n), dtype=np.uint64)
            half[1] = acc[1]
            assert L.ref_switch_key_finish(C.byref(ref.c), k, O.ptr(target), O.ptr(half)) == 0
            target[0] = 0
        inv = None if giant_inv is None else [giant_inv[j]]
        prod = HD.products(ref, k, target, [h], [giant_keys[j]], inv)[0]
        for c2 in range(2):
            BS._add_rows(ref, e_primes, ACC[c2], prod[c2])
        if acc is not None:
            BS._add_rows(ref, e_primes, ACC[0], H.permute_rows_ntt(acc[0], ref.logn, h))
        BS._add_rows(ref, q_primes, BASE[0], H.permute_rows_ntt(base[0], ref.logn, h))
        formed = True
    return finish_rescale(ref, k, BASE, ACC if formed else None)


def bsgs_plain_rescale(ref, k, cts, baby, baby_keys, giant, giant_keys, plains):
    """cts: (count, 2, k, N) -> (count, 2, k - 1, N)"""
    baby_inv = [None if g == 1 else H.hoisted_key(ref, key, g) for g, key in zip(baby, baby_keys)]
    giant_inv = [None if g == 1 else H.hoisted_key(ref, key, g) for g, key in zip(giant, giant_keys)]
    out = np.zeros((cts.shape[0], 2, k - 1, ref.n), dtype=np.uint64)
    for c in range(cts.shape[0]):
        out[c] = bsgs_plain_rescale_one(ref, k, cts[c], baby, baby_keys, giant, giant_keys, plains, baby_inv, giant_inv)
    return out


def rescale(ref, k, ct):
    """ref_mod_switch_scale_to_next of a size-2 ciphertext (2, k, N) -> (2, k - 1, N): the second half of the composition"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    out = np.zeros((2, k - 1, ref.n), dtype=np.uint64)
    assert O.lib().ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(ct), 2, O.ptr(out)) == 0
    return out
