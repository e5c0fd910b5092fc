"""CPU restatement of the hoisted rotation, from functions the oracle already has.

out_g = finish( (sigma_g(c0), 0), sum_j sigma_g(D_j) (.) K_g ) with D_j the rows switch_key_inplace multiplies with digit j of
the key for the target c1. The oracle has no entry that permutes the digits, so the restatement rests on
    sum_j sigma(D_j) (.) K = sigma( sum_j D_j (.) sigma^-1(K) ):
point-wise products commute with a permutation of the points, and the partial sum is canonical before it is permuted. The
key is permuted with g^-1, ref_switch_key_partial forms the canonical inner product, its rows are permuted with g, and
ref_switch_key_finish does the rest. This -- not repeated ref_apply_galois_inplace -- is what the device result equals."""
import ctypes as C

import numpy as np

import oracle_lib as O


def galois_table(logn, elt):
    tab = np.zeros(1 << logn, dtype=np.uint32)
    O.lib().ref_galois_table_ntt(logn, elt, tab.ctypes.data)
    return tab


def permute_rows_ntt(a, logn, elt):
    """apply_galois_ntt on every row of an array whose last axis is N"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    flat = a.reshape(-1, a.shape[-1])
    out = np.zeros_like(flat)
    for r in range(flat.shape[0]):
        O.lib().ref_apply_galois_ntt(O.ptr(flat[r]), logn, elt, O.ptr(out[r]))
    return out.reshape(a.shape)


def sigma_c0(ref, k, c0, elt):
    """the automorphism on component 0 in the form of the scheme's ciphertexts: NTT form for CKKS, coefficients for BFV"""
    c0 = np.ascontiguousarray(c0, dtype=np.uint64)
    if ref.scheme == 2:
        return permute_rows_ntt(c0, ref.logn, elt)
    out = np.zeros_like(c0)
    for r in range(k):
        O.lib().ref_apply_galois(O.ptr(c0[r]), ref.logn, elt, C.byref(ref.c.key_mod[r]), O.ptr(out[r]))
    return out


def hoisted_key(ref, key, elt):
    """sigma_{g^-1} on every row of the key (shared by all ciphertexts rotated with it)"""
    return permute_rows_ntt(key, ref.logn, pow(int(elt), -1, 2 * ref.n))


def hoisted_rotation(ref, k, ct, elt, key, key_inv=None):
    """ct: (2, k, N) at level k; key: (digits, 2, n_key, N) of element elt. Returns the (2, k, N) result."""
    L = O.lib()
    nd = (k + ref.nsp - 1) // ref.nsp  # of the level, not of the key
    if key_inv is None:
        key_inv = hoisted_key(ref, key, elt)
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    partial = np.zeros((2, k + ref.nsp, ref.n), dtype=np.uint64)
    assert L.ref_switch_key_partial(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(ct[1])), O.ptr(key_inv), 0, nd,
                                    O.ptr(partial)) == 0
    partial = permute_rows_ntt(partial, ref.logn, elt)
    out = np.zeros((2, k, ref.n), dtype=np.uint64)
    out[0] = sigma_c0(ref, k, ct[0], elt)
    assert L.ref_switch_key_finish(C.byref(ref.c), k, O.ptr(out), O.ptr(partial)) == 0
    return out


def hoisted_many(ref, k, cts, elts, keys):
    """cts: (count, 2, k, N) -> (len(elts), count, 2, k, N), the layout of sealhip_evaluator_apply_galois_many"""
    out = np.zeros((len(elts),) + cts.shape, dtype=np.uint64)
    for i, (elt, key) in enumerate(zip(elts, keys)):
        kinv = hoisted_key(ref, key, elt)
        for c in range(cts.shape[0]):
            out[i, c] = hoisted_rotation(ref, k, cts[c], elt, key, kinv)
    return out


def elt_from_step(n, step):
    return int(O.lib().ref_galois_elt_from_step(n, step, None))
