"""CPU restatement of the baby-step/giant-step matrix-vector product with the giant steps in the extended basis (DESIGN.md
section 17), from functions tests/hoist_dot_ref.py, tests/hoist_ref.py and the oracle already have.

    out = sum_j sigma_{h_j}( sum_i W[j][i] * sigma_{g_i}(ct) )

1. base_j (k rows, NTT form) and acc_j (k + nsp rows) are section 16's parts of inner sum j before its finish.
2. d_j (h_j != 1) = component 1 of ref_switch_key_finish on (0, base_j[1]) and (0, acc_j[1]); BFV's base_j[1] goes through the
   canonical inverse transform first; without acc_j, d_j = base_j[1].
3. ACC (k + nsp rows) and BASE (k rows) collect, canonically: for h_j = 1 acc_j and base_j as they are; else the giant's
   inner product (HD.products on a ciphertext whose component 1 is d_j), the permuted acc_j[0], and the permuted base_j[0].
4. BFV: the canonical inverse transform of BASE. out = ref_switch_key_finish(BASE, ACC), or BASE when no ACC term was formed.
This -- not dot_plain + apply_galois + add -- is what the device result equals."""
import ctypes as C

import numpy as np

import hoist_dot_ref as HD
import hoist_ref as H
import oracle_lib as O


def _add_rows(ref, primes, into, x):
    """into[r] += x[r] modulo key prime primes[r], canonical, in place"""
    for r, prime in enumerate(primes):
        O.lib().ref_add_poly_coeffmod(O.ptr(into[r]), O.ptr(np.ascontiguousarray(x[r])), ref.n, C.byref(ref.c.key_mod[prime]),
                                      O.ptr(into[r]))


def _intt_rows(ref, k, a):
    for r in range(k):
        O.lib().ref_ntt_inverse(O.ptr(a[r]), ref.tables(r))


def inner_parts(ref, k, baby, plains_j, prods, cn, sig0):
    """section 16's steps 1-3 for one sum, before the finish: base (2, k, N) in NTT form and acc (2, k + nsp, N), or None when
    no baby element differs from 1. plains_j: (n_baby, n_key, N)."""
    n, rows = ref.n, k + ref.nsp
    base = np.zeros((2, k, n), dtype=np.uint64)
    acc = np.zeros((2, rows, n), dtype=np.uint64) if any(g != 1 for g in baby) else None
    for i, g in enumerate(baby):
        for r in range(k):
            HD._mul_add(ref, r, plains_j[i, r], sig0[i][r], base[0, r])
            if g == 1:
                HD._mul_add(ref, r, plains_j[i, r], cn[1, r], base[1, r])
        if g != 1:
            for l in range(2):
                for r in range(rows):
                    rp = HD.row_prime(ref, k, r)
                    HD._mul_add(ref, rp, plains_j[i, rp], prods[i][l, r], acc[l, r])
    return base, acc


def bsgs_one(ref, k, ct, baby, baby_keys, giant, giant_keys, plains, baby_inv=None, giant_inv=None):
    """ct: (2, k, N); plains: (n_giant, n_baby, n_key, N) in key-level NTT form. Returns (2, k, N)."""
    L = O.lib()
    n, rows = ref.n, k + ref.nsp
    bfv = ref.scheme != 2
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
        base, acc = inner_parts(ref, k, baby, plains[j], prods, cn, sig0)
        if h == 1:
            for l in range(2):
                _add_rows(ref, q_primes, BASE[l], base[l])
                if acc is not None:
                    _add_rows(ref, e_primes, ACC[l], acc[l])
            formed = formed or acc is not None
            continue
        target = np.zeros((2, k, n), dtype=np.uint64)
        target[1] = base[1]
        if bfv:
            _intt_rows(ref, k, target[1])
        if acc is not None:
            half = np.zeros((2, rows, n), dtype=np.uint64)
            half[1] = acc[1]
            assert L.ref_switch_key_finish(C.byref(ref.c), k, O.ptr(target), O.ptr(half)) == 0
            target[0] = 0  # (component 0 of this finish is not part of the definition: d_j is component 1 alone)
        inv = None if giant_inv is None else [giant_inv[j]]
        prod = HD.products(ref, k, target, [h], [giant_keys[j]], inv)[0]
        for l in range(2):
            _add_rows(ref, e_primes, ACC[l], prod[l])
        if acc is not None:
            _add_rows(ref, e_primes, ACC[0], H.permute_rows_ntt(acc[0], ref.logn, h))
        _add_rows(ref, q_primes, BASE[0], H.permute_rows_ntt(base[0], ref.logn, h))
        formed = True
    if bfv:
        for l in range(2):
            _intt_rows(ref, k, BASE[l])
    if formed:
        assert L.ref_switch_key_finish(C.byref(ref.c), k, O.ptr(BASE), O.ptr(ACC)) == 0
    return BASE


def bsgs(ref, k, cts, baby, baby_keys, giant, giant_keys, plains, items=None):
    """cts: (count, 2, k, N) -> (count, 2, k, N), the layout of sealhip_evaluator_apply_galois_bsgs_plain; only the ciphertexts
    of `items` are computed when given (the others stay zero)"""
    baby_inv = [None if g == 1 else H.hoisted_key(ref, key, g) for g, key in zip(baby, baby_keys)]
    giant_inv = [None if g == 1 else H.hoisted_key(ref, key, g) for g, key in zip(giant, giant_keys)]
    out = np.zeros(cts.shape, dtype=np.uint64)
    for c in (range(cts.shape[0]) if items is None else items):
        out[c] = bsgs_one(ref, k, cts[c], baby, baby_keys, giant, giant_keys, plains, baby_inv, giant_inv)
    return out


def composed_one(ref, k, ct, baby, baby_keys, giant, giant_keys, plains):
    """the composition the fused operation replaces: HD.dot_plain for the inner sums, the hoisted rotation of each by its giant
    element, the adds. Returns (2, k, N)."""
    inner = HD.dot_plain_one(ref, k, ct, baby, baby_keys, plains)
    total = np.zeros((2, k, ref.n), dtype=np.uint64)
    for j, h in enumerate(giant):
        rot = inner[j] if h == 1 else H.hoisted_rotation(ref, k, inner[j], h, giant_keys[j])
        for l in range(2):
            _add_rows(ref, list(range(k)), total[l], rot[l])
    return total
