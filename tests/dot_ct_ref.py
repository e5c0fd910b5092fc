"""CPU restatement of the ciphertext inner product (sealhip_evaluator_dot_product), composed only from
the oracle's functions. BFV (STRICT): steps 1-3 of ref_bfv_multiply (oracle/sealref.c:1185-1265) per term, the tensor
products of all terms summed canonically over the rows of q and Bsk, then ref_bfv_multiply's tail ONCE. CKKS: the oracle
composition itself (ref_ckks_multiply per term, ref_evaluator_add left to right). With keys, ref_relinearize of the sum.
Also the Python-integer form of the bound on the number of terms."""
import ctypes as C

import numpy as np

import oracle_lib as O


def max_terms(n, q, bsk, t):
    """room = bits(prod Bsk) - (bits(t) + log2 N + bits(Q) + 4); max(1, 2^room - 1), saturating at 2^64 - 1"""
    Q = 1
    for p in q:
        Q *= int(p)
    M = 1
    for p in bsk:
        M *= int(p)
    room = M.bit_length() - (int(t).bit_length() + (int(n).bit_length() - 1) + Q.bit_length() + 4)
    if room <= 0:
        return 1, room
    return min(max(1, (1 << room) - 1), (1 << 64) - 1), room


def bsk_primes(n, q, t):
    """the level's base Bsk as the engine and the oracle build it: B from the 60-bit auxiliary primes after m_sk and gamma,
    then m_sk (rns.cpp:568-592)"""
    nb = O.base_b_size([int(p) for p in q], int(t))
    aux = O.aux_primes(n, nb + 2)
    return [int(p) for p in aux[2:2 + nb]] + [int(aux[0])]


def _lift(ref, rt, k, poly):
    """steps 1-3 for one operand polynomial [k][N] (coefficient form) -> (q rows, Bsk rows), lazily transformed"""
    L = O.lib()
    n, B = ref.n, int(rt.contents.Bsk_size)
    strict = 1 if int(ref.c.mode) == 1 else 0
    xq = np.ascontiguousarray(poly, dtype=np.uint64).copy()
    for i in range(k):
        L.ref_ntt_forward_lazy(O.ptr(xq[i]), C.byref(ref.c.key_tables[i]), strict)
    temp = np.zeros((B + 1, n), dtype=np.uint64)
    xb = np.zeros((B, n), dtype=np.uint64)
    src = np.ascontiguousarray(poly, dtype=np.uint64)
    L.ref_fastbconv_m_tilde(rt, O.ptr(src), O.ptr(temp))
    L.ref_sm_mrq(rt, O.ptr(temp), O.ptr(xb))
    for i in range(B):
        L.ref_ntt_forward_lazy(O.ptr(xb[i]), C.byref(rt.contents.Bsk_ntt[i]), strict)
    return xq, xb


def bfv_dot_product(ref, k, a_terms, b_terms, relin_key=None):
    """a_terms[i], b_terms[i]: [2][k][N] coefficient form. Returns [3][k][N], or [2][k][N] with relin_key."""
    L = O.lib()
    rt = ref.rns_tool(k)
    n, B = ref.n, int(rt.contents.Bsk_size)
    dq = np.zeros((3, k, n), dtype=np.uint64)
    dB = np.zeros((3, B, n), dtype=np.uint64)
    prod = np.zeros(n, dtype=np.uint64)
    lifted = {}

    def lift(ct):
        key = id(ct)
        if key not in lifted:
            lifted[key] = [_lift(ref, rt, k, ct[j]) for j in range(2)]
        return lifted[key]

    for a, b in zip(a_terms, b_terms):
        xa, xb = lift(a), lift(b)
        for i1 in range(2):
            for i2 in range(2):
                I = i1 + i2
                for r in range(k):
                    m = C.byref(ref.c.key_mod[r])
                    L.ref_dyadic_product_coeffmod(O.ptr(xa[i1][0][r]), O.ptr(xb[i2][0][r]), n, m, O.ptr(prod))
                    L.ref_add_poly_coeffmod(O.ptr(prod), O.ptr(dq[I, r]), n, m, O.ptr(dq[I, r]))
                for r in range(B):
                    m = C.byref(rt.contents.Bsk[r])
                    L.ref_dyadic_product_coeffmod(O.ptr(xa[i1][1][r]), O.ptr(xb[i2][1][r]), n, m, O.ptr(prod))
                    L.ref_add_poly_coeffmod(O.ptr(prod), O.ptr(dB[I, r]), n, m, O.ptr(dB[I, r]))
    out = np.zeros((3, k, n), dtype=np.uint64)
    tqB = np.zeros((k + B, n), dtype=np.uint64)
    tB = np.zeros((B, n), dtype=np.uint64)
    t = int(ref.c.t)
    for I in range(3):
        for r in range(k):
            L.ref_ntt_inverse(O.ptr(dq[I, r]), C.byref(ref.c.key_tables[r]))
            L.ref_multiply_poly_scalar_coeffmod(O.ptr(dq[I, r]), n, t, C.byref(ref.c.key_mod[r]), O.ptr(tqB[r]))
        for r in range(B):
            L.ref_ntt_inverse(O.ptr(dB[I, r]), C.byref(rt.contents.Bsk_ntt[r]))
            L.ref_multiply_poly_scalar_coeffmod(O.ptr(dB[I, r]), n, t, C.byref(rt.contents.Bsk[r]), O.ptr(tqB[k + r]))
        L.ref_fast_floor(rt, O.ptr(tqB), O.ptr(tB))
        L.ref_fastbconv_sk(rt, O.ptr(tB), O.ptr(out[I]))
    return _relin(ref, k, out, relin_key)


def ckks_dot_product(ref, k, a_terms, b_terms, relin_key=None):
    """the oracle composition: ref_ckks_multiply per term, ref_evaluator_add over the products left to right"""
    L = O.lib()
    n = ref.n
    acc = None
    for a, b in zip(a_terms, b_terms):
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        prod = np.zeros((3, k, n), dtype=np.uint64)
        assert L.ref_ckks_multiply(C.byref(ref.c), k, O.ptr(a), 2, O.ptr(b), 2, O.ptr(prod)) == 0
        if acc is None:
            acc = prod
        else:
            nxt = np.zeros_like(acc)
            L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(acc), 3, O.ptr(prod), 3, O.ptr(nxt))
            acc = nxt
    return _relin(ref, k, acc, relin_key)


def _relin(ref, k, ct3, relin_key):
    if relin_key is None:
        return ct3
    L = O.lib()
    ct3 = np.ascontiguousarray(ct3).copy()
    key = np.ascontiguousarray(relin_key, dtype=np.uint64)
    keys = (C.c_void_p * 1)(key.ctypes.data)
    assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(ct3), 3, keys) == 0
    return np.ascontiguousarray(ct3[:2])


def dot_product(ref, k, a_terms, b_terms, relin_key=None):
    fn = bfv_dot_product if ref.scheme == 1 else ckks_dot_product
    return fn(ref, k, a_terms, b_terms, relin_key)
