"""The library's fixed-weight rule restated in numpy over tests/sample_ref.py's stream words:
  w_i, i < N = stream words [0, N) of BlakePRNG(seed);
  rank_i = #{ j : w_j < w_i, or w_j == w_i and j < i } -- the position of i in a STABLE sort of the words;
  coefficient i = 0 when rank_i >= h, else -1 when w_i & 1, else +1.
Also what the tests of sparse-secret encapsulation share: an oracle client around a given secret, and the decryption of a
CKKS ciphertext to centred integers."""
import ctypes as C

import numpy as np

import oracle_lib as O
import sample_ref as R


def fixed_weight_map(words, h):
    """int32 of words' shape [..., N]: the rule along the last axis"""
    words = np.asarray(words, dtype=np.uint64)
    order = np.argsort(words, axis=-1, kind="stable")
    support = order[..., :h]
    signs = np.where((np.take_along_axis(words, support, axis=-1) & np.uint64(1)).astype(bool), -1, 1).astype(np.int32)
    out = np.zeros(words.shape, dtype=np.int32)
    np.put_along_axis(out, support, signs, axis=-1)
    return out


def sample_fixed_weight(S, seeds, n, h):
    """int32 [count][n]"""
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1, 8)
    return fixed_weight_map(np.stack([R.stream_words(S, s, n) for s in seeds]), h)


class SecretClient(O.Client):
    """oracle_lib.Client around a given small secret s (int values in {-1, 0, 1}, N of them)"""

    def __init__(self, ref, s, seed):
        super().__init__(ref, seed=seed)
        self.s = np.ascontiguousarray(s, dtype=np.int8)
        self.sk = np.zeros((self.n_key, self.n), dtype=np.uint64)
        O.lib().ref_small_poly_to_rns(C.byref(ref.c), self.s.ctypes.data, self.n_key, 1, O.ptr(self.sk))


def lifted(s, mods):
    """KeyGenerator::generate_sk's lift: row j is s modulo mods[j] (-1 -> q_j - 1), coefficient form"""
    s = np.asarray(s, dtype=np.int64)
    return np.stack([np.where(s < 0, int(q) + s, s).astype(np.uint64) for q in mods])


def decrypt_centred(cl, ct):
    """ct (2, k, N) in NTT form under cl's secret -> (centred integer coefficients of c_0 + c_1 s modulo q_0 .. q_(k-1), q)"""
    L, c = O.lib(), cl.ref.c
    k = ct.shape[1]
    dot = np.ascontiguousarray(ct[0]).copy()
    for r in range(k):
        t = np.zeros(cl.n, dtype=np.uint64)
        L.ref_dyadic_product_coeffmod(O.ptr(np.ascontiguousarray(ct[1, r])), O.ptr(cl.sk[r]), cl.n, C.byref(c.key_mod[r]), O.ptr(t))
        L.ref_add_poly_coeffmod(O.ptr(dot[r]), O.ptr(t), cl.n, C.byref(c.key_mod[r]), O.ptr(dot[r]))
    return cl.centered_from_ntt_rows(dot)


def switch_secret(ref, ct, key):
    """(c_0, 0) + switch_key(c_1) of ct (2, k, N) through the oracle's ref_switch_key_inplace"""
    k = ct.shape[1]
    out = np.ascontiguousarray(ct).copy()
    out[1] = 0
    target = np.ascontiguousarray(ct[1]).copy()
    assert O.lib().ref_switch_key_inplace(C.byref(ref.c), k, O.ptr(out), O.ptr(target), O.ptr(np.ascontiguousarray(key))) == 0
    return out
