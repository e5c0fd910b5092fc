"""Planted inputs and an exact reference for the encrypt-side kernels (rlwe.hip, encrypt.hip, scaling_variant_fix in
engine.hpp): the words at which a rounding, a wrap or a zero decides the result, the keys that make a product polynomial
equal a chosen target word for word, and what the kernels must return on them, in Python integers. The oracle is used for its
transforms only (ref_ntt_forward with a RefContext's tables); the library under test is not imported.
tests/test_encrypt_edges_host.py pins every function here to the oracle."""
import ctypes as C
import functools
from math import gcd

import numpy as np

import oracle_lib as O

M64 = (1 << 64) - 1
PLAIN_MODULI = [2, 257, 65537, 786433, 1 << 20, (1 << 60) - 93]
# name: (bits of the key primes, special primes) -- rows smaller and larger than the prime divided out at the first level;
# one prime class; 60-bit primes, where the oracle builds no RNSTool
CHAINS = {"mixed": ([30, 40, 50, 45, 55], 2), "55": ([55, 55, 55, 55], 1), "60": ([60, 60, 60], 1)}


def chains_for(t):
    """the chains a plain modulus is used with: the 60-bit one goes with the 60-bit primes"""
    return ["60"] if t >= 1 << 59 else ["mixed", "55"]


SAMPLE_BOUND = 19  # the noise sampler's range is [-19, 19]


def product(mods):
    q = 1
    for p in mods:
        q *= int(p)
    return q


def unique(values):
    out = []
    for v in values:
        if v not in out:
            out.append(v)
    return out


# ---------------------------------------------------------------- the scaling variant (scalingvariant.cpp:31-51)
def planted_plain_words(mods_k, t):
    """the words m < t whose numerator m (q mod t) + (t + 1) // 2 leaves 0, 1, t - 2, t - 1 modulo t (an exact multiple of t is
    where the Barrett estimate of the quotient falls one short), then the ends and the middle of the range"""
    t = int(t)
    qt, thr = product(mods_k) % t, (t + 1) // 2
    assert gcd(qt, t) == 1, (qt, t)
    inv = pow(qt, -1, t) if t > 1 else 0
    words = [(r - thr) * inv % t for r in (0, 1, t - 2, t - 1)]
    words += [0, 1, t - 1, t // 2, (t + 1) // 2, (t + 1) // 2 - 1]
    return unique([w % t for w in words])


def barrett_quotient_estimate(num, t):
    """the quotient barrett_reduce_128 (uintarithsmallmod.h:140-178) forms for num < 2^128 before its one correction: the
    words of scaling_variant_fix up to `fix += rem >= t`, limb by limb. Equals floor(num floor(2^128 / t) / 2^128)."""
    num, t = int(num), int(t)
    ratio = (1 << 128) // t
    cr0, cr1 = ratio & M64, ratio >> 64
    lo, hi = num & M64, num >> 64
    carry0 = (lo * cr0) >> 64
    t1 = lo * cr1
    tmp1 = (t1 & M64) + carry0
    tmp3 = ((t1 >> 64) + (tmp1 >> 64)) & M64
    tmp1 &= M64
    u = hi * cr0
    tmp1b = tmp1 + (u & M64)
    carry1 = ((u >> 64) + (tmp1b >> 64)) & M64
    return (hi * cr1 + tmp3 + carry1) & M64


def numerator(m, mods_k, t):
    return int(m) * (product(mods_k) % int(t)) + (int(t) + 1) // 2


def ref_delta_m(m, mods_k, t):
    """Delta m = round(q m / t) row by row: floor(q / t) m + floor((m (q mod t) + (t + 1) // 2) / t) modulo each q_i"""
    m, t, q = int(m), int(t), product(mods_k)
    v = q // t * m + (m * (q % t) + (t + 1) // 2) // t
    return [v % int(p) for p in mods_k]


# ---------------------------------------------------------------- divide_and_round_q_last_inplace (rns.cpp:731-775)
@functools.lru_cache(maxsize=None)
def _inverse(v, p):
    return pow(v, -1, p)


def divround_rows(x_rows, mods_R, trace=None):
    """one coefficient's R residues -> the R - 1 residues of round(x / q_last). trace (a dict) receives what happened on the
    way: 'wrapped' (x + half reached q_last), and per row 'borrow' (the subtraction went below zero) and 'zero' (it gave 0)."""
    mods = [int(p) for p in mods_R]
    ql = mods[-1]
    half = ql >> 1
    s = int(x_rows[-1]) + half
    wrapped = s >= ql
    last = s - ql if wrapped else s
    out, borrow, zero = [], [], []
    for xv, qi in zip(x_rows[:-1], mods[:-1]):
        temp = (last % qi - half % qi) % qi
        xv = int(xv)
        borrow.append(xv < temp)
        zero.append(xv == temp)
        out.append((xv - temp) % qi * _inverse(ql, qi) % qi)
    if trace is not None:
        trace.update(wrapped=wrapped, last=last, borrow=borrow, zero=zero)
    return out


def row_temp(x_last, mods_R, r):
    """what row r subtracts when the last row holds x_last: (last mod q_r) - (half mod q_r) modulo q_r"""
    ql, qr = int(mods_R[-1]), int(mods_R[r])
    half = ql >> 1
    return ((int(x_last) + half) % ql % qr - half % qr) % qr


def divround_restated(x, mods, R, ntt, c):
    """divide_and_round_q_last_inplace (rns.cpp:731-775) / _ntt_inplace (:777-851) of one R-row polynomial in place,
    restated line by line from oracle/sealref.c with Python integers and the oracle's transforms (c: the RefContext's
    struct). Returns the last row's coefficients before half is added."""
    L = O.lib()
    n = x.shape[-1]
    q = [int(p) for p in mods[:R]]
    ql = q[R - 1]
    half = ql >> 1
    last_row = x[R - 1].copy()
    if ntt:
        L.ref_ntt_inverse(O.ptr(last_row), C.byref(c.key_tables[R - 1]))
    coeffs = [int(v) for v in last_row]
    if not ntt:
        cols = [divround_rows([int(x[r, i]) for r in range(R)], q) for i in range(n)]
        for i in range(R - 1):
            x[i] = np.array([col[i] for col in cols], dtype=np.uint64)
        return coeffs
    last = [(v + half) % ql for v in coeffs]
    for i in range(R - 1):
        qi = q[i]
        inv = pow(ql, -1, qi)
        temp = np.array([(lv % qi if qi < ql else lv) + qi - half % qi for lv in last], dtype=np.uint64)
        L.ref_ntt_forward_lazy(O.ptr(temp), C.byref(c.key_tables[i]), 0)
        out = [((int(xv) + 4 * qi - int(tv)) % (1 << 64)) * inv % qi for xv, tv in zip(x[i], temp)]
        x[i] = np.array(out, dtype=np.uint64)
    return coeffs


def planted_last_row(q_last):
    """the last-row sums either side of where x + half wraps q_last, and the ends of the range"""
    q_last = int(q_last)
    half = q_last >> 1
    return unique([0, 1, half - 1, half, half + 1, q_last - half - 1, q_last - half, q_last - half + 1, q_last - 1])


ROW_KINDS = 5


def planted_row(q_r, temp_r):
    """the residues either side of the value row r subtracts (the difference is -1, 0, +1), and the ends of the range"""
    q_r, temp_r = int(q_r), int(temp_r)
    return [(temp_r - 1) % q_r, temp_r % q_r, (temp_r + 1) % q_r, 0, q_r - 1]


# ---------------------------------------------------------------- sums with a small sample
def planted_sample_pairs(p):
    """(c, e): c + lift(e) wraps p, stops one short of it, or is exactly 0; e within the sampler's range"""
    p, b = int(p), SAMPLE_BOUND
    return unique([(p - 1, 1), (0, -1), (p - b, b), (b - 1, -b), (b, -b), (p - b, b), (0, 0), (p - 1, 0)])


SAMPLE_VALUES = (1, -1, SAMPLE_BOUND, -SAMPLE_BOUND, 0)


def lift(e, p):
    """a small signed sample as a residue (sample_poly_normal's representation, util/rlwe.cpp:25-95)"""
    e, p = int(e), int(p)
    return e if e >= 0 else p + e


def add_small(c, e, p):
    return (int(c) + int(e)) % int(p)


# ---------------------------------------------------------------- where the planted words go
def planted_positions(n, rng):
    """coefficients 0 and 1 (the two lanes of a coefficient pair), n - 2 and n - 1, and one random index between them"""
    return [0, 1, n - 2, n - 1, int(rng.integers(2, n - 2))]


def planted_slots(n, rng, items, polys=1):
    """(item, polynomial, coefficient) for the first and the last item of a batch (`items`), every polynomial"""
    pos = planted_positions(n, rng)
    return [(i, j, c) for i in items for j in range(polys) for c in pos]


def random_rows(rng, mods, n, lead=()):
    """canonical residues [lead..][len(mods)][n] as Python integers in an object array"""
    out = np.empty(tuple(lead) + (len(mods), n), dtype=object)
    for r, p in enumerate(mods):
        draw = rng.integers(0, int(p), size=tuple(lead) + (n,), dtype=np.uint64)
        out[..., r, :] = draw.astype(object)
    return out


def to_u64(a):
    return np.ascontiguousarray(np.array(a, dtype=object).astype(np.uint64))


# ---------------------------------------------------------------- keys whose product is a chosen polynomial
@functools.lru_cache(maxsize=None)
def _math_ntt(logn, p):
    return O.MathNtt(logn, p)


def ntt_row_raw(ref, row, r):
    """one row through ref_ntt_forward with the table of key prime r, as the oracle has it"""
    out = to_u64(row)
    O.lib().ref_ntt_forward(O.ptr(out), C.byref(ref.c.key_tables[r]), 0)
    return out


def round_trips(ref, row, r):
    """ref_ntt_inverse(ref_ntt_forward(row)) is row: the forward transform's uncorrected butterflies did not wrap 2^64 (they
    can on 60-bit primes from 2^11 on, depending on the words)"""
    row = to_u64(row)
    back = ntt_row_raw(ref, row, r)
    O.lib().ref_ntt_inverse(O.ptr(back), C.byref(ref.c.key_tables[r]))
    return np.array_equal(back, row)


def ntt_row(ref, row, r):
    """the transform of one row, exactly: ref_ntt_forward where it round-trips, else the transform from its definition
    (oracle_lib.MathNtt), which the oracle's inverse then takes back to the row"""
    row = to_u64(row)
    if round_trips(ref, row, r):
        return ntt_row_raw(ref, row, r)
    out = to_u64(_math_ntt(ref.logn, ref.key_moduli[r]).forward(row))
    back = out.copy()
    O.lib().ref_ntt_inverse(O.ptr(back), C.byref(ref.c.key_tables[r]))
    assert np.array_equal(back, row)
    return out


def ntt_rows(ref, x, exact=True):
    """rows r of x[..][rows][N] transformed with key prime r (exact: ntt_row, else ntt_row_raw)"""
    out = to_u64(x)
    flat = out.reshape(-1, out.shape[-2], out.shape[-1])
    for poly in flat:
        for r in range(poly.shape[0]):
            poly[r] = ntt_row(ref, poly[r], r) if exact else ntt_row_raw(ref, poly[r], r)
    return out


def delta_u(n, sign=1):
    """u = +-(1, 0, .., 0): its transform is +-1 in every word, so u (.) pk_j = +-pk_j"""
    u = np.zeros(n, dtype=np.int32)
    u[0] = sign
    return u


def pk_for_targets(ref, target):
    """pk[j][r] = NTT_r(target[j][r]): with u = (1, 0, .., 0), INTT(u (.) pk_j) is target[j] word for word"""
    return ntt_rows(ref, target)


def ones_key(mods, n):
    """the transform of the secret key s = 1"""
    return np.ones((len(mods), n), dtype=np.uint64)


def sk_for_targets(ref, target, a, mods, target_is_ntt=False):
    """sk[r] = NTT_r(target[r]) a[r]^{-1} word by word: a (.) sk is the transform of target. a: the words the kernel
    multiplies by (NTT form); none of them may be zero."""
    a = np.asarray(a)
    assert all(int(v) != 0 for v in a.reshape(-1)), "a has a zero word: pick another seed"
    want = to_u64(target) if target_is_ntt else ntt_rows(ref, target)
    out = np.empty(want.shape, dtype=np.uint64)
    for r, p in enumerate(mods[:want.shape[0]]):
        p = int(p)
        out[r] = np.array([int(w) * pow(int(v), -1, p) % p for w, v in zip(want[r], a[r])], dtype=np.uint64)
    return out


def seeded_a(ref, seed, mods, n, transform):
    """the words encrypt_symmetric multiplies the secret key by: the oracle's expand_seed of the seed (the sample itself),
    or its forward transform in the seeded BFV branch (rlwe.cpp:233-243)"""
    sample = np.ascontiguousarray(O.expand_seed(seed, mods, n))
    return sample, (ntt_rows(ref, sample, exact=False) if transform else sample)  # (the branch's transform, wrapped or not)


def pick_seed(rng, mods, n, ref=None, transform=False):
    """a seed whose expansion (and transform, when asked) has no zero word"""
    for _ in range(16):
        seed = rng.integers(0, 2**64, size=8, dtype=np.uint64, endpoint=False)
        sample, a = seeded_a(ref, seed, mods, n, transform)
        if sample.all() and a.all():
            return seed
    raise AssertionError("no seed without a zero word")
