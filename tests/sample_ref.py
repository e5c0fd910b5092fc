"""The library's RLWE sampling rule restated in numpy over sealhip.blake2xb:
  stream word m of a 64-byte seed = the little-endian 64-bit word at byte 8m of BlakePRNG(seed), where buffer c of the PRNG
    is BLAKE2Xb(4096 bytes, in = c as 8 little-endian bytes, key = seed);
  an item draws n_ternary ternary polynomials, then n_noise noise polynomials; coefficient i of polynomial p comes from
    word pN + i alone;
  ternary: floor(3 w / 2^64) - 1;  noise: r = w >> 1, magnitude = #{m : r >= T_m}, negative when w & 1.
The thresholds come from tests/golden/noise_cdt.json, not from the library."""
import json
import math
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_cdt.json")
SIGMA, MAX_DEV = 3.2, 19.2  # globals.h: noise_standard_deviation, 6 x it


def thresholds():
    with open(GOLDEN) as f:
        return [int(x, 16) for x in json.load(f)["thresholds"]]


def tail(m):
    """P(|X| >= m + 1) for X ~ N(0, 3.2^2) conditioned on |X| <= 19.2"""
    s2 = math.sqrt(2.0)
    return (math.erfc((m + 1) / (SIGMA * s2)) - math.erfc(MAX_DEV / SIGMA / s2)) / math.erf(MAX_DEV / SIGMA / s2)


def magnitude_probabilities(T=None):
    """P(magnitude = 0 .. 19) of the table"""
    T = thresholds() if T is None else T
    edges = [0] + list(T) + [1 << 63]
    return [(edges[i + 1] - edges[i]) / float(1 << 63) for i in range(20)]


def stream_words(S, seed_words, count):
    """words 0 .. count-1 of the stream of one seed"""
    key = struct.pack("<8Q", *[int(x) for x in seed_words])
    bufs = [np.frombuffer(S.blake2xb(4096, struct.pack("<Q", c), key), dtype="<u8") for c in range((count + 511) // 512)]
    return np.concatenate(bufs).astype(np.uint64)[:count]


def ternary_map(w):
    w = np.asarray(w, dtype=np.uint64)
    one, two = np.uint64(-((-1 << 64) // 3)), np.uint64(-((-2 << 64) // 3))  # ceil(2^64 / 3), ceil(2^65 / 3)
    return (w >= one).astype(np.int32) + (w >= two).astype(np.int32) - 1


def noise_map(w, T=None):
    w = np.asarray(w, dtype=np.uint64)
    T = np.array(thresholds() if T is None else T, dtype=np.uint64)
    mag = np.searchsorted(T, w >> np.uint64(1), side="right").astype(np.int32)  # thresholds at or below r
    return np.where((w & np.uint64(1)).astype(bool), -mag, mag).astype(np.int32)


def map_item(words, n, n_ternary, n_noise, T=None):
    """the (n_ternary + n_noise) x n samples of an item from its first (n_ternary + n_noise) n stream words"""
    words = np.asarray(words, dtype=np.uint64)[: (n_ternary + n_noise) * n]
    out = np.empty(words.size, dtype=np.int32)
    out[: n_ternary * n] = ternary_map(words[: n_ternary * n])
    out[n_ternary * n :] = noise_map(words[n_ternary * n :], T)
    return out.reshape(n_ternary + n_noise, n)


def sample_polys(S, seeds, n, n_ternary, n_noise):
    """int32 [count][n_ternary + n_noise][n]"""
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1, 8)
    T = thresholds()
    return np.stack([map_item(stream_words(S, s, (n_ternary + n_noise) * n), n, n_ternary, n_noise, T) for s in seeds])


def chi2_bound(cells, p=1e-6):
    """the 1 - p quantile of chi-square with cells - 1 degrees of freedom"""
    df = cells - 1
    try:
        from scipy.stats import chi2

        return float(chi2.ppf(1 - p, df))
    except ImportError:
        pass
    if df == 2:
        return -2.0 * math.log(p)  # exact: chi-square with 2 degrees of freedom is exponential with mean 2
    from statistics import NormalDist

    z = NormalDist().inv_cdf(1 - p)
    return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3  # Wilson-Hilferty


def noise_chi2(counts_by_value, total):
    """chi-square of a histogram {signed value: count} against the table: every signed value with an expected count of at
    least 5 has its own cell, the rest are pooled. Returns (statistic, cells)."""
    P = magnitude_probabilities()
    stat, cells, pooled_obs, pooled_exp = 0.0, 0, 0.0, 0.0
    for v in range(-19, 20):
        exp = total * (P[0] if v == 0 else P[abs(v)] / 2)
        obs = counts_by_value.get(v, 0)
        if exp >= 5:
            stat += (obs - exp) ** 2 / exp
            cells += 1
        else:
            pooled_obs += obs
            pooled_exp += exp
    stat += (pooled_obs - pooled_exp) ** 2 / pooled_exp
    return stat, cells + 1
