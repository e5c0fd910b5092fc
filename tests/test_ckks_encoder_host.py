"""The inputs of tests/test_gpu_ckks_encoder.py are what its cases say they are: checked with the oracle alone, without a
device, so that a failure on the GPU cannot be blamed on a badly chosen input. The builders are imported from the GPU file
(importing it touches no device), and every seed is the one the GPU test uses.

Also checked by reading the constants: the levels hit both ends of every ckks_compose_kernel instance's range, and the ring
sizes hit every tail of run_fft above its LDS tile."""
import numpy as np
import pytest

import oracle_lib as O
import test_gpu_ckks_encoder as G

K_CKKS_MAX_LIMBS = 32  # engine.hpp kCkksMaxLimbs
TILE_LOG = 11          # ckks_encoder.hip kTileLog


class Ref:
    def __init__(self, logn, bits):
        self.n = 1 << logn
        self.mods = list(G.moduli(logn, tuple(bits)))
        self.ref = O.RefContext(G.CKKS, logn, self.mods, nsp=1)
        self.ck = O.CkksRef(self.ref)


@pytest.fixture(scope="module")
def limb():
    return Ref(G.LIMB_LOGN, G.LIMB_BITS)


@pytest.fixture(scope="module")
def edge():
    return Ref(G.EDGE_LOGN, G.EDGE_BITS)


def test_levels_reach_both_ends_of_every_compose_instance():
    """launch_ckks_decode_back: <4> for k <= 4, <8> for k <= 8, <16> for k <= 16, <32> up to kCkksMaxLimbs"""
    ranges, lo = [], 1
    for top in (4, 8, 16, K_CKKS_MAX_LIMBS):
        ranges.append((lo, top))
        lo = top + 1
    for lo, top in ranges:
        assert lo in G.LIMB_LEVELS and top in G.LIMB_LEVELS, (lo, top)
    assert G.OVER_LIMIT == K_CKKS_MAX_LIMBS + 1 and len(G.LIMB_BITS) == G.OVER_LIMIT + 1  # (one special prime on top)
    assert all(p.bit_length() == 30 for p in G.limb_moduli()) and len(set(G.limb_moduli())) == len(G.LIMB_BITS)


def test_ring_sizes_reach_every_fft_tail():
    """run_fft above the tile: pairs of layers, then a single one when their number is odd. The suite elsewhere runs
    log N = 12 (single), 13 (pair), 15 (pair, pair)"""
    def tail(logn):
        rest = logn - TILE_LOG
        return ("pair",) * (rest // 2) + ("single",) * (rest % 2)

    assert {tail(logn) for logn in G.FFT_LOGNS} == {("pair", "single"), ("pair", "pair", "single")}
    assert G.STRIDE_COUNT << (G.STRIDE_LOGN - 2) > G.LAYER2_LANES  # quadruples of one launch: a second loop iteration
    assert (G.STRIDE_COUNT - 1) << (G.STRIDE_LOGN - 2) <= G.LAYER2_LANES  # (and no smaller batch would do)
    v = G.stride_values()
    assert len({v[i].tobytes() for i in range(G.STRIDE_COUNT)}) == G.STRIDE_COUNT


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("k", G.LIMB_LEVELS)
def test_decoded_residues_are_finite(limb, k):
    for i, plain in enumerate(G.limb_residues(k)):
        dec = limb.ck.decode(plain, G.limb_scale(k))
        assert np.all(np.isfinite(dec.real)) and np.all(np.isfinite(dec.imag)), (k, i)


@pytest.mark.parametrize("k", G.LIMB_LEVELS)
def test_decoded_constants(limb, k):
    scale = G.limb_scale(k)
    dec = {name: limb.ck.decode(G.constant_plain(limb.mods, k, limb.n, h), scale) for name, h in G.limb_constants(k)}
    for name, d in dec.items():
        assert np.all(np.isfinite(d.real)) and np.all(np.isfinite(d.imag)), (k, name)
    assert np.all(dec["zero"] == 0.0)
    assert np.all(dec["one"].real == 1.0 / scale) and np.all(dec["one"].imag == 0.0)
    assert np.all(dec["minus one"].real == -1.0 / scale) and np.all(dec["minus one"].imag == 0.0)
    # the threshold (Q + 1) >> 1 is the first value read as negative (h - Q); just below it h is read as it is
    assert np.all(dec["threshold"].real < 0) and np.all(dec["below threshold"].real > 0)


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("k", G.LIMB_LEVELS + (G.OVER_LIMIT,))
def test_wide_values_are_accepted(limb, k):
    v, scale = G.wide_values(k), G.limb_scale(k)
    assert np.any(v.real > 0) and np.any(v.real < 0) and np.any(v.imag > 0) and np.any(v.imag < 0)
    for i in range(G.LIMB_COUNT):
        rc, words = limb.ck.encode(v[i], k, scale)
        assert rc == 0, (k, i, rc)
        if k <= K_CKKS_MAX_LIMBS:
            dec = limb.ck.decode(words, scale)
            assert np.all(np.isfinite(dec.real)) and np.all(np.isfinite(dec.imag)), (k, i)


def largest_coefficient_log2(k):
    """log2 of the largest coefficient magnitude the first vector of wide_values(k) encodes to, from the definition: the
    coefficients are (scale / N) sum_j 2 Re(z_j zeta_j^-i), zeta_j = exp(2 pi i 5^j / 2N). In doubles on the values scaled
    down to a + bi, which is exact; good to far more than the whole bits the assertions below leave as margin."""
    n, scale = 1 << G.LIMB_LOGN, G.limb_scale(k)
    e = G.product(G.limb_moduli(), k).bit_length() - int(np.log2(scale)) - G.WIDE_SLACK
    z = np.ldexp(G.wide_values(k)[0].real, -e) + 1j * np.ldexp(G.wide_values(k)[0].imag, -e)
    g = np.array([pow(5, j, 2 * n) for j in range(n // 2)], dtype=np.int64)
    angles = -2.0 * np.pi * ((g[None, :] * np.arange(n, dtype=np.int64)[:, None]) % (2 * n)) / (2 * n)
    coeff = 2.0 * np.real(np.exp(1j * angles) @ z) / n
    return float(np.log2(np.max(np.abs(coeff)))) + e + np.log2(scale)


def test_wide_values_cross_the_three_regimes_and_reach_limb_13_and_14():
    """the reference decomposes by the largest bit count int(log2) + 2: at most 64 (ckks.h:515-540), at most 128 (:541-568),
    beyond (:569-607); the device's limb index is (e - 52) >> 6 for a coefficient in [2^e, 2^(e+1)), e >= 53"""
    log2s = {k: largest_coefficient_log2(k) for k in G.LIMB_LEVELS + (G.OVER_LIMIT,)}
    frac = {k: v - np.floor(v) for k, v in log2s.items()}
    assert all(0.01 < f < 0.99 for f in frac.values()), frac  # (no value so close to a power of two that rounding decides)
    bits = {k: int(np.floor(v)) + 2 for k, v in log2s.items()}
    assert bits[1] <= 64 < bits[4] <= 128 < bits[5], bits
    # the largest coefficient at k = 32 lies in [2^946, 2^947): limb 13, two bits short of 14, which the vectors of k = 33
    # (encode only) reach
    assert (bits[32] - 2 - 52) >> 6 == 13 and (bits[G.OVER_LIMIT] - 2 - 52) >> 6 == 14, bits
    total = {k: G.product(G.limb_moduli(), k).bit_length() for k in bits}
    assert all(total[k] - 16 <= bits[k] < total[k] for k in bits), (bits, total)  # most of the modulus, and accepted


def test_small_values_above_the_limit_are_accepted(limb):
    rc, _ = limb.ck.encode(G.small_values(G.OVER_LIMIT)[0], G.OVER_LIMIT, G.LIMB_SCALE)
    assert rc == 0


# ---------------------------------------------------------------- C
def test_edge_setting(edge):
    assert G.product(edge.mods, G.EDGE_K).bit_length() == 80
    wide = Ref(G.EDGE_LOGN, G.REGIME_BITS)
    assert G.product(wide.mods, G.REGIME_K).bit_length() == 120
    assert G.REFUSED[0] == 2.0 ** 48 and G.ACCEPTED[0] == 2.0 ** 47
    for series, top in ((G.REFUSED, 2.0 ** 48), (G.ACCEPTED, 2.0 ** 47)):
        assert len(series) == 6 and all(a > b for a, b in zip(series, series[1:])) and series[-1] == top - 5 * np.spacing(top / 2)


@pytest.mark.parametrize("ulps", range(6))
def test_oracle_refuses_2_pow_48_and_the_doubles_below(edge, ulps):
    c = G.REFUSED[ulps]
    rc, _ = edge.ck.encode(G.constant_slots(G.EDGE_LOGN, c)[0], G.EDGE_K, G.EDGE_SCALE)
    assert rc == -2, (c.hex(), rc)
    # the planted coefficient is exactly c * scale: one level up, where it is accepted, the oracle returns c in every slot
    rc, words = edge.ck.encode(G.constant_slots(G.EDGE_LOGN, c)[0], 3, G.EDGE_SCALE)
    assert rc == 0
    dec = edge.ck.decode(words, G.EDGE_SCALE)
    assert np.all(dec.real == c) and np.all(dec.imag == 0.0), c.hex()


@pytest.mark.parametrize("ulps", range(6))
def test_oracle_accepts_2_pow_47_and_the_doubles_below(edge, ulps):
    c = G.ACCEPTED[ulps]
    rc, words = edge.ck.encode(G.constant_slots(G.EDGE_LOGN, c)[0], G.EDGE_K, G.EDGE_SCALE)
    assert rc == 0, (c.hex(), rc)
    dec = edge.ck.decode(words, G.EDGE_SCALE)
    assert np.all(dec.real == c) and np.all(dec.imag == 0.0), c.hex()


def test_edge_batch_is_refused_for_its_last_item_only(edge):
    rc = [edge.ck.encode(v, G.EDGE_K, G.EDGE_SCALE)[0] for v in G.edge_batch()]
    assert rc == [0, 0, -2]


def test_regime_boundaries_are_accepted():
    wide = Ref(G.EDGE_LOGN, G.REGIME_BITS)
    assert [c * G.EDGE_SCALE for c in G.REGIME] == [2.0 ** 62, G.below(2.0 ** 62, 1), 2.0 ** 63, G.below(2.0 ** 63, 1)]
    for c in G.REGIME:
        rc, words = wide.ck.encode(G.constant_slots(G.EDGE_LOGN, c)[0], G.REGIME_K, G.EDGE_SCALE)
        assert rc == 0, c.hex()
        dec = wide.ck.decode(words, G.EDGE_SCALE)
        assert np.all(dec.real == c) and np.all(dec.imag == 0.0), c.hex()


def test_ties_round_away_from_zero_and_minus_zero_is_zero(edge):
    for x, rounded in G.TIES:
        rc, words = edge.ck.encode(G.constant_slots(G.EDGE_LOGN, x / G.TIE_SCALE)[0], G.EDGE_K, G.TIE_SCALE)
        assert rc == 0, x
        for r in range(G.EDGE_K):  # the NTT form of the constant `rounded`
            assert np.all(words[r] == rounded % edge.mods[r]), (x, r)
    assert [rounded for _, rounded in G.TIES] == [1, -1, 3, -3, 0]


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("logn", G.FFT_LOGNS)
def test_fft_inputs_are_accepted(logn):
    r = Ref(logn, G.FFT_BITS)
    v = G.fft_values(logn)
    for i in range(G.FFT_COUNT):
        assert r.ck.encode(v[i], G.FFT_K, G.FFT_SCALE)[0] == 0
        assert r.ck.encode(v[i, : r.n // 8], G.FFT_K, G.FFT_SCALE)[0] == 0
    for plain in G.fft_residues(logn):
        dec = r.ck.decode(plain, G.FFT_SCALE)
        assert np.all(np.isfinite(dec.real)) and np.all(np.isfinite(dec.imag))


def test_stride_inputs_are_accepted():
    r = Ref(G.STRIDE_LOGN, G.FFT_BITS)
    v = G.stride_values()
    assert all(r.ck.encode(v[i], G.STRIDE_K, G.STRIDE_SCALE)[0] == 0 for i in range(G.STRIDE_COUNT))
