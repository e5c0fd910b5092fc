"""The CKKS encoder (csrc/ckks_encoder.hip) at every kernel instance and at the edges of its size check, against the CPU oracle.

Every comparison is with oracle_lib.CkksRef and is exact: plaintext words with np.array_equal, decoded doubles by their uint64
views. No tolerance is involved anywhere. The inputs are built by the functions of this module, which need no device;
tests/test_ckks_encoder_host.py imports them and asserts, with the oracle alone, the preconditions each case relies on (the
oracle accepts what is to be accepted and refuses what is to be refused, its doubles are finite, the planted coefficients are
what the case says they are).

The sections:
  A  ckks_compose_kernel<4 | 8 | 16 | 32>: N = 2^10, 34 primes of 30 bits, decode at k in {1, 4, 5, 8, 9, 16, 17, 32} -- both
     ends of every instance's range of k -- of random canonical residues and of the constant polynomials 0, 1, Q - 1 and the
     two sides of the upper-half threshold (Q + 1) >> 1, at scale 2^40 (2^20 at k = 1, where the reference refuses 2^40 as
     out of bounds, and so must the device). Decode at k = 33 is refused (32 limbs at most); encode at k = 33 is not.
  B  the multi-limb branch of ckks_round_decompose_kernel: the same context, levels and scales, values (a + bi) 2^e with
     e = T_k - 3 - log2(scale) - 22 - 5 and T_k the bit count of the first k primes' product, so that the coefficients take
     most of the modulus (the largest has limb index e2 >> 6 = 13 at k = 32 and 14 at k = 33) and cross the reference's
     three decomposition regimes (at most 64 bits, at most 128, beyond).
  C  the "encoded values are too large" check where static_cast<int>(log2(d)) and the exponent of d differ (d one to five
     ulps below a power of two), on the largest coefficient of a whole batch; the reference's regime boundaries; ties and
     negative zero.
  D  run_fft's tails above the LDS tile: log N = 14 (a two-layer launch and a single one) and 16 (two, two, one), and one batch
     of 129 plaintexts at log N = 16, whose 129 * 2^14 quadruples take fft_layer2_kernel's grid-stride loop (8192 workgroups
     of 256 lanes) into a second iteration; the chunk log shows that the batch went through in one chunk."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from support import S as sealhip

pytestmark = pytest.mark.gpu

CKKS = 2

# ---- A and B: every compose instance, every decomposition regime
LIMB_LOGN, LIMB_BITS = 10, [30] * 34
LIMB_LEVELS = (1, 4, 5, 8, 9, 16, 17, 32)  # <4>: 1..4, <8>: 5..8, <16>: 9..16, <32>: 17..32
LIMB_SCALE, LIMB_COUNT = 2.0 ** 40, 3
# One prime of 30 bits admits no scale of 2^40: encode wants int(log2(scale)) + 1 < 30 and decode int(log2(scale)) < 30
# (ckks.h:440-444, :651-656), in the reference as here -- both sides must refuse it, which is asserted. Level 1 is the lower
# end of ckks_compose_kernel<4>'s range and stays in the list, at 2^20.
SINGLE_PRIME_SCALE = 2.0 ** 20
OVER_LIMIT = 33  # kCkksMaxLimbs + 1
# (a + bi) 2^(T_k - 3 - log2(scale) - 22 - 5): 3 bits below the modulus, the scale, |a|, |b| < 2^20, and 5 to spare
WIDE_SLACK = 3 + 22 + 5

# ---- C: the size check
EDGE_LOGN, EDGE_BITS, EDGE_K, EDGE_SCALE = 10, [40] * 3, 2, 2.0 ** 30
REGIME_BITS, REGIME_K = [40] * 4, 3
TIE_SCALE = 2.0 ** 16
TIES = ((0.5, 1), (-0.5, -1), (2.5, 3), (-2.5, -3), (-0.3, 0))  # x and the integer it rounds to (away from zero; -0.3 to -0.0)

# ---- D: FFT launch shapes
FFT_LOGNS, FFT_BITS, FFT_K, FFT_COUNT, FFT_SCALE = (14, 16), [50] * 3, 2, 2, 2.0 ** 40
STRIDE_LOGN, STRIDE_K, STRIDE_COUNT, STRIDE_SCALE = 16, 1, 129, 2.0 ** 16
LAYER2_LANES = 8192 * 256  # kMaxBlocks * kThreads: one iteration of the two-layer kernel's grid-stride loop


@functools.lru_cache(maxsize=None)
def moduli(logn, bits):
    return tuple(O.coeff_modulus_create(1 << logn, list(bits)))


def limb_moduli():
    return moduli(LIMB_LOGN, tuple(LIMB_BITS))


def limb_scale(k):
    return SINGLE_PRIME_SCALE if k == 1 else LIMB_SCALE


def product(mods, k):
    q = 1
    for p in mods[:k]:
        q *= int(p)
    return q


def below(x, ulps):
    """the double `ulps` steps below the positive double x"""
    for _ in range(ulps):
        x = np.nextafter(x, 0.0)
    return float(x)


def random_residues(rng, mods, count, n):
    out = np.empty((count, len(mods), n), dtype=np.uint64)
    for r, p in enumerate(mods):
        out[:, r, :] = rng.integers(0, int(p), size=(count, n), dtype=np.uint64)
    return out


def limb_residues(k):
    """section A: LIMB_COUNT plaintexts of uniformly random canonical residues at level k"""
    return random_residues(np.random.default_rng(1000 + k), limb_moduli()[:k], LIMB_COUNT, 1 << LIMB_LOGN)


def constant_plain(mods, k, n, h):
    """the NTT form of the constant polynomial h: row r filled with h mod p_r"""
    out = np.empty((k, n), dtype=np.uint64)
    for r in range(k):
        out[r, :] = int(h) % int(mods[r])
    return out


def limb_constants(k):
    """section A: [(name, h)] with Q the product of the first k primes, a Python integer"""
    q = product(limb_moduli(), k)
    half = (q + 1) >> 1
    return [("zero", 0), ("one", 1), ("minus one", q - 1), ("threshold", half), ("below threshold", half - 1)]


def wide_values(k):
    """section B: LIMB_COUNT vectors of (a + bi) 2^(T_k - log2(scale) - WIDE_SLACK), a and b random integers in +-2^20"""
    rng = np.random.default_rng(2000 + k)
    shape = (LIMB_COUNT, (1 << LIMB_LOGN) // 2)
    a, b = (rng.integers(-(1 << 20), 1 << 20, size=shape).astype(np.float64) for _ in range(2))
    e = product(limb_moduli(), k).bit_length() - int(np.log2(limb_scale(k))) - WIDE_SLACK
    return np.ldexp(a, e) + 1j * np.ldexp(b, e)


def small_values(k):
    """one vector of small integers for the level above the decoder's limit"""
    rng = np.random.default_rng(3000 + k)
    m = (1 << LIMB_LOGN) // 2
    return (rng.integers(-(1 << 20), 1 << 20, size=(1, m)) + 1j * rng.integers(-(1 << 20), 1 << 20, size=(1, m))).astype(np.complex128)


def constant_slots(logn, c, count=1):
    """every slot the real c: the polynomial is the constant c * scale, exactly (sums of equal doubles, products with powers of two)"""
    return np.full((count, (1 << logn) // 2), c, dtype=np.complex128)


REFUSED = [2.0 ** 48] + [below(2.0 ** 48, u) for u in range(1, 6)]   # c * 2^30 at 2^78 and 1..5 ulps below: 80 bits of 80
ACCEPTED = [2.0 ** 47] + [below(2.0 ** 47, u) for u in range(1, 6)]  # 79 bits
# c * 2^30 on both sides of 2^62 (the case the bit count of which an exponent gets wrong inside the first regime) and of 2^63
# (the first coefficient of the 128-bit regime, 65 bits, and the double below it, which log2 also rounds up to 65 bits)
REGIME = [2.0 ** 32, below(2.0 ** 32, 1), 2.0 ** 33, below(2.0 ** 33, 1)]


def edge_batch():
    """three items, the largest coefficient of the batch in the last one"""
    v = constant_slots(EDGE_LOGN, 1.0, 3)
    v[2, :] = below(2.0 ** 48, 1)
    return v


def fft_values(logn):
    rng = np.random.default_rng(4000 + logn)
    shape = (FFT_COUNT, (1 << logn) // 2)
    return (rng.integers(-(1 << 30), 1 << 30, size=shape) + 1j * rng.integers(-(1 << 30), 1 << 30, size=shape)).astype(np.complex128)


def fft_residues(logn):
    return random_residues(np.random.default_rng(5000 + logn), moduli(logn, tuple(FFT_BITS))[:FFT_K], FFT_COUNT, 1 << logn)


def stride_values():
    """129 distinct vectors of integers in +-2^20 (at scale 2^16 the coefficients stay below 2^38 of the prime's 50 bits)"""
    rng = np.random.default_rng(6000)
    shape = (STRIDE_COUNT, (1 << STRIDE_LOGN) // 2)
    re = rng.integers(-(1 << 20), 1 << 20, size=shape).astype(np.float64)
    return re + 1j * rng.integers(-(1 << 20), 1 << 20, size=shape).astype(np.float64)


def stride_residues():
    return random_residues(np.random.default_rng(6001), moduli(STRIDE_LOGN, tuple(FFT_BITS))[:STRIDE_K], STRIDE_COUNT, 1 << STRIDE_LOGN)


def bits_of(z):
    return np.ascontiguousarray(z).view(np.uint64)


class Side:
    """a context on the device and the oracle's encoder over the same primes"""

    def __init__(self, S, logn, bits):
        self.logn, self.n = logn, 1 << logn
        self.mods = list(moduli(logn, tuple(bits)))
        self.ctx = S.Context(S.SCHEME_CKKS, logn, self.mods, 1, 0)
        self.ref = O.RefContext(CKKS, logn, self.mods, nsp=1)
        self.ck = O.CkksRef(self.ref)

    def encode_equals_oracle(self, values, k, scale, what):
        """the device's words of every item are the oracle's; returns them"""
        count = len(values)
        plain = self.ctx.ckks_encode(values, k, scale)
        got = plain.download((count, k, self.n))
        plain.free()
        for i in range(count):
            rc, want = self.ck.encode(values[i], k, scale)
            assert rc == 0, (what, "the oracle refuses item", i, rc)
            assert np.array_equal(got[i], want), (what, "encode", "item", i)
        return got

    def decode_equals_oracle(self, plain, k, scale, what):
        """the device's doubles of every item are the oracle's, bit for bit; returns them"""
        count = len(plain)
        d = self.ctx.upload(plain)
        got = self.ctx.ckks_decode(d, k, count, scale)
        d.free()
        for i in range(count):
            assert np.array_equal(bits_of(got[i]), bits_of(self.ck.decode(plain[i], scale))), (what, "decode", "item", i)
        return got

    def refused(self, values, k, scale, what):
        rc = [self.ck.encode(v, k, scale)[0] for v in values]
        assert -2 in rc and set(rc) <= {0, -2}, (what, "the oracle does not refuse it", rc)
        with pytest.raises(ValueError, match="encoded values are too large"):
            self.ctx.ckks_encode(values, k, scale)


@pytest.fixture(scope="module")
def limb_side(sealhip):
    return Side(sealhip, LIMB_LOGN, LIMB_BITS)


@pytest.fixture(scope="module")
def edge_side(sealhip):
    return Side(sealhip, EDGE_LOGN, EDGE_BITS)


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("k", LIMB_LEVELS)
def test_decode_at_every_compose_instance(limb_side, k):
    se, scale = limb_side, limb_scale(k)
    se.decode_equals_oracle(limb_residues(k), k, scale, ("random residues", k))
    consts = limb_constants(k)
    plains = np.stack([constant_plain(se.mods, k, se.n, h) for _, h in consts])
    dec = se.decode_equals_oracle(plains, k, scale, ("constants", k))
    by_name = {name: dec[i] for i, (name, _) in enumerate(consts)}
    assert np.all(by_name["zero"] == 0.0), k
    assert np.all(by_name["one"].real == 1.0 / scale), k
    assert np.all(by_name["minus one"].real == -1.0 / scale), k


def test_decode_refuses_33_primes_encode_does_not(limb_side):
    se, k = limb_side, OVER_LIMIT
    plain = se.ctx.upload(constant_plain(se.mods, k, se.n, 1)[None])
    with pytest.raises(ValueError, match="at most 32"):
        se.ctx.ckks_decode(plain, k, 1, LIMB_SCALE)
    plain.free()
    se.encode_equals_oracle(small_values(k), k, LIMB_SCALE, ("small values", k))
    se.encode_equals_oracle(wide_values(k), k, LIMB_SCALE, ("wide values", k))


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("k", LIMB_LEVELS)
def test_encode_coefficients_as_wide_as_the_modulus(limb_side, k):
    se, scale = limb_side, limb_scale(k)
    words = se.encode_equals_oracle(wide_values(k), k, scale, ("wide values", k))
    se.decode_equals_oracle(words, k, scale, ("wide values", k))


def test_single_prime_refuses_the_scale_of_the_other_levels(limb_side):
    se = limb_side
    assert se.ck.encode(small_values(1)[0], 1, LIMB_SCALE)[0] == -1
    with pytest.raises(ValueError, match="scale out of bounds"):
        se.ctx.ckks_encode(small_values(1), 1, LIMB_SCALE)
    plain = se.ctx.upload(limb_residues(1))
    with pytest.raises(ValueError, match="scale out of bounds"):
        se.ctx.ckks_decode(plain, 1, LIMB_COUNT, LIMB_SCALE)
    plain.free()


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("ulps", range(6))
def test_size_check_refuses_what_the_reference_refuses(edge_side, ulps):
    """c * 2^30 = 2^78 and the five doubles below it: log2 of each is 78 in the reference's arithmetic, 80 bits of 80"""
    edge_side.refused(constant_slots(EDGE_LOGN, REFUSED[ulps]), EDGE_K, EDGE_SCALE, ("2^48 less ulps", ulps))


@pytest.mark.parametrize("ulps", range(6))
def test_size_check_accepts_what_the_reference_accepts(edge_side, ulps):
    edge_side.encode_equals_oracle(constant_slots(EDGE_LOGN, ACCEPTED[ulps]), EDGE_K, EDGE_SCALE, ("2^47 less ulps", ulps))


def test_size_check_is_over_the_whole_batch(edge_side):
    edge_side.refused(edge_batch(), EDGE_K, EDGE_SCALE, "the edge value in the last item of three")


def test_regime_boundaries(sealhip):
    se = Side(sealhip, EDGE_LOGN, REGIME_BITS)
    for c in REGIME:
        se.encode_equals_oracle(constant_slots(EDGE_LOGN, c), REGIME_K, EDGE_SCALE, ("regime boundary", c.hex()))


def test_ties_and_negative_zero(edge_side):
    se = edge_side
    for x, _ in TIES:
        words = se.encode_equals_oracle(constant_slots(EDGE_LOGN, x / TIE_SCALE), EDGE_K, TIE_SCALE, ("tie", x))
        for r in range(EDGE_K):
            assert np.all(words[0, r] < se.mods[r]), ("a word is not canonical", x, r)


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("logn", FFT_LOGNS)
def test_fft_tails_above_the_tile(sealhip, logn):
    se = Side(sealhip, logn, FFT_BITS)
    v = fft_values(logn)
    words = se.encode_equals_oracle(v, FFT_K, FFT_SCALE, ("full input", logn))
    se.decode_equals_oracle(words, FFT_K, FFT_SCALE, ("encoded", logn))
    se.encode_equals_oracle(v[:, : se.n // 8].copy(), FFT_K, FFT_SCALE, ("short input", logn))
    se.decode_equals_oracle(fft_residues(logn), FFT_K, FFT_SCALE, ("arbitrary residues", logn))


def assert_one_chunk(log):
    """the operation logged its batch of 129 and nothing in the log was split: otherwise the stride loop was not reached"""
    assert (STRIDE_COUNT, STRIDE_COUNT) in log and all(chunk == logged for logged, chunk in log), log


def test_fft_two_layer_kernel_strides(sealhip):
    se = Side(sealhip, STRIDE_LOGN, FFT_BITS)
    assert STRIDE_COUNT << (STRIDE_LOGN - 2) > LAYER2_LANES
    se.ctx.chunk_log()
    se.encode_equals_oracle(stride_values(), STRIDE_K, STRIDE_SCALE, "129 plaintexts")
    assert_one_chunk(se.ctx.chunk_log())
    se.decode_equals_oracle(stride_residues(), STRIDE_K, STRIDE_SCALE, "129 plaintexts")
    assert_one_chunk(se.ctx.chunk_log())
