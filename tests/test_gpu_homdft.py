"""Homomorphic DFT on the device (sealhip_evaluator_coeffs_to_slots / _slots_to_coeffs and the sealhip_dft_* entries, DESIGN.md
section 23).

1. The generator kernel: the bits of its host restatement, and within 2^-40 gain 2^(-r or 0) of the numpy layer products
   (tests/homdft_ref.py). N = 2^4 is a ring below a workgroup, N = 2^6 with [5] a single full-width folded stage, N = 2^12 with
   [4,4,3] and [6,5] has folded and unfolded stages over many blocks.
2. The tables: every plaintext is, word for word, the oracle's encoding of the device's own values at the key level.
3. The transforms' words: those of the same stages issued one by one through rotate_vector_bsgs_plain_rescale, composed on the
   oracle with conjugation, add, sub and the dyadic product; at N = 2^6 also the CPU chain of tests/ks_rescale_ref.py.
4. End to end with real keys at N = 2^12, Delta = 2^40: slots against coefficients, the round trip against the message, the
   error against the same chain over numpy-made, oracle-encoded diagonals.
5. Boundary behaviour."""
import ctypes as C

import numpy as np
import pytest

import hoist_ref as H
import homdft_ref as R
import ks_rescale_ref as KR
import oracle_lib as O
from support import BaseSession, S, compile_cpp, rows, run_exe, session_memo

pytestmark = pytest.mark.gpu


def _download(S, ctx, ptr, shape):
    out = np.empty(shape, dtype=np.uint64)
    ctx.synchronize()
    S._check(S.lib().sealhip_memcpy_d2h(ctx.handle, out.ctypes.data, ptr, out.nbytes))
    return out


_MATRICES = {}


def _grid(n_ring, direction, s0, r, n_baby=None):
    """(W, baby, giant) of a stage from its layers, computed once"""
    key = (n_ring, direction, s0, r, n_baby)
    if key not in _MATRICES:
        _MATRICES[key] = R.bsgs_grid(R.stage_matrix(n_ring, direction, s0, r), s0, r, n_baby)
    return _MATRICES[key]


def _numpy_values(n_ring, direction, counts, t, gain):
    s0, r = R.stage_layout(n_ring, direction, counts)[t]
    return _grid(n_ring, direction, s0, r)[0] * R.stage_gain(direction, t, len(counts), gain)


class Session(BaseSession):
    """contexts on both sides; keys are random words unless a client makes real ones"""

    def __init__(self, S, logn, bits, nsp, mode=0, seed=0):
        super().__init__(S, S.SCHEME_CKKS, logn, bits, nsp, mode, 0, seed + 31 * logn + nsp)
        self.n_key = len(self.mods)
        self.host_keys, self.dev_keys = {}, {}

    def random_keys(self, steps, conj):
        elts = [H.elt_from_step(self.n, s) for s in steps] + ([2 * self.n - 1] if conj else [])
        for g in elts:
            if g not in self.host_keys:
                self.host_keys[g] = rows(self.rng, self.mods, self.n, (self.nd, 2))
                self.dev_keys[g] = self.S.KSwitchKeys(self.ctx, self.host_keys[g])
        return {g: self.dev_keys[g] for g in elts}

    def xhalf(self, k):
        """NTT(X^(N/2)) over the first k primes: multiplication by i"""
        out = np.zeros((k, self.n), dtype=np.uint64)
        out[:, self.n // 2] = 1
        for r in range(k):
            O.lib().ref_ntt_forward(O.ptr(out[r]), self.ref.tables(r), 0)
        return out

    # ---- the oracle's composition of the split and the merge on host words
    def _dyadic(self, a, b, k):
        out = np.zeros_like(a)
        for r in range(k):
            O.lib().ref_dyadic_product_coeffmod(O.ptr(np.ascontiguousarray(a[r])), O.ptr(np.ascontiguousarray(b[r])), self.n,
                                                C.byref(self.ref.c.key_mod[r]), O.ptr(out[r]))
        return out

    def oracle_split(self, c, k):
        """c: (count, 2, k, N) -> re, im"""
        L, xh, conj_key = O.lib(), self.xhalf(k), self.host_keys[2 * self.n - 1]
        re, im = np.zeros_like(c), np.zeros_like(c)
        for i in range(c.shape[0]):
            s = np.ascontiguousarray(c[i]).copy()
            assert L.ref_apply_galois_inplace(C.byref(self.ref.c), k, O.ptr(s), 2 * self.n - 1, O.ptr(conj_key)) == 0
            a = np.ascontiguousarray(c[i])
            diff = np.zeros_like(a)
            L.ref_evaluator_add(C.byref(self.ref.c), k, O.ptr(a), 2, O.ptr(s), 2, O.ptr(re[i]))
            L.ref_evaluator_sub(C.byref(self.ref.c), k, O.ptr(s), 2, O.ptr(a), 2, O.ptr(diff))  # -i (a - s) = i (s - a)
            for p in range(2):
                im[i, p] = self._dyadic(diff[p], xh, k)
        return re, im

    def oracle_merge(self, re, im, k):
        L, xh = O.lib(), self.xhalf(k)
        out = np.zeros_like(re)
        for i in range(re.shape[0]):
            t = np.zeros_like(re[i])
            for p in range(2):
                t[p] = self._dyadic(im[i, p], xh, k)
            L.ref_evaluator_add(C.byref(self.ref.c), k, O.ptr(np.ascontiguousarray(re[i])), 2, O.ptr(t), 2, O.ptr(out[i]))
        return out

    def stages_one_by_one(self, plan, table_ptrs, ct, count, gk):
        """the plan's stages through rotate_vector_bsgs_plain_rescale, from Python: device buffer in -> device buffer out"""
        cur = ct
        for t, st in enumerate(plan["stages"]):
            out = self.ctx.alloc(count * 2 * (st["level"] - 1) * self.n)
            self.ev.rotate_vector_bsgs_plain_rescale(cur, st["level"], count, st["baby_steps"], st["giant_steps"], gk,
                                                     table_ptrs[t], out)
            cur = out
        return cur


_made = session_memo(Session)


def _session(S, logn, bits, nsp, mode=0):
    return _made(S, logn, list(bits), nsp, mode)


# ------------------------------------------------------------------ 1. the generator
GENERATOR_SHAPES = [(4, [3]), (4, [2, 1]), (6, [5]), (12, [4, 4, 3]), (12, [6, 5])]


@pytest.mark.parametrize("logn,counts", GENERATOR_SHAPES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("direction", [R.C2S, R.S2C], ids=["c2s", "s2c"])
def test_generator_values(S, logn, counts, direction):
    se = _session(S, logn, [40] * 6, 1)
    gain, k = 1.5, 5
    worst = 0.0
    for t, (s0, r) in enumerate(R.stage_layout(se.n, direction, counts)):
        dev = se.ev.dft_stage_values(direction, k, counts, t, gain=gain)
        host = se.ev.dft_stage_values(direction, k, counts, t, gain=gain, host=True)
        assert np.array_equal(dev.view(np.uint64), host.view(np.uint64)), (t, "device and host restatement differ in bits")
        want = _numpy_values(se.n, direction, counts, t, gain)
        f = R.stage_gain(direction, t, len(counts), gain)
        bar = 2.0 ** -40 * abs(f) * (2.0 ** -r if direction == R.C2S else 1.0)
        err = float(np.max(np.abs(dev - want)))
        worst = max(worst, err / bar)
        assert err <= bar, (t, err, bar)
        assert np.array_equal(dev == 0, want == 0)
    print("generator N=2^%d %s direction %d: worst error / bar = %.3g" % (logn, counts, direction, worst))


# ------------------------------------------------------------------ 2. the tables
@pytest.mark.parametrize("logn,counts", [(4, [2, 1]), (6, [5]), (12, [4, 4, 3])], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("direction", [R.C2S, R.S2C], ids=["c2s", "s2c"])
def test_tables_are_the_encoding_of_the_device_values(S, logn, counts, direction):
    se = _session(S, logn, [40] * 6, 1)
    enc = O.CkksRef(se.ref)
    k, gain = 5, 0.75
    tables = S.DftTables(se.ctx, direction, k, counts, gain=gain)
    plan = se.ev.dft_plan(direction, k, counts)
    assert tables.plan["table_words"] == plan["table_words"] == sum(
        st["n_giant"] * st["n_baby"] * se.n_key * se.n for st in plan["stages"])
    for t, st in enumerate(plan["stages"]):
        values = se.ev.dft_stage_values(direction, k, counts, t, gain=gain)
        got = _download(S, se.ctx, tables.stage_ptr(t), (st["n_giant"], st["n_baby"], se.n_key, se.n))
        assert st["scale"] == float(se.mods[st["level"] - 1])
        for g in range(st["n_giant"]):
            for b in range(st["n_baby"]):
                rc, want = enc.encode(values[g, b], se.n_key, st["scale"])
                assert rc == 0 and np.array_equal(got[g, b], want), (t, g, b)
    tables.free()


# ------------------------------------------------------------------ 3. the words
def _check_words(S, se, counts, k, count, cpu_chain=False):
    n = se.n
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    d_ct = se.ctx.upload(ct)
    # CoeffToSlot
    plan = se.ev.dft_plan(R.C2S, k, counts)
    gk = se.random_keys(plan["key_steps"], conj=True)
    tables = S.DftTables(se.ctx, R.C2S, k, counts)
    ko = plan["out_level"]
    re, im = se.ctx.alloc(count * 2 * ko * n), se.ctx.alloc(count * 2 * ko * n)
    se.ev.coeffs_to_slots(tables, d_ct, count, gk, re, im)
    got_re, got_im = re.download((count, 2, ko, n)), im.download((count, 2, ko, n))
    ptrs = [tables.stage_ptr(t) for t in range(len(counts))]
    table_words = [_download(S, se.ctx, ptrs[t], (st["n_giant"], st["n_baby"], se.n_key, n)) for t, st in enumerate(plan["stages"])]
    mid = se.stages_one_by_one(plan, ptrs, d_ct, count, gk).download((count, 2, ko, n))
    want_re, want_im = se.oracle_split(mid, ko)
    assert np.array_equal(got_re, want_re) and np.array_equal(got_im, want_im), "coeffs_to_slots"
    assert np.array_equal(d_ct.download(ct.shape), ct), "the input was modified"
    for t, st in enumerate(plan["stages"]):
        assert np.array_equal(_download(S, se.ctx, ptrs[t], table_words[t].shape), table_words[t]), "the tables were modified"
    if cpu_chain:
        cur = ct
        for t, st in enumerate(plan["stages"]):
            baby = [1 if s == 0 else H.elt_from_step(n, s) for s in st["baby_steps"]]
            giant = [1 if s == 0 else H.elt_from_step(n, s) for s in st["giant_steps"]]
            cur = KR.bsgs_plain_rescale(se.ref, st["level"], cur, baby, [se.host_keys.get(g) for g in baby], giant,
                                        [se.host_keys.get(g) for g in giant], table_words[t])
        assert np.array_equal(cur, mid), "the CPU chain differs"
    tables.free()
    # SlotToCoeff, on fresh random operands at its own entry level
    plan = se.ev.dft_plan(R.S2C, k, counts)
    gk = se.random_keys(plan["key_steps"], conj=False)
    tables = S.DftTables(se.ctx, R.S2C, k, counts)
    a, b = rows(se.rng, se.mods[:k], n, (count, 2)), rows(se.rng, se.mods[:k], n, (count, 2))
    d_a, d_b = se.ctx.upload(a), se.ctx.upload(b)
    out = se.ctx.alloc(count * 2 * ko * n)
    se.ev.slots_to_coeffs(tables, d_a, d_b, count, gk, out)
    ptrs = [tables.stage_ptr(t) for t in range(len(counts))]
    merged = se.oracle_merge(a, b, k)
    want = se.stages_one_by_one(plan, ptrs, se.ctx.upload(merged), count, gk).download((count, 2, ko, n))
    assert np.array_equal(out.download((count, 2, ko, n)), want), "slots_to_coeffs"
    assert np.array_equal(d_a.download(a.shape), a) and np.array_equal(d_b.download(b.shape), b), "an input was modified"
    if cpu_chain:
        cur = merged
        for t, st in enumerate(plan["stages"]):
            tw = _download(S, se.ctx, ptrs[t], (st["n_giant"], st["n_baby"], se.n_key, n))
            baby = [1 if s == 0 else H.elt_from_step(n, s) for s in st["baby_steps"]]
            giant = [1 if s == 0 else H.elt_from_step(n, s) for s in st["giant_steps"]]
            cur = KR.bsgs_plain_rescale(se.ref, st["level"], cur, baby, [se.host_keys.get(g) for g in baby], giant,
                                        [se.host_keys.get(g) for g in giant], tw)
        assert np.array_equal(cur, want), "the CPU chain differs"
    tables.free()


@pytest.mark.parametrize("nsp,counts", [(1, [4, 4, 3]), (2, [6, 5])], ids=["nsp1-443", "nsp2-65"])
@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
@pytest.mark.parametrize("count", [1, 5])
def test_transform_words_are_the_stages_one_by_one(S, nsp, counts, mode, count):
    se = _session(S, 12, [40] * (5 + nsp), nsp, mode)
    _check_words(S, se, counts, 5, count)


@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
def test_transform_words_small_ring_and_cpu_chain(S, mode):
    se = _session(S, 6, [40] * 5, 1, mode)
    _check_words(S, se, [3, 2], 4, 2, cpu_chain=True)


# ------------------------------------------------------------------ 4. end to end
def _real_keys(S, se, cl, steps):
    elts = sorted({H.elt_from_step(se.n, s) for s in steps} | {2 * se.n - 1})
    d = se.nd
    seeds = se.rng.integers(0, 2**64, size=(len(elts), d, 8), dtype=np.uint64, endpoint=False)
    noise = se.rng.integers(-6, 7, size=(len(elts), d, se.n), dtype=np.int32)
    keys = se.ctx.generate_galois_keys(se.ctx.upload(cl.sk), elts, seeds, se.ctx.upload_i32(noise))
    return dict(zip(elts, keys))


def test_end_to_end_with_real_keys(S):
    """N = 2^12, Delta = 2^40, q_0 of 50 bits, five 40-bit primes, a special prime of 59 bits: CoeffToSlot [4,4,3] from
    level 6 to 3, SlotToCoeff [6,5] from 3 to 1. The device may err at most twice as much as the same chain over numpy-made, oracle-encoded
    diagonals through the entries that existed before. Measured on the MI355X: CoeffToSlot 9.22e-8 on both; round trip
    8.04e-9 (device) against 7.99e-9 (reference chain), in units of Delta."""
    logn, n, half, delta = 12, 1 << 12, 1 << 11, 2.0 ** 40
    se = _session(S, logn, [50] + [40] * 5 + [59], 1)
    cl = O.Client(se.ref, seed=23)
    ev, ctx = se.ev, se.ctx
    k, c2s_counts, s2c_counts = 6, [4, 4, 3], [6, 5]
    p1 = ev.dft_plan(R.C2S, k, c2s_counts)
    p2 = ev.dft_plan(R.S2C, p1["out_level"], s2c_counts)
    gk = _real_keys(S, se, cl, p1["key_steps"] + p2["key_steps"])
    rng = np.random.default_rng(5)
    m = rng.integers(-(1 << 39), 1 << 39, size=n).astype(np.int64)
    scale_m = float(np.max(np.abs(m))) / delta
    ct = ctx.upload(cl.encrypt_poly_ntt([int(v) for v in m]))
    sk = ctx.upload(cl.sk_powers(1))
    perm = R.bitrev_perm(half)

    def slots_of(buf, level):
        plain = ctx.alloc(level * n)
        ctx.decrypt(buf, 2, level, 1, sk, True, plain)
        return ctx.ckks_decode(plain, level, 1, delta)[0]

    def coeffs_of(buf, level):
        plain = ctx.alloc(level * n)
        ctx.decrypt(buf, 2, level, 1, sk, True, plain)
        vals, _ = cl.centered_from_ntt_rows(plain.download((level, n)))
        return np.array([float(v) for v in vals])

    def c2s_error(re, im, level):
        zr, zi = slots_of(re, level), slots_of(im, level)
        return max(np.max(np.abs(zr - m[perm] / delta)), np.max(np.abs(zi - m[perm + half] / delta)))

    # the device's transforms
    t1, t2 = S.DftTables(ctx, R.C2S, k, c2s_counts), S.DftTables(ctx, R.S2C, p1["out_level"], s2c_counts)
    lo, l1 = p1["out_level"], p2["out_level"]
    re, im, back = ctx.alloc(2 * lo * n), ctx.alloc(2 * lo * n), ctx.alloc(2 * l1 * n)
    ev.coeffs_to_slots(t1, ct, 1, gk, re, im)
    ev.slots_to_coeffs(t2, re, im, 1, gk, back)
    dev_c2s = c2s_error(re, im, lo)
    dev_rt = np.max(np.abs(coeffs_of(back, l1) - m)) / delta

    # the reference: numpy-made, oracle-encoded diagonals through the existing entries
    enc = O.CkksRef(se.ref)

    def oracle_tables(direction, counts, plan):
        ptrs = []
        for t, st in enumerate(plan["stages"]):
            vals = _numpy_values(n, direction, counts, t, 1.0)
            words = np.zeros((st["n_giant"], st["n_baby"], se.n_key, n), dtype=np.uint64)
            for g in range(st["n_giant"]):
                for b in range(st["n_baby"]):
                    rc, words[g, b] = enc.encode(vals[g, b], se.n_key, st["scale"])
                    assert rc == 0
            ptrs.append(ctx.upload(words))
        return ptrs

    r1, r2 = oracle_tables(R.C2S, c2s_counts, p1), oracle_tables(R.S2C, s2c_counts, p2)
    mid = se.stages_one_by_one(p1, r1, ct, 1, gk)
    conj = ctx.upload(mid.download())
    ev.apply_galois_inplace(conj, lo, 1, 2 * n - 1, gk[2 * n - 1])
    xh = ctx.upload(np.stack([se.xhalf(lo)] * 2))
    ref_re, diff, ref_im, tmp, merged = (ctx.alloc(2 * lo * n) for _ in range(5))
    ev.add(mid, 2, conj, 2, lo, 1, ref_re)
    ev.sub(conj, 2, mid, 2, lo, 1, diff)
    ctx.dyadic_product_coeffmod(diff, xh, 2, lo, ref_im)
    ref_c2s = c2s_error(ref_re, ref_im, lo)
    ctx.dyadic_product_coeffmod(ref_im, xh, 2, lo, tmp)
    ev.add(ref_re, 2, tmp, 2, lo, 1, merged)
    ref_back = se.stages_one_by_one(p2, r2, merged, 1, gk)
    ref_rt = np.max(np.abs(coeffs_of(ref_back, l1) - m)) / delta

    print("coeffs_to_slots: max slot error device %.3g reference chain %.3g; round trip: max coefficient error / Delta device "
          "%.3g reference chain %.3g; max|m| / Delta = %.3g" % (dev_c2s, ref_c2s, dev_rt, ref_rt, scale_m))
    assert ref_c2s < 2.0 ** -16 * scale_m and ref_rt < 2.0 ** -16 * scale_m, "the primes do not carry the reference chain"
    assert dev_c2s <= 2 * ref_c2s, (dev_c2s, ref_c2s)
    assert dev_rt <= 2 * ref_rt, (dev_rt, ref_rt)


# ------------------------------------------------------------------ 5. boundary behaviour
def test_checks_flags_capture(S):
    se = _session(S, 6, [40] * 5, 1)
    ctx, ev, n, k, counts, count = se.ctx, se.ev, se.n, 4, [3, 2], 3
    plan = ev.dft_plan(R.C2S, k, counts)
    gk = se.random_keys(plan["key_steps"], conj=True)
    c2s, s2c = S.DftTables(ctx, R.C2S, k, counts), S.DftTables(ctx, R.S2C, k, counts)
    gk2 = se.random_keys(ev.dft_plan(R.S2C, k, counts)["key_steps"], conj=False)
    ko = plan["out_level"]
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    d_ct = ctx.upload(ct)
    re, im, out = (ctx.alloc(count * 2 * ko * n) for _ in range(3))
    # a missing key: a step's, and the conjugation's
    for drop in (H.elt_from_step(n, plan["key_steps"][-1]), 2 * n - 1):
        fewer = {g: key for g, key in gk.items() if g != drop}
        with pytest.raises(ValueError, match="Galois key not present"):
            ev.coeffs_to_slots(c2s, d_ct, count, fewer, re, im)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.slots_to_coeffs(s2c, d_ct, d_ct, count, {}, out)
    # tables of the other direction; overlapping buffers
    with pytest.raises(ValueError, match="slots_to_coeffs"):
        ev.coeffs_to_slots(s2c, d_ct, count, gk, re, im)
    with pytest.raises(ValueError, match="coeffs_to_slots"):
        ev.slots_to_coeffs(c2s, d_ct, d_ct, count, gk2, out)
    with pytest.raises(ValueError, match="overlap"):
        ev.coeffs_to_slots(c2s, d_ct, count, gk, re, re)
    with pytest.raises(ValueError, match="overlap"):
        ev.coeffs_to_slots(c2s, d_ct, count, gk, d_ct, im)
    with pytest.raises(ValueError, match="overlap"):
        ev.slots_to_coeffs(s2c, d_ct, d_ct, count, gk2, d_ct)
    # pointers the split and merge kernels cannot take; tables of another context
    with pytest.raises(ValueError, match="16-byte aligned"):
        ev.coeffs_to_slots(c2s, d_ct, count, gk, re.ptr + 8, im)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ev.slots_to_coeffs(s2c, d_ct, d_ct.ptr + 8, count, gk2, out)
    other = S.Context(S.SCHEME_CKKS, 6, se.mods, 1, 0)
    with pytest.raises(ValueError, match="another context"):
        S.Evaluator(other).coeffs_to_slots(c2s, d_ct, count, gk, re, im)
    with pytest.raises(ValueError, match="another context"):
        S.Evaluator(other).slots_to_coeffs(s2c, d_ct, d_ct, count, gk2, out)
    # the level: no room for the stages below it, or above the first level
    for bad_k in (2, 5):
        with pytest.raises(ValueError):
            S.DftTables(ctx, R.C2S, bad_k, counts)
    # BFV
    bfv = S.Context(S.SCHEME_BFV, 6, se.mods, 1, 65537, mode=S.MODE_STRICT)
    with pytest.raises(ValueError, match="CKKS only"):
        S.DftTables(bfv, R.C2S, k, counts)
    # the empty batch launches nothing
    ev.coeffs_to_slots(c2s, d_ct, 0, gk, re, im)
    ev.slots_to_coeffs(s2c, d_ct, d_ct, 0, gk2, out)
    # transparency flags: one per output ciphertext; a zero ciphertext is transparent in both outputs
    flags = ctx.alloc(4)  # 8 x 32 bits
    zeroed = ct.copy()
    zeroed[1] = 0
    d_z = ctx.upload(zeroed)
    ctx.transparency_sink(flags, 8)
    ev.coeffs_to_slots(c2s, d_z, count, gk, re, im)
    f = flags.download().view(np.uint32)[:2 * count]
    assert list(f != 0) == [True, False, True] * 2, f
    ev.slots_to_coeffs(s2c, d_z, d_z, count, gk2, out)
    f = flags.download().view(np.uint32)[:count]
    assert list(f != 0) == [True, False, True], f
    with pytest.raises(ValueError, match="transparency sink"):
        ev.coeffs_to_slots(c2s, ctx.upload(rows(se.rng, se.mods[:k], n, (5, 2))), 5, gk, ctx.alloc(5 * 2 * ko * n),
                           ctx.alloc(5 * 2 * ko * n))
    ctx.transparency_sink(None, 0)
    # graph capture: a replay gives the eager words; the workspace is pool memory the tables hold
    ev.coeffs_to_slots(c2s, d_ct, count, gk, re, im)
    assert ctx.pool_stats()["bytes_in_use"] >= count * c2s.plan["temp_bytes_per_item"]
    want_re, want_im = re.download().copy(), im.download().copy()
    ev.slots_to_coeffs(s2c, d_ct, d_ct, count, gk2, out)
    want_out = out.download().copy()

    def both():
        ev.coeffs_to_slots(c2s, d_ct, count, gk, re, im)
        ev.slots_to_coeffs(s2c, d_ct, d_ct, count, gk2, out)

    graph = ctx.capture(both)
    for buf in (re, im, out):
        ctx.memset_zero(buf, buf.words * 8)
    graph.launch()
    assert np.array_equal(re.download(), want_re) and np.array_equal(im.download(), want_im)
    assert np.array_equal(out.download(), want_out)
    with pytest.raises(S.LogicError):
        ctx.capture(lambda: S.DftTables(ctx, R.C2S, k, counts))


def test_cpp_adapter(tmp_path):
    """tests/host_adapter_homdft_check.cpp: the host-ciphertext and the DeviceCiphertext forms give the C ABI's words on the
    same seeded inputs, at the plan's level and the operand's scale; the operand checks and their messages"""
    exe = compile_cpp(tmp_path, "host_adapter_homdft_check.cpp", link_sealhip=True)
    mods = O.coeff_modulus_create(256, [40] * 5)
    assert "homdft adapter checks ok" in run_exe(exe, "0", *mods, timeout=120)
