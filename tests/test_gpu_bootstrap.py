"""CKKS bootstrapping on the device: sealhip_evaluator_mod_raise, _double_angle, _eval_mod and
_bootstrap.

1. ModRaise, word for word against the restatement over the oracle's transforms (tests/bootstrap_ref.py). N = 2^3 is smaller
   than one wavefront's worth of vector loads, 2^12 takes the small-ring transforms and 2^14 the half-row ones; a 61-bit q_0
   over 30-bit q_i needs a real reduction of the centred value, a 50-bit q_0 under 54-bit q_i none, and a 40-bit q_0 takes
   the FP64 transform instance at 2^14. One input holds 0, (q_0 - 1) / 2, (q_0 + 1) / 2 and q_0 - 1 in coefficient form.
2. The double-angle step, word for word against the three entries it merges, issued one by one; EvalMod against the
   polynomial evaluator followed by double_angle calls; the bootstrap end to end with real keys and a sparse secret.
3. Boundary behaviour: the header's refusals, the empty batch, host-only contexts, transparency flags, graph capture."""

import numpy as np
import pytest

import bootstrap_ref as B
import hoist_ref as H
import homdft_ref as R
import oracle_lib as O
import poly_eval_ckks_ref as PC
from support import S, compile_cpp, rows, run_exe

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. ModRaise
def _prime_set(name, logn):
    """five data primes and one 60-bit special prime"""
    n = 1 << logn
    if name == "61over30":
        q0 = O.ntt_primes_around(1 << 61, logn)[0][0]
        assert q0.bit_length() == 61
        return [q0] + O.get_primes(n, 30, 4) + O.get_primes(n, 60, 1)
    if name == "50under54":
        return O.get_primes(n, 50, 1) + O.get_primes(n, 54, 4) + O.get_primes(n, 60, 1)
    assert name == "40"
    return O.get_primes(n, 40, 5) + O.get_primes(n, 60, 1)


_RAISE_CASES = {}


def _raise_case(logn, primes, k_in, k_out, count):
    """(mods, input, restated output), computed once and shared by both modes"""
    key = (logn, primes, k_in, k_out, count)
    if key not in _RAISE_CASES:
        n = 1 << logn
        mods = _prime_set(primes, logn)
        ref = O.RefContext(2, logn, mods, nsp=1, t=0, mode=0)
        rng = np.random.default_rng(1000 * logn + 10 * k_in + count)
        ct = rows(rng, mods[:k_in], n, (count, 2))
        # the q_0 row of component 0 of the last item: the centring's edges in coefficient form, then transformed
        q0 = mods[0]
        coef = rng.integers(0, q0, size=n, dtype=np.uint64)
        coef[:4] = [0, (q0 - 1) // 2, (q0 + 1) // 2, q0 - 1]
        O.lib().ref_ntt_forward(O.ptr(coef), ref.tables(0), 0)
        ct[count - 1, 0, 0] = coef
        _RAISE_CASES[key] = (mods, ct, B.mod_raise(ref, ct, k_out))
    return _RAISE_CASES[key]


@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
@pytest.mark.parametrize("primes", ["61over30", "50under54", "40"])
@pytest.mark.parametrize("logn", [3, 12, 14])
def test_mod_raise_words(S, logn, primes, mode):
    n = 1 << logn
    ctx = ev = None
    for k_in, k_out in ((1, 2), (3, 5)):
        for count in (1, 3):
            mods, ct, want = _raise_case(logn, primes, k_in, k_out, count)
            if ctx is None:
                ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0, mode=mode)
                ev = S.Evaluator(ctx)
            d_ct, d_out = ctx.upload(ct), ctx.alloc(count * 2 * k_out * n)
            ev.mod_raise(d_ct, k_in, count, k_out, d_out)
            got = d_out.download().reshape(count, 2, k_out, n)
            assert np.array_equal(got[:, :, 0], ct[:, :, 0]), "row 0 is the input's"
            assert np.array_equal(got, want), (k_in, k_out, count)
            assert np.array_equal(d_ct.download().reshape(ct.shape), ct), "the input is not modified"


def test_mod_raise_decrypts_to_m_plus_q0_I(S):
    """the raised ciphertext decrypts to m + q_0 I with a small integer polynomial I (N = 2^6, a real secret)"""
    logn, n = 6, 64
    mods = O.get_primes(n, 40, 1) + O.get_primes(n, 45, 2) + O.get_primes(n, 60, 1)
    ref = O.RefContext(2, logn, mods, nsp=1, t=0, mode=0)
    cl = O.Client(ref, seed=5)
    rng = np.random.default_rng(7)
    m = [int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=n)]
    low = np.ascontiguousarray(cl.encrypt_poly_ntt(m)[:, :1])  # mod_switch_to level 1: the q_0 rows
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    d_out = ctx.alloc(2 * 3 * n)
    S.Evaluator(ctx).mod_raise(ctx.upload(low), 1, 1, 3, d_out)
    up = d_out.download().reshape(2, 3, n)
    dot = up[0].copy()
    for r in range(3):
        t = np.zeros(n, dtype=np.uint64)
        O.lib().ref_dyadic_product_coeffmod(O.ptr(np.ascontiguousarray(up[1, r])), O.ptr(cl.sk[r]), n,
                                            O.C.byref(ref.c.key_mod[r]), O.ptr(t))
        O.lib().ref_add_poly_coeffmod(O.ptr(dot[r]), O.ptr(t), n, O.C.byref(ref.c.key_mod[r]), O.ptr(dot[r]))
    c, _ = cl.centered_from_ntt_rows(dot)
    q0 = mods[0]
    I = [round((c[j] - m[j]) / q0) for j in range(n)]
    h = int(np.count_nonzero(cl.s))
    assert max(abs(v) for v in I) <= (h + 1) // 2 + 1
    assert max(abs(c[j] - m[j] - q0 * I[j]) for j in range(n)) < 1 << 10, "what is left is the encryption's noise"
    assert any(I), "a raise that never wraps tests nothing"


# ------------------------------------------------------------------ 2. the double-angle step
def _three_entry_chain(S, ctx, ev, mods, k, d_ct, count, scale, rk, n):
    """2 ct^2 - rint(scale^2) through dot_product without keys, linear_combination_levels and relinearize_rescale"""
    wide, comb = ctx.alloc(count * 3 * k * n), ctx.alloc(count * 3 * k * n)
    ev.dot_product([d_ct], [d_ct], k, count, wide)
    w = ctx.upload(np.array([2 % p for p in mods[:k]], dtype=np.uint64))
    kc = ctx.upload(np.array(PC.residues(-float(PC.rint(scale * scale)), mods[:k]), dtype=np.uint64))
    ev.linear_combination_levels([wide], [k], [3], w, k, count, comb, size=3, n_sums=1, constant=kc)
    out = ctx.alloc(count * 2 * (k - 1) * n)
    ev.relinearize_rescale(comb, k, count, rk, out)
    return out.download()


_DA_CASES = [(12, [50, 50, 60], 1, 2), (12, [40, 45, 50, 50, 45, 60, 60], 2, 5), (12, [54, 54, 54, 54, 54, 60], 1, 5),
             (14, [50, 45, 50, 60, 60], 2, 2)]


@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
@pytest.mark.parametrize("logn,bits,nsp,k", _DA_CASES, ids=["k2-1sp", "k5-2sp", "k5-1sp", "n14-k2-2sp"])
def test_double_angle_words(S, logn, bits, nsp, k, mode):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, nsp, 0, mode=mode)
    ev = S.Evaluator(ctx)
    k_first = len(mods) - nsp
    nd = (k_first + nsp - 1) // nsp
    rng = np.random.default_rng(17 * logn + k + nsp)
    rk = [S.KSwitchKeys(ctx, rows(rng, mods, n, (nd, 2)))]
    for count in (1, 5):
        for scale in (2.0 ** 40, 2.0 ** 53.6):  # the second one's square exceeds 2^64
            ct = rows(rng, mods[:k], n, (count, 2))
            d_ct, d_out = ctx.upload(ct), ctx.alloc(count * 2 * (k - 1) * n)
            out_scale = ev.double_angle(d_ct, k, count, scale, rk, d_out)
            assert out_scale == scale * scale / float(mods[k - 1])
            want = _three_entry_chain(S, ctx, ev, mods, k, d_ct, count, scale, rk, n)
            assert np.array_equal(d_out.download(), want), (count, scale)


# ------------------------------------------------------------------ 2b. EvalMod
@pytest.mark.parametrize("K,r,d,n_baby,k", [(12, 3, 31, 8, 10), (4, 1, 7, 0, 6)], ids=["12-3-31", "4-1-7"])
def test_eval_mod_words(S, K, r, d, n_baby, k):
    """the words of evaluate_polynomial_ckks with the plan's t_0 and the library's coefficients, then r double_angle calls"""
    logn, n = 12, 1 << 12
    mods = O.get_primes(n, 50, k) + O.get_primes(n, 60, 2)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 2, 0)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(100 * K + d)
    rk = [S.KSwitchKeys(ctx, rows(rng, mods, n, ((k + 1) // 2, 2)))]
    s_x = 2.0 ** 50
    plan = ev.evalmod_plan(k, s_x, K, r, d, n_baby=n_baby)
    assert plan["out_level"] == plan["poly_level"] - r >= 1
    for count in (1, 2):
        d_ct = ctx.upload(rows(rng, mods[:k], n, (count, 2)))
        out = ctx.alloc(count * 2 * plan["out_level"] * n)
        level, scale = ev.eval_mod(d_ct, k, count, s_x, K, r, d, rk, out, n_baby=n_baby)
        assert (level, scale) == (plan["out_level"], plan["out_scale"])
        cur = ctx.alloc(count * 2 * plan["poly_level"] * n)
        lv, sc = ev.evaluate_polynomial_ckks(d_ct, plan["coeffs"], k, count, s_x, cur, relin_keys=rk, basis=1, n_baby=n_baby,
                                             scale_out=plan["poly_scale_out"])
        assert (lv, sc) == (plan["poly_level"], plan["scales"][0])
        for i in range(1, r + 1):
            nxt = ctx.alloc(count * 2 * (lv - 1) * n)
            sc = ev.double_angle(cur, lv, count, sc, rk, nxt)
            assert sc == plan["scales"][i]
            cur, lv = nxt, lv - 1
        assert np.array_equal(out.download(), cur.download()), count
    assert ctx.pool_stats()["bytes_in_use"] == 0, "the temporaries went back to the pool"


# ------------------------------------------------------------------ 2c. the bootstrap, end to end
class SparseClient(O.Client):
    """oracle_lib.Client with its secret replaced by a fixed-seed ternary vector of Hamming weight h (the library does not
    sample such secrets; the test makes one so that K = 12 bounds ModRaise's integer polynomial)"""

    def __init__(self, ref, h, seed):
        super().__init__(ref, seed=seed)
        rng = np.random.default_rng(seed)
        s = np.zeros(self.n, dtype=np.int8)
        s[rng.choice(self.n, size=h, replace=False)] = rng.choice(np.array([-1, 1], dtype=np.int8), size=h)
        self.s = s
        self.sk = np.zeros((self.n_key, self.n), dtype=np.uint64)
        O.lib().ref_small_poly_to_rns(O.C.byref(ref.c), s.ctypes.data, self.n_key, 1, O.ptr(self.sk))


def _primes_next_to(value, logn, count):
    """`count` NTT primes next to `value`, alternately above and below, from oracle_lib.ntt_primes_around"""
    below, above = O.ntt_primes_around(value, logn)
    while len(below) + len(above) < count + 2:
        below += O.ntt_primes_around(below[-1] - 1, logn)[0]
        above += O.ntt_primes_around(above[-1], logn)[1]
    out = []
    for lo, hi in zip(below, above):
        out += [hi, lo]
    assert len(set(out)) == len(out)
    return out[:count]


def test_bootstrap_end_to_end(S):
    """N = 2^12 -- NOT a secure ring, a test shape --, q_0 of 50 bits, fifteen primes next to 12 q_0, two 59-bit special primes;
    a ternary secret of Hamming weight 32; m uniform in +-2^39. (59 bits, not 60: at N = 2^12 a key switch with even one
    60-bit special prime does not decrypt on the oracle itself, in either mode: key generation transforms the noise with
    the reference's uncorrected forward butterflies, which wrap modulo 2^64 there -- DESIGN.md section 24. The existing
    end-to-end tests use 59 bits too.) ModRaise to level 16, CoeffToSlot [4,4,3] to 13, EvalMod
    (K 12, r 3, degree 31, eight baby steps) to 4, SlotToCoeff [6,5] to 2.
    1. the raised ciphertext decrypts to m + q_0 I with max|I| <= K - 1;
    2. the words of bootstrap are those of the chain through the entries that existed before it;
    3. that chain's decrypted coefficients are within 2^-16 max|m| of m (the sine term alone is 2^-19.3).
    Measured on the MI355X: max|I| = 5; max coefficient error / max|m| = 2^-19.29, the sine term: the chain's CKKS noise
    does not show at these primes."""
    logn, n, K, r, d, nb = 12, 1 << 12, 12, 3, 31, 8
    q0 = O.get_primes(n, 50, 1)[0]
    mods = [q0] + _primes_next_to(12 * q0, logn, 15) + O.get_primes(n, 59, 2)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 2, 0)
    ref = O.RefContext(2, logn, mods, nsp=2, t=0, mode=0)
    ev = S.Evaluator(ctx)
    cl = SparseClient(ref, 32, seed=11)
    assert int(np.count_nonzero(cl.s)) == 32
    k_top, c2s_counts, s2c_counts = 16, [4, 4, 3], [6, 5]
    plan = ev.bootstrap_plan(k_top, c2s_counts, s2c_counts, K, r, d, n_baby=nb)
    assert (plan["c2s_out_level"], plan["evalmod_out_level"], plan["out_level"]) == (13, 4, 2)
    em = plan["evalmod"]
    assert plan["raise_scale"] == float(q0) * K
    assert plan["s2c_gain"] == float(q0) / (6.283185307179586476925286766559 * em["out_scale"])
    p1, p2 = ev.dft_plan(R.C2S, k_top, c2s_counts), ev.dft_plan(R.S2C, 4, s2c_counts)
    assert plan["key_steps"] == sorted(set(p1["key_steps"]) | set(p2["key_steps"])) and plan["needs_conjugation"] == 1
    # keys, made on the device
    rng = np.random.default_rng(77)
    nd = 8
    d_sk = ctx.upload(cl.sk)
    elts = sorted({H.elt_from_step(n, s) for s in plan["key_steps"]} | {2 * n - 1})
    seeds = rng.integers(0, 2**64, size=(len(elts), nd, 8), dtype=np.uint64, endpoint=False)
    noise = rng.integers(-6, 7, size=(len(elts), nd, n), dtype=np.int32)
    gk = dict(zip(elts, ctx.generate_galois_keys(d_sk, elts, seeds, ctx.upload_i32(noise))))
    rk = ctx.generate_relin_keys(d_sk, 1, rng.integers(0, 2**64, size=(1, nd, 8), dtype=np.uint64, endpoint=False),
                                 ctx.upload_i32(rng.integers(-6, 7, size=(1, nd, n), dtype=np.int32)))
    m = rng.integers(-(1 << 39), 1 << 39, size=n).astype(np.int64)
    low = np.ascontiguousarray(cl.encrypt_poly_ntt([int(v) for v in m])[:, :1])[None]  # (1, 2, 1, N): the q_0 rows
    # 1. ModRaise on the CPU: m + q_0 I
    raised = B.mod_raise(ref, low, k_top)
    dot = raised[0, 0].copy()
    for row in range(k_top):
        t = np.zeros(n, dtype=np.uint64)
        O.lib().ref_dyadic_product_coeffmod(O.ptr(np.ascontiguousarray(raised[0, 1, row])), O.ptr(cl.sk[row]), n,
                                            O.C.byref(ref.c.key_mod[row]), O.ptr(t))
        O.lib().ref_add_poly_coeffmod(O.ptr(dot[row]), O.ptr(t), n, O.C.byref(ref.c.key_mod[row]), O.ptr(dot[row]))
    c, _ = cl.centered_from_ntt_rows(dot)
    I = [(c[j] - int(m[j]) + q0 // 2) // q0 for j in range(n)]
    print("ModRaise: max|I| = %d, residual noise %d" % (max(abs(v) for v in I), max(abs(c[j] - int(m[j]) - q0 * I[j]) for j in range(n))))
    assert max(abs(v) for v in I) <= K - 1
    # 2. the device's bootstrap against the chain of the entries that existed before
    tables = S.BootstrapTables(ctx, k_top, c2s_counts, s2c_counts, K, r, d, n_baby=nb)
    out = ctx.alloc(2 * 2 * n)
    ev.bootstrap(tables, ctx.upload(low), 1, 1, gk, rk, out)
    got = out.download((2, 2, n))
    assert ctx.pool_stats()["bytes_in_use"] >= plan["temp_bytes_per_item"], "the tables hold the intermediates' block"
    t1 = S.DftTables(ctx, R.C2S, k_top, c2s_counts)
    t2 = S.DftTables(ctx, R.S2C, 4, s2c_counts, gain=plan["s2c_gain"])
    re, im = ctx.alloc(2 * 13 * n), ctx.alloc(2 * 13 * n)
    ev.coeffs_to_slots(t1, ctx.upload(raised), 1, gk, re, im)
    halves = []
    for half in (re, im):
        cur, lv = ctx.alloc(2 * em["poly_level"] * n), em["poly_level"]
        _, sc = ev.evaluate_polynomial_ckks(half, S.evalmod_coeffs(K, r, d), 13, 1, plan["raise_scale"], cur, relin_keys=rk,
                                            basis=1, n_baby=nb, scale_out=em["poly_scale_out"])
        for i in range(r):
            assert sc == em["scales"][i]
            nxt = ctx.upload(_three_entry_chain(S, ctx, ev, mods, lv, cur, 1, sc, rk, n))
            cur, lv, sc = nxt, lv - 1, B.double_angle_scale(sc, mods[lv - 1])
        assert (lv, sc) == (4, em["out_scale"])
        halves.append(cur)
    ref_out = ctx.alloc(2 * 2 * n)
    ev.slots_to_coeffs(t2, halves[0], halves[1], 1, gk, ref_out)
    assert np.array_equal(got, ref_out.download((2, 2, n))), "bootstrap differs from the chain of existing entries"
    # 3. the reference chain carries the message
    plain = ctx.alloc(2 * n)
    ctx.decrypt(ref_out, 2, 2, 1, ctx.upload(cl.sk_powers(1)), True, plain)
    vals, _ = cl.centered_from_ntt_rows(plain.download((2, n)))
    err = max(abs(int(vals[j]) - int(m[j])) for j in range(n)) / float(np.max(np.abs(m)))
    print("bootstrap: max coefficient error / max|m| = 2^%.2f" % np.log2(err))
    assert err < 2.0 ** -16, "the primes do not carry the reference chain"
    for t in (t1, t2, tables):
        t.free()
    assert ctx.pool_stats()["bytes_in_use"] == 0, "destroy releases the blocks"


# ------------------------------------------------------------------ 3. boundary behaviour
def test_checks_flags_capture(S):
    logn, n, k = 6, 64, 4
    mods = O.coeff_modulus_create(n, [40] * 5)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(3)
    count = 3
    rk = [S.KSwitchKeys(ctx, rows(rng, mods, n, (4, 2)))]
    ct = rows(rng, mods[:k], n, (count, 2))
    d_ct = ctx.upload(ct)
    up, down = ctx.alloc(count * 2 * 4 * n), ctx.alloc(count * 2 * (k - 1) * n)
    # ---- mod_raise: levels, overlap, alignment, the scheme
    for k_in, k_out in ((0, 2), (5, 2), (1, 1), (1, 0), (1, 5)):
        with pytest.raises(ValueError):
            ev.mod_raise(d_ct, k_in, count, k_out, up)
    with pytest.raises(ValueError, match="at least 2"):
        ev.mod_raise(d_ct, 1, count, 1, up)
    with pytest.raises(ValueError, match="overlap"):
        ev.mod_raise(d_ct, k, count, 4, d_ct)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ev.mod_raise(d_ct.ptr + 8, k, 1, 4, up)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ev.mod_raise(d_ct, k, 1, 4, up.ptr + 8)
    with pytest.raises(TypeError):
        ev.mod_raise(None, k, count, 4, up)
    with pytest.raises(TypeError):
        ev.mod_raise(d_ct, k, count, 4, None)
    bfv = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, mode=S.MODE_STRICT)
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).mod_raise(d_ct, k, count, 4, up)
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).double_angle(d_ct, k, count, 2.0 ** 30, rk, down)
    # ---- double_angle: the level, the scale, the keys, overlap
    for bad_k in (0, 1, 5):
        with pytest.raises(ValueError):
            ev.double_angle(d_ct, bad_k, count, 2.0 ** 30, rk, down)
    for bad_scale in (0.0, -1.0, float("inf"), float("nan"), 1e200):
        with pytest.raises(ValueError, match="scale out of bounds"):
            ev.double_angle(d_ct, k, count, bad_scale, rk, down)
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        ev.double_angle(d_ct, k, count, 2.0 ** 30, [], down)
    with pytest.raises(TypeError):
        ev.double_angle(d_ct, k, count, 2.0 ** 30, None, down)
    short = [S.KSwitchKeys(ctx, rows(rng, mods, n, (3, 2)))]
    with pytest.raises(ValueError, match="not valid for encryption parameters"):
        ev.double_angle(d_ct, k, count, 2.0 ** 30, short, down)
    with pytest.raises(ValueError, match="overlap"):
        ev.double_angle(d_ct, k, count, 2.0 ** 30, rk, d_ct)
    # ---- the empty batch launches nothing; a host-only context has no fallback
    ev.mod_raise(d_ct, k, 0, 4, up)
    assert ev.double_angle(d_ct, k, 0, 2.0 ** 30, rk, down) == 2.0 ** 60 / float(mods[k - 1])
    host = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0, device=-1)
    hev = S.Evaluator(host)
    with pytest.raises(ValueError, match="overlap"):
        hev.mod_raise(d_ct, k, count, 4, d_ct)
    hev.mod_raise(d_ct, k, 0, 4, up)
    with pytest.raises(S.LogicError):
        hev.mod_raise(d_ct, k, count, 4, up)
    # ---- transparency flags: one per output ciphertext
    flags = ctx.alloc(4)
    zeroed = ct.copy()
    zeroed[1] = 0
    d_z = ctx.upload(zeroed)
    ctx.transparency_sink(flags, 8)
    ev.mod_raise(d_z, k, count, 4, up)
    assert list(flags.download().view(np.uint32)[:count] != 0) == [True, False, True]
    ctx.memset_zero(flags, 32)
    ev.double_angle(d_z, k, count, 2.0 ** 30, rk, down)
    assert list(flags.download().view(np.uint32)[:count] != 0) == [True, False, True]
    with pytest.raises(ValueError, match="transparency sink"):
        ev.mod_raise(ctx.upload(rows(rng, mods[:1], n, (9, 2))), 1, 9, 2, ctx.alloc(9 * 2 * 2 * n))
    ctx.transparency_sink(None, 0)
    # ---- graph capture after one warm-up: a replay gives the eager words
    ev.mod_raise(d_ct, k, count, 4, up)
    ev.double_angle(d_ct, k, count, 2.0 ** 30, rk, down)
    want_up, want_down = up.download().copy(), down.download().copy()

    def both():
        ev.mod_raise(d_ct, k, count, 4, up)
        ev.double_angle(d_ct, k, count, 2.0 ** 30, rk, down)

    graph = ctx.capture(both)
    for buf in (up, down):
        ctx.memset_zero(buf, buf.words * 8)
    graph.launch()
    assert np.array_equal(up.download(), want_up) and np.array_equal(down.download(), want_down)


def test_cpp_adapter(tmp_path):
    """tests/host_adapter_bootstrap_check.cpp: the host-ciphertext and the DeviceCiphertext forms of mod_raise, double_angle,
    eval_mod and bootstrap give the C ABI's words on the same seeded inputs, at the plans' levels and scales; the operand
    checks and their messages"""
    exe = compile_cpp(tmp_path, "host_adapter_bootstrap_check.cpp", link_sealhip=True)
    q0 = O.get_primes(256, 40, 1)[0]
    mods = [q0] + _primes_next_to(2 * q0, 8, 9) + O.get_primes(256, 59, 1)
    assert "bootstrap adapter checks ok" in run_exe(exe, "0", *mods, timeout=120)
