"""CKKS bootstrapping on the device: what a batch of one cannot show, and the refusals of
sealhip_evaluator_bootstrap and sealhip_evaluator_eval_mod through the ABI.

1. bootstrap at count = 3 after a count = 1 call on the same tables, word for word against single calls (which
   tests/test_gpu_bootstrap.py ties to the chain of existing entries): CoeffToSlot's out_re and out_im sit contiguously over
   `count` items and EvalMod runs once over 2 count of them, so an indexing mistake there coincides with the right answer at
   count = 1. The input has k_in = 2, so that the item stride differs from what is read. The pool holds both blocks until
   destroy. One flag per output ciphertext, with the sink sized for exactly `count`: the words behind it keep their
   sentinel, so the 2 count intermediates of EvalMod did not write flags. The same for eval_mod alone.
2. Every refusal the header names for bootstrap and eval_mod, the empty batch on a device, host-only contexts.
3. double_angle with 61-bit data primes: square_affine_kernel's 128-bit values at their bound.
N = 2^8 with random keys: the words do not depend on the keys being real."""
import numpy as np
import pytest

import hoist_ref as H
import oracle_lib as O
from test_gpu_bootstrap import _primes_next_to, _three_entry_chain
from support import S, rows

pytestmark = pytest.mark.gpu

LOGN, N = 8, 256
K_TOP, STAGES, K, R, D = 11, [4, 3], 2, 2, 7
SENTINEL = 0xA5A5A5A5


class _Session:
    """q_0 of 40 bits, ten primes next to 2 q_0, one 59-bit special prime: ModRaise to level 11, CoeffToSlot [4,3] to 9,
    EvalMod (K 2, r 2, degree 7) to 3, SlotToCoeff [4,3] to 1. Random keys for the plan's steps. (Not a BaseSession: the
    primes are picked one by one and there is no oracle side.)"""

    def __init__(self, S):
        q0 = O.get_primes(N, 40, 1)[0]
        self.mods = [q0] + _primes_next_to(2 * q0, LOGN, 10) + O.get_primes(N, 59, 1)
        self.ctx = S.Context(S.SCHEME_CKKS, LOGN, self.mods, 1, 0)
        self.ev = S.Evaluator(self.ctx)
        self.plan = self.ev.bootstrap_plan(K_TOP, STAGES, STAGES, K, R, D)
        assert (self.plan["c2s_out_level"], self.plan["evalmod_out_level"], self.plan["out_level"]) == (9, 3, 1)
        self.rng = np.random.default_rng(2024)
        self.nd = K_TOP
        self.elts = sorted({H.elt_from_step(N, s) for s in self.plan["key_steps"]} | {2 * N - 1})
        self.gk = {g: self.key(self.ctx) for g in self.elts}
        self.rk = [self.key(self.ctx)]

    def key(self, ctx, digits=None):
        import sealhip

        return sealhip.KSwitchKeys(ctx, rows(self.rng, self.mods, N, (digits or self.nd, 2)))


@pytest.fixture(scope="module")
def se(S):
    return _Session(S)


def _flags(buf, count):
    words = buf.download().view(np.uint32)
    assert np.all(words[count:] == SENTINEL), "flags were written behind the batch's"
    return list(words[:count] != 0)


def _sentinels(ctx, words):
    return ctx.upload(np.full(words, SENTINEL | (SENTINEL << 32), dtype=np.uint64))


def test_bootstrap_batch_words_flags_pool(S, se):
    ctx, ev, per_item = se.ctx, se.ev, se.plan["temp_bytes_per_item"]
    assert ctx.pool_stats()["bytes_in_use"] == 0
    count, k_in = 3, 2
    ct = rows(se.rng, se.mods[:k_in], N, (count, 2))
    ct[1] = 0  # a transparent item: it stays one through every part
    tables = S.BootstrapTables(ctx, K_TOP, STAGES, STAGES, K, R, D)
    assert ctx.pool_stats()["bytes_in_use"] == 0, "the block is taken on first use"

    def single(i):
        out = ctx.alloc(2 * N)
        ev.bootstrap(tables, ctx.upload(ct[i:i + 1]), k_in, 1, se.gk, se.rk, out)
        return out.download((2, 1, N))

    first = single(0)
    held_1 = ctx.pool_stats()["bytes_in_use"]
    assert held_1 >= per_item
    flags = _sentinels(ctx, 4)
    ctx.transparency_sink(flags, count)
    try:
        out = ctx.alloc(count * 2 * N)
        ev.bootstrap(tables, ctx.upload(ct), k_in, count, se.gk, se.rk, out)
        got = out.download((count, 2, 1, N))
        assert _flags(flags, count) == [True, False, True]
        with pytest.raises(ValueError, match="transparency sink"):
            ev.bootstrap(tables, ctx.upload(rows(se.rng, se.mods[:1], N, (4, 2))), 1, 4, se.gk, se.rk, ctx.alloc(4 * 2 * N))
    finally:
        ctx.transparency_sink(None, 0)
    held_3 = ctx.pool_stats()["bytes_in_use"]
    assert held_3 >= held_1 + count * per_item, "a larger batch takes a larger block, the earlier one stays held"
    want = np.stack([first, single(1), single(2)])
    assert ctx.pool_stats()["bytes_in_use"] == held_3, "a smaller batch fits the block that is there"
    assert np.array_equal(got, want), "a batch differs from its items bootstrapped one by one"
    assert not got[1, 1].any() and got[0, 1].any()
    tables.free()
    assert ctx.pool_stats()["bytes_in_use"] == 0, "destroy releases all the blocks"


def test_eval_mod_flags(S, se):
    ctx, ev, k, count = se.ctx, se.ev, 9, 3
    ct = rows(se.rng, se.mods[:k], N, (count, 2))
    ct[1] = 0
    plan = ev.evalmod_plan(k, se.plan["raise_scale"], K, R, D)
    assert plan["out_level"] == 3
    flags = _sentinels(ctx, 4)
    out = ctx.alloc(count * 2 * 3 * N)
    ctx.transparency_sink(flags, count)
    try:
        ev.eval_mod(ctx.upload(ct), k, count, se.plan["raise_scale"], K, R, D, se.rk, out)
        assert _flags(flags, count) == [True, False, True]
        with pytest.raises(ValueError, match="transparency sink"):
            ev.eval_mod(ctx.upload(rows(se.rng, se.mods[:k], N, (4, 2))), k, 4, se.plan["raise_scale"], K, R, D, se.rk,
                        ctx.alloc(4 * 2 * 3 * N))
    finally:
        ctx.transparency_sink(None, 0)
    assert ctx.pool_stats()["bytes_in_use"] == 0


def test_bootstrap_refusals(S, se):
    ctx, ev, gk, rk = se.ctx, se.ev, se.gk, se.rk
    count, k_in = 2, 2
    ct = rows(se.rng, se.mods[:k_in], N, (count, 2))
    d_ct, out = ctx.upload(ct), ctx.alloc(count * 2 * N)
    tables = S.BootstrapTables(ctx, K_TOP, STAGES, STAGES, K, R, D)
    # ---- NULL pointers
    for bad in ((tables, None, out), (tables, d_ct, None)):
        with pytest.raises(TypeError):
            ev.bootstrap(bad[0], bad[1], k_in, count, gk, rk, bad[2])
    gone = S.BootstrapTables(ctx, K_TOP, STAGES, STAGES, K, R, D)
    gone.free()
    with pytest.raises(TypeError):
        ev.bootstrap(gone, d_ct, k_in, count, gk, rk, out)
    # ---- tables of another context: a second device context, and a host-only one (which cannot make tables at all)
    other = S.Context(S.SCHEME_CKKS, LOGN, se.mods, 1, 0)
    host = S.Context(S.SCHEME_CKKS, LOGN, se.mods, 1, 0, device=-1)
    for foreign in (other, host):
        for n_items in (count, 0):
            with pytest.raises(ValueError, match="another context"):
                S.Evaluator(foreign).bootstrap(tables, d_ct, k_in, n_items, gk, rk, out)
    with pytest.raises(S.LogicError):
        S.BootstrapTables(host, K_TOP, STAGES, STAGES, K, R, D)
    assert S.Evaluator(host).bootstrap_plan(K_TOP, STAGES, STAGES, K, R, D) == se.plan, "the plan needs no device"
    # ---- the level, the alignment, overlap
    for bad_k in (0, 12):
        with pytest.raises(ValueError):
            ev.bootstrap(tables, d_ct, bad_k, count, gk, rk, out)
    with pytest.raises(ValueError, match="ct must be 16-byte aligned"):
        ev.bootstrap(tables, d_ct.ptr + 8, k_in, 1, gk, rk, out)
    with pytest.raises(ValueError, match="out must be 16-byte aligned"):
        ev.bootstrap(tables, d_ct, k_in, 1, gk, rk, out.ptr + 8)
    with pytest.raises(ValueError, match="overlap"):
        ev.bootstrap(tables, d_ct, k_in, count, gk, rk, d_ct)
    with pytest.raises(ValueError, match="overlap"):
        ev.bootstrap(tables, d_ct, k_in, count, gk, rk, d_ct.ptr + 16 * N)
    # ---- Galois keys: a rotation step's and the conjugation's absent, one with too few digits
    conj = 2 * N - 1
    step = next(g for g in se.elts if g != conj)
    for missing in (step, conj):
        with pytest.raises(ValueError, match="Galois key not present"):
            ev.bootstrap(tables, d_ct, k_in, count, {g: v for g, v in gk.items() if g != missing}, rk, out)
    short = se.key(ctx, digits=1)  # every stage, the conjugation and the squarings run at level 2 or above
    for g in (step, conj):
        with pytest.raises(ValueError, match="not valid for encryption parameters"):
            ev.bootstrap(tables, d_ct, k_in, count, {**gk, g: short}, rk, out)
    # ---- relinearization keys: none, an empty list, too few digits
    for none in (None, []):
        with pytest.raises(ValueError, match="not enough relinearization keys"):
            ev.bootstrap(tables, d_ct, k_in, count, gk, none, out)
    with pytest.raises(ValueError, match="not valid for encryption parameters"):
        ev.bootstrap(tables, d_ct, k_in, count, gk, [short], out)
    # ---- a refused call and the empty batch launch nothing and take no block
    marker = np.arange(count * 2 * N, dtype=np.uint64)
    out.upload(marker)
    ev.bootstrap(tables, d_ct, k_in, 0, gk, rk, out)
    assert np.array_equal(out.download(), marker) and np.array_equal(d_ct.download().reshape(ct.shape), ct)
    assert ctx.pool_stats()["bytes_in_use"] == 0
    tables.free()


def test_eval_mod_refusals(S, se):
    ctx, ev, rk, k, count = se.ctx, se.ev, se.rk, 9, 2
    s_x = se.plan["raise_scale"]
    d_ct, out = ctx.upload(rows(se.rng, se.mods[:k], N, (count, 2))), ctx.alloc(count * 2 * 3 * N)
    with pytest.raises(TypeError):
        ev.eval_mod(None, k, count, s_x, K, R, D, rk, out)
    with pytest.raises(TypeError):
        ev.eval_mod(d_ct, k, count, s_x, K, R, D, rk, None)
    for bad_k in (0, 12):
        with pytest.raises(ValueError):
            ev.eval_mod(d_ct, bad_k, count, s_x, K, R, D, rk, out)
    with pytest.raises(ValueError, match="K must be at least 1"):
        ev.eval_mod(d_ct, k, count, s_x, 0, R, D, rk, out)
    with pytest.raises(ValueError, match="r must be at most 8"):
        ev.eval_mod(d_ct, k, count, s_x, K, 9, D, rk, out)
    with pytest.raises(ValueError, match="end of modulus switching chain"):
        ev.eval_mod(d_ct, k, count, s_x, K, 6, D, rk, out)
    with pytest.raises(ValueError, match="scale out of bounds"):
        ev.eval_mod(d_ct, k, count, 2.0 ** 63, K, R, D, rk, out)  # 41-bit primes under it: s_r is not below 2^62
    for none in (None, []):
        with pytest.raises(ValueError, match="not enough relinearization keys"):
            ev.eval_mod(d_ct, k, count, s_x, K, R, D, none, out)
    with pytest.raises(ValueError, match="not valid for encryption parameters"):
        ev.eval_mod(d_ct, k, count, s_x, K, R, D, [se.key(ctx, digits=1)], out)
    with pytest.raises(ValueError, match="overlap"):
        ev.eval_mod(d_ct, k, count, s_x, K, R, D, rk, d_ct)
    with pytest.raises(ValueError, match="CKKS only"):
        bfv = S.Context(S.SCHEME_BFV, LOGN, se.mods, 1, 65537, mode=S.MODE_STRICT)
        S.Evaluator(bfv).eval_mod(d_ct, k, count, s_x, K, R, D, rk, out)
    # ---- the empty batch: the plan's level and scale, nothing launched; a host-only context has no fallback
    marker = np.arange(count * 2 * 3 * N, dtype=np.uint64)
    out.upload(marker)
    plan = ev.evalmod_plan(k, s_x, K, R, D)
    assert ev.eval_mod(d_ct, k, 0, s_x, K, R, D, rk, out) == (plan["out_level"], plan["out_scale"])
    assert np.array_equal(out.download(), marker)
    host = S.Context(S.SCHEME_CKKS, LOGN, se.mods, 1, 0, device=-1)
    hev = S.Evaluator(host)
    assert hev.eval_mod(d_ct, k, 0, s_x, K, R, D, rk, out) == (plan["out_level"], plan["out_scale"])
    with pytest.raises(ValueError, match="overlap"):
        hev.eval_mod(d_ct, k, count, s_x, K, R, D, rk, d_ct)
    with pytest.raises(S.LogicError):
        hev.eval_mod(d_ct, k, count, s_x, K, R, D, rk, out)
    assert ctx.pool_stats()["bytes_in_use"] == 0


def test_double_angle_alignment(S, se):
    """square_affine_kernel loads ct two words at a time: the entry refuses a ct that is not 16-byte aligned"""
    ctx, ev, k = se.ctx, se.ev, 3
    d_ct, out = ctx.upload(rows(se.rng, se.mods[:k], N, (2, 2))), ctx.alloc(2 * 2 * N)
    with pytest.raises(ValueError, match="ct must be 16-byte aligned"):
        ev.double_angle(d_ct.ptr + 8, k, 1, 2.0 ** 40, se.rk, out)
    with pytest.raises(ValueError, match="ct must be 16-byte aligned"):
        S.Evaluator(S.Context(S.SCHEME_CKKS, LOGN, se.mods, 1, 0, device=-1)).double_angle(d_ct.ptr + 8, k, 1, 2.0 ** 40,
                                                                                          se.rk, out)


@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
def test_double_angle_words_61_bit_primes(S, mode):
    """three data primes just below 2^61 and a 60-bit special prime at N = 2^12, level 3 to 2: every 128-bit value of
    square_affine_kernel (2 a_0^2 + C, 4 a_0 a_1, 2 a_1^2) is at its bound of 2^124 before its one reduction"""
    logn, n, k = 12, 1 << 12, 3
    data = O.ntt_primes_around(1 << 61, logn)[0]
    assert len(data) == 3 and all(p.bit_length() == 61 for p in data)
    mods = data + O.get_primes(n, 60, 1)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0, mode=mode)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(61)
    rk = [S.KSwitchKeys(ctx, rows(rng, mods, n, (3, 2)))]
    for count in (1, 5):
        ct = rows(rng, mods[:k], n, (count, 2))
        ct[0, :, :, :4] = np.array([p - 1 for p in data], dtype=np.uint64)[None, :, None]  # the largest residues
        for scale in (2.0 ** 40, 2.0 ** 53.6):
            d_ct, d_out = ctx.upload(ct), ctx.alloc(count * 2 * (k - 1) * n)
            out_scale = ev.double_angle(d_ct, k, count, scale, rk, d_out)
            assert out_scale == scale * scale / float(mods[k - 1])
            want = _three_entry_chain(S, ctx, ev, mods, k, d_ct, count, scale, rk, n)
            assert np.array_equal(d_out.download(), want), (count, scale)
