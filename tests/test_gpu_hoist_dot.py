"""Plaintext-weighted sums of rotations on the device (sealhip_evaluator_apply_galois_dot_plain / _rotate_vector_dot_plain,
DESIGN.md section 16) against the CPU restatement of tests/hoist_dot_ref.py, word for word in the context's mode.

Shapes: as tests/test_gpu_hoist.py, the smallest that reach every path. N = 2^12 takes the tiled transforms, the explicit
mod-up and the moddown_pre / moddown_post back half; the gathered mod-up, the CKKS fold and BFV's deferred top layer exist
from N = 2^14, the fused mod-down store from 2^15: one three-prime case each. A lane of the inner product holds four
(ciphertext, sum) slots: four ciphertexts at one sum, two at two sums, one at three or more sums in groups of four -- so
eleven ciphertexts give a short last group at one sum and at two, and five sums a short last sum group. Seventeen digits take
the loop kernel; 22 elements with the identity at position 18 take two launches of the base kernel (16 + 6) and of the inner
product (16 + 5), the second adding into what the first left."""
import os
import sys

import numpy as np
import pytest

import hoist_dot_ref as HD
import hoist_ref as H
import oracle_lib as O
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe

pytestmark = pytest.mark.gpu


def _elts(n):
    return [H.elt_from_step(n, 1), 1, H.elt_from_step(n, -3), 2 * n - 1, 3]


class Session(BaseSession):
    """contexts on both sides and random keys: the word-for-word comparison needs no valid keys"""

    def __init__(self, S, scheme, logn, bits, nsp, mode, t=0, seed=0):
        super().__init__(S, scheme, logn, bits, nsp, mode, t, seed + logn + len(bits))
        self.keys = {}

    def key(self, g):
        if g == 1:
            return None, None
        if g not in self.keys:
            host = rows(self.rng, self.mods, self.n, (self.nd, 2))
            self.keys[g] = (host, self.S.KSwitchKeys(self.ctx, host))
        return self.keys[g]

    def compare(self, k, count, elts, n_sums, tag, items=None):
        n = self.n
        ct = rows(self.rng, self.mods[:k], n, (count, 2))
        plains = rows(self.rng, self.mods, n, (n_sums, len(elts)))
        d, dp = self.ctx.upload(ct), self.ctx.upload(plains)
        out = self.ctx.alloc(n_sums * count * 2 * k * n)
        keys = [self.key(g) for g in elts]
        self.ev.apply_galois_dot_plain(d, k, count, elts, [kk[1] for kk in keys], dp, n_sums, out)
        got = out.download((n_sums, count, 2, k, n))
        assert np.array_equal(d.download(ct.shape), ct), (tag, "the input was modified")
        assert np.array_equal(dp.download(plains.shape), plains), (tag, "the plaintexts were modified")
        want = HD.dot_plain(self.ref, k, ct, elts, [kk[0] for kk in keys], plains, items)
        for s in range(n_sums):
            for c in (range(count) if items is None else items):
                assert np.array_equal(got[s, c], want[s, c]), (tag, "sum", s, "item", c)
        for b in (d, dp, out):
            b.free()
        return ct, plains, got


@pytest.mark.parametrize("bits", [[40, 40, 40, 40], [55, 55, 56, 55]])
def test_ckks_parity_words(S, bits):
    """the FP64 and the integer transform instances; first level and a single digit; the identity in the middle of the list
    (both components of base)"""
    se = Session(S, S.SCHEME_CKKS, 12, bits, 1, S.MODE_PARITY)
    for k in (3, 1):
        se.compare(k, 3, _elts(se.n), 2, ("ckks", bits, k))


@pytest.mark.parametrize("mode", [0, 1])
def test_ckks_two_special_primes(S, mode):
    """five ciphertext primes in bundles of two: the last bundle is short; the special rows take the plaintext's rows
    n_key - 2 and n_key - 1 at every level"""
    se = Session(S, S.SCHEME_CKKS, 12, [40] * 5 + [41] * 2, 2, mode)
    for k in (5, 2):
        se.compare(k, 3, _elts(se.n), 2, ("ckks nsp 2", mode, k))


@pytest.mark.parametrize("logn", [12, 14])
def test_bfv_strict_words(S, logn):
    """coefficient-form ciphertexts: both components transformed, base transformed back; 2^14 has the deferred top layer"""
    se = Session(S, S.SCHEME_BFV, logn, [40, 40, 40, 41] if logn == 12 else [40, 40, 41], 1, S.MODE_STRICT, t=65537)
    k = 3 if logn == 12 else 2
    se.compare(k, 2, _elts(se.n)[:3], 2, ("bfv", logn))


@pytest.mark.parametrize("logn,mode", [(14, 0), (15, 0), (15, 1)])
def test_single_pass_transform_paths(S, logn, mode):
    """gathered mod-up and the CKKS fold (2^14), its fused mod-down store adding into base (2^15)"""
    se = Session(S, S.SCHEME_CKKS, logn, [40, 40, 41], 1, mode)
    se.compare(2, 2, _elts(se.n)[1:3], 1, ("single pass", logn, mode))


@pytest.mark.parametrize("count,n_sums", [(11, 1), (11, 2), (2, 5)])
def test_lane_slots(S, count, n_sums):
    """four ciphertexts per lane at one sum (11 = 4 + 4 + 3), two at two sums (a last group of one), one at five sums in
    sum groups of 4 + 1"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 41], 1, S.MODE_PARITY)
    se.compare(2, count, _elts(se.n)[:2], n_sums, ("slots", count, n_sums), items=(0, count - 2, count - 1))


def test_more_digits_than_kernel_instances(S):
    """seventeen digits: past the sixteen instances of the inner product, the per-lane loop kernel"""
    se = Session(S, S.SCHEME_CKKS, 12, [40] * 17 + [41], 1, S.MODE_PARITY)
    se.compare(17, 2, _elts(se.n)[:2], 2, "17 digits")


def test_more_elements_than_one_launch(S):
    """22 elements, the identity at position 18, one repeated: the second launch of each kernel adds into acc and base"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 41], 1, S.MODE_PARITY)
    elts = [2 * i + 3 for i in range(22)]
    elts[18] = 1
    elts[20] = elts[2]
    se.compare(2, 2, elts, 2, "22 elements")


def test_only_identity_elements(S):
    """out_s = sum_i W[s][i] (.) ct; with a single term the words of multiply_plain_ntt with the plaintext's leading k rows;
    nothing of the key switch is launched"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 2
    se.compare(k, count, [1, 1, 1], 2, "identities")
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    plain = rows(se.rng, se.mods, n, (1, 1))
    d, dp = ctx.upload(ct), ctx.upload(plain)
    out = ctx.alloc(count * 2 * k * n)
    ctx.profile_enable(True)
    ev.apply_galois_dot_plain(d, k, count, [1], [None], dp, 1, out)
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    assert set(prof) == {"hoist_dot_base"}, prof
    lead = ctx.upload(plain[0, 0, :k])
    ev.multiply_plain_inplace(d, 2, k, count, lead)
    assert np.array_equal(out.download(), d.download())


def test_one_decomposition_and_one_mod_down_per_sum(S):
    """n_sums = 2, four elements: the digits are formed as often as for ONE apply_galois of the batch, and the mod-down runs
    over two ciphertext batches, not eight. apply_galois_many with two elements is exactly that much transform work -- one
    decomposition and two mod-downs of the same batch -- so the transformed rows of every NTT kernel and the launches of the
    mod-up and mod-down kernels must equal its; with eight mod-downs the row counts would be those of eight elements."""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 3
    elts = _elts(n)[2:] + [5] + [7, 9, 11, 13]
    keys = [se.key(g)[1] for g in elts]
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    plains = rows(se.rng, se.mods, n, (2, 4))
    d, dp = ctx.upload(ct), ctx.upload(plains)
    out = ctx.alloc(8 * count * 2 * k * n)
    ev.apply_galois_many(d, k, count, elts, keys, out)  # (tables resident)

    def profile(fn):
        ctx.profile_enable(True)
        fn()
        prof = ctx.profile_fetch()
        ctx.profile_enable(False)
        return prof

    def transforms(prof):
        return {tag: v["units"] for tag, v in prof.items() if tag.startswith("ntt_")}

    dot = profile(lambda: ev.apply_galois_dot_plain(d, k, count, elts[:4], keys[:4], dp, 2, out))
    two = profile(lambda: ev.apply_galois_many(d, k, count, elts[:2], keys[:2], out))
    eight = profile(lambda: ev.apply_galois_many(d, k, count, elts, keys, out))
    one = profile(lambda: ev.apply_galois_inplace(d, k, count, elts[0], keys[0]))
    assert transforms(dot) == transforms(two) and transforms(dot) != transforms(eight), (dot, two, eight)
    assert dot["ks_modup"]["launches"] == one["ks_modup"]["launches"], (dot, one)
    for tag in two:
        if tag.startswith("ks_moddown"):
            assert dot[tag]["launches"] == two[tag]["launches"], (tag, dot, two)
    assert dot["hoist_dot_mac"]["launches"] == 1 and dot["hoist_dot_base"]["launches"] == 1, dot
    assert "hoist_mac" not in dot and "ks_mac" not in dot and "hoist_galois" not in dot, dot


def test_refusals(S):
    """BFV in PARITY mode; a bad element; a short key; a NULL key for an element other than 1; overlap of out with ct and
    with plain_ntt; an empty sum. Each leaves input and output untouched."""
    logn, n = 12, 1 << 12
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    rng = np.random.default_rng(1)
    k, count = 3, 1
    key = rows(rng, mods, n, (3, 2))
    for scheme, mode, t in ((S.SCHEME_BFV, S.MODE_PARITY, 65537), (S.SCHEME_CKKS, S.MODE_PARITY, 0)):
        ctx = S.Context(scheme, logn, mods, 1, t, mode=mode)
        ev = S.Evaluator(ctx)
        dkey, short = S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, key[:2])
        ct = rows(rng, mods[:k], n, (count, 2))
        plains = rows(rng, mods, n, (2, 2))
        d, dp = ctx.upload(ct), ctx.upload(plains)
        out = ctx.alloc(2 * count * 2 * k * n)
        sentinel = np.full(out.words, 7, dtype=np.uint64)
        out.upload(sentinel)
        if scheme == S.SCHEME_BFV:
            with pytest.raises(ValueError, match="STRICT"):
                ev.apply_galois_dot_plain(d, k, count, [3, 1], [dkey, None], dp, 2, out)
            with pytest.raises(ValueError, match="STRICT"):
                ev.rotate_vector_dot_plain(d, k, count, [1, 0], {H.elt_from_step(n, 1): dkey}, dp, 2, out)
        else:
            for bad in (4, 2 * n, 2 * n + 1, 0):
                with pytest.raises(ValueError, match="Galois element is not valid"):
                    ev.apply_galois_dot_plain(d, k, count, [3, bad], [dkey, dkey], dp, 2, out)
            with pytest.raises(ValueError, match="kswitch_keys is not valid"):
                ev.apply_galois_dot_plain(d, k, count, [3, 5], [dkey, short], dp, 2, out)
            with pytest.raises(TypeError):
                ev.apply_galois_dot_plain(d, k, count, [1, 5], [dkey, None], dp, 2, out)
            with pytest.raises(ValueError, match="Galois key not present"):
                ev.rotate_vector_dot_plain(d, k, count, [0, 1], {3: dkey}, dp, 2, out)
            for n_sums, elts in ((0, [3, 5]), (2, [])):
                with pytest.raises(ValueError, match="empty sum"):
                    ev.apply_galois_dot_plain(d, k, count, elts, [dkey] * len(elts), dp, n_sums, out)
            with pytest.raises(ValueError, match="overlap ct"):
                ev.apply_galois_dot_plain(d, k, count, [3], [dkey], dp, 1, d)
            with pytest.raises(ValueError, match="overlap ct"):
                ev.apply_galois_dot_plain(d.ptr + 8 * k * n, k, count, [3, 5], [dkey, dkey], dp, 1, d)
            with pytest.raises(ValueError, match="overlap plain_ntt"):
                ev.apply_galois_dot_plain(d, k, count, [3, 5], [dkey, dkey], dp, 2, dp.ptr + 8 * 3 * 4 * n)
            ev.apply_galois_dot_plain(d, 2, count, [3, 5], [dkey, short], dp, 2, out)  # (two digits are enough one level below)
            out.upload(sentinel)
        assert np.array_equal(out.download(), sentinel) and np.array_equal(d.download(ct.shape), ct)
        assert np.array_equal(dp.download(plains.shape), plains)


def test_transparency_flags_in_output_order(S):
    """a ciphertext with c1 = 0 is flagged under every sum: one flag per output, sum-major; identity-only sums included; a
    sink that is too small is refused"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 3
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    ct[1, 1] = 0
    d = ctx.upload(ct)
    e1, e2 = H.elt_from_step(n, 1), H.elt_from_step(n, -2)
    dkeys = [se.key(e1)[1], se.key(e2)[1]]
    dp = ctx.upload(rows(se.rng, se.mods, n, (2, 2)))
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        out = ctx.alloc(2 * count * 2 * k * n)
        for elts, keys in (([e1, e2], dkeys), ([1, 1], [None, None])):
            flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
            ev.apply_galois_dot_plain(d, k, count, elts, keys, dp, 2, out)
            got = flags.download().view(np.uint32)
            assert (got[:6] != 0).tolist() == [True, False, True] * 2 and np.all(got[6:] == 5), (elts, got)
        ev.apply_galois_dot_plain(d, k, count, [e1, e2], dkeys, dp, 2, out)
        with_sink = out.download().copy()
        ctx.transparency_sink(flags, 5)
        with pytest.raises(ValueError, match="sink"):
            ev.apply_galois_dot_plain(d, k, count, [e1, e2], dkeys, dp, 2, out)
    finally:
        ctx.transparency_sink(None, 0)
    ev.apply_galois_dot_plain(d, k, count, [e1, e2], dkeys, dp, 2, out)
    assert np.array_equal(out.download(), with_sink)


def test_graph_capture(S):
    """warm the Galois tables, capture one call, replay it twice on new inputs: the words of the restatement"""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 2
    elts = _elts(n)[:3]
    keys = [se.key(g) for g in elts]
    d = ctx.upload(rows(se.rng, se.mods[:k], n, (count, 2)))
    dp = ctx.upload(rows(se.rng, se.mods, n, (2, 3)))
    out = ctx.alloc(2 * count * 2 * k * n)
    g = ctx.capture(lambda: ev.apply_galois_dot_plain(d, k, count, elts, [kk[1] for kk in keys], dp, 2, out))
    for _ in range(2):
        ct = rows(se.rng, se.mods[:k], n, (count, 2))
        plains = rows(se.rng, se.mods, n, (2, 3))
        d.upload(ct)
        dp.upload(plains)
        g.launch()
        got = out.download((2, count, 2, k, n))
        assert np.array_equal(got, HD.dot_plain(se.ref, k, ct, elts, [kk[0] for kk in keys], plains))


def test_key_level_plaintexts_and_a_matrix_vector_product(S):
    """BFV STRICT, N = 2^12, t = 65537, real keys: a 16 x 16 matrix times a vector replicated along the batching rows, by
    baby-step/giant-step with 4 x 4 diagonals. The pre-rotated diagonals are batch-encoded and lifted with
    transform_plain_to_ntt at k = n_key (the key level stays admitted); ONE rotate_vector_dot_plain with steps {0, 1, 2, 3}
    and n_sums = 4 forms the inner sums, the existing apply_galois and add the outer one. Every slot decrypts to M v mod t,
    and every inner sum has at least the noise budget of the composition (rotate_vector_many, multiply_plain, add) minus
    one bit: the floor of a log2 of terms with the same bound."""
    logn, n, t, dim, bs = 12, 1 << 12, 65537, 16, 4
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    n_key = len(mods)
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT)
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    cl = O.Client(ref, seed=12)
    ev = S.Evaluator(ctx)
    k = cl.k
    rng = np.random.default_rng(12)
    M = rng.integers(0, t, size=(dim, dim), dtype=np.uint64)
    v = rng.integers(0, t, size=dim, dtype=np.uint64)
    # The vector index of every slot. The batch encoder orders the slots of a row by powers of 3 (batchencoder.cpp:77), the
    # Galois tool steps by powers of 5 (galois.h:169), and 5 = -3^s0 mod 2N: a rotation by one step moves a row by s0 slots of
    # the encoder's order and swaps the two rows. s0 is odd, so slot j of either row gets index j / s0 mod N/2, reduced mod
    # 16: a step then advances the index by one, and the swap does not show because both rows are labelled alike.
    half, e1 = n // 2, H.elt_from_step(n, 1)
    s0 = next(s for s in range(half) if pow(3, s, 2 * n) in (e1, 2 * n - e1))
    slot = ((np.arange(n) % half) * pow(s0, -1, half) % half) % dim

    def encode(values):
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, n)
        plain = ctx.alloc(values.shape[0] * n)
        ctx.batch_encode(ctx.upload(values), n, values.shape[0], plain)
        return plain

    ct = ctx.upload(cl.encrypt_bfv(encode(v[slot]).download()))
    # W[g][b] = diagonal 4g + b rotated right by 4g: slot i holds M[i - 4g][i + b]
    diag = np.empty((bs, bs, n), dtype=np.uint64)
    for g in range(bs):
        for b in range(bs):
            diag[g, b] = M[(slot - bs * g) % dim, (slot + b) % dim]
    coeffs = encode(diag)
    plains = ctx.alloc(bs * bs * n_key * n)
    ev.transform_plain_to_ntt(coeffs, n, n_key, bs * bs, plains)
    steps = list(range(bs)) + [bs * g for g in range(1, bs)]
    gk = {H.elt_from_step(n, st): S.KSwitchKeys(ctx, cl.galois_key(H.elt_from_step(n, st))) for st in steps if st}
    inner = ctx.alloc(bs * 2 * k * n)
    ev.rotate_vector_dot_plain(ct, k, 1, list(range(bs)), gk, plains, bs, inner)
    sk = ctx.upload(cl.sk_powers(1))
    fused = ctx.invariant_noise_budget(inner, 2, k, bs, sk)
    # the composition on the same inputs
    rots = ctx.alloc(bs * 2 * k * n)
    ev.rotate_vector_many(ct, k, 1, list(range(bs)), gk, rots)
    rot_host = rots.download((bs, 2, k, n))
    coeff_host = coeffs.download((bs, bs, n))
    composed = np.empty(bs, dtype=np.int64)
    for g in range(bs):
        total = None
        for b in range(bs):
            term = ctx.upload(rot_host[b])
            ev.multiply_plain_inplace(term, 2, k, 1, ctx.upload(coeff_host[g, b]), ntt_form=False)
            if total is None:
                total = term
            else:
                nxt = ctx.alloc(2 * k * n)
                ev.add(total, 2, term, 2, k, 1, nxt)
                total = nxt
        composed[g] = ctx.invariant_noise_budget(total, 2, k, 1, sk)[0]
    print("matvec inner sums, noise budgets: fused %s composed %s" % (fused.tolist(), composed.tolist()))
    assert np.all(fused >= composed - 1), (fused, composed)
    # the giant steps
    inner_host = inner.download((bs, 2, k, n))
    result = ctx.upload(inner_host[0])
    for g in range(1, bs):
        term = ctx.upload(inner_host[g])
        ev.apply_galois_inplace(term, k, 1, H.elt_from_step(n, bs * g), gk[H.elt_from_step(n, bs * g)])
        nxt = ctx.alloc(2 * k * n)
        ev.add(result, 2, term, 2, k, 1, nxt)
        result = nxt
    plain = ctx.alloc(n)
    ctx.decrypt(result, 2, k, 1, sk, False, plain)
    values = ctx.alloc(n)
    ctx.batch_decode(plain, 1, values)
    want = np.array([sum(int(M[i, j]) * int(v[j]) for j in range(dim)) % t for i in range(dim)], dtype=np.uint64)
    assert np.array_equal(values.download(), want[slot])


def test_ckks_key_level_encoding_agrees_with_the_level_encoding(S):
    """The CKKS road to a key-level plaintext: sealhip_ckks_encode at k = n_key. With a single identity element the result
    equals multiply_plain_ntt with the level-k encoding's words only where the two encodings agree on the rows below k --
    they do (one integer polynomial, reduced modulo each prime), which is asserted here first."""
    se = Session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 2, 2
    n_key = len(se.mods)
    values = (se.rng.standard_normal((1, n // 2)) + 1j * se.rng.standard_normal((1, n // 2))) * 8
    at_key = ctx.ckks_encode(values, n_key, 2.0 ** 30)
    at_k = ctx.ckks_encode(values, k, 2.0 ** 30)
    assert np.array_equal(at_key.download((n_key, n))[:k], at_k.download((k, n)))
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    d = ctx.upload(ct)
    out = ctx.alloc(count * 2 * k * n)
    ev.apply_galois_dot_plain(d, k, count, [1], [None], at_key, 1, out)
    ev.multiply_plain_inplace(d, 2, k, count, at_k)
    assert np.array_equal(out.download(), d.download())


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_hoist_dot_check.cpp: the host-ciphertext and the DeviceCiphertext / DevicePlaintext overloads give
    the ABI's words on the same seeded inputs, with the operand's level and the product of the scales; a warm resident call
    takes every block from the pool; the deferred transparency exception arrives"""
    logn, n, k, n_sums = 12, 1 << 12, 3, 2
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_hoist_dot_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    sm = O.SplitMix(0x4016)
    ct = sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n)
    keys = [sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n) for _ in range(2)]
    plains = sm.fill(n_sums * 3 * 4, n, mods * (n_sums * 3)).reshape(n_sums, 3, 4, n)
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    e1, e2 = H.elt_from_step(n, 1), H.elt_from_step(n, -2)
    dkeys = [S.KSwitchKeys(ctx, key) for key in keys]
    d, dp = ctx.upload(ct), ctx.upload(plains)
    by_elt = ctx.alloc(n_sums * 2 * k * n)
    ev.apply_galois_dot_plain(d, k, 1, [e1, 1, e2], [dkeys[0], None, dkeys[1]], dp, n_sums, by_elt)
    by_step = ctx.alloc(n_sums * 2 * k * n)
    ev.rotate_vector_dot_plain(d, k, 1, [1, 0, -2], {e1: dkeys[0], e2: dkeys[1]}, dp, n_sums, by_step)
    for name, buf in (("apply_galois_dot_plain", by_elt), ("rotate_vector_dot_plain", by_step)):
        for side in ("host", "device"):
            line = "%s %s digest %016x count %d meta 1" % (side, name, O.fnv(buf.download()), n_sums)
            assert line in stdout, (line, stdout)
    assert "warm call pool mallocs 0 frees 0" in stdout, stdout
    assert "deferred transparency ok" in stdout, stdout


# ---------------------------------------------------------------- arena chunks (a child process with the smallest arena)
LOGN, N = 13, 1 << 13


def _child():
    """N = 2^13, 8 + 1 primes, k = 8, CKKS. The arena rule of DESIGN.md section 16: per item the digits once, w_coeff + w_ext
    = (8 + 8 * 9) N words = 5 MiB, and per sum w_prod + w_temp = (18 + 16) N words = 2.125 MiB. Two sums: 9.25 MiB per item,
    6 items in 64 MiB, so 7 items need a second, ragged chunk (one back half per sum there). 28 sums: 64.5 MiB for one item,
    so the sum list is split 27 + 1 with the digits kept, and the chunk is a single item."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    mods = O.coeff_modulus_create(N, [50] * 8 + [60])
    ctx = S.Context(S.SCHEME_CKKS, LOGN, mods, 1, 0)
    ref = O.RefContext(2, LOGN, mods, nsp=1)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(64)
    k = 8
    budget = int(ARENA_MB) << 20
    base, per_sum = (k + k * (k + 1)) * N * 8, (2 * (k + 1) + 2 * k) * N * 8

    def run(count, elts, n_sums, items, sums):
        keys = [None if g == 1 else rows(rng, mods, N, (8, 2)) for g in elts]
        dkeys = [None if key is None else S.KSwitchKeys(ctx, key) for key in keys]
        ct = rows(rng, mods[:k], N, (count, 2))
        plains = rows(rng, mods, N, (n_sums, len(elts)))
        d, dp = ctx.upload(ct), ctx.upload(plains)
        out = ctx.alloc(n_sums * count * 2 * k * N)
        ctx.chunk_log()
        ev.apply_galois_dot_plain(d, k, count, elts, dkeys, dp, n_sums, out)
        log = ctx.chunk_log()
        got = out.download((n_sums, count, 2, k, N))
        want = HD.dot_plain(ref, k, ct, elts, keys, plains[list(sums)], items)
        for j, s in enumerate(sums):
            for c in items:
                assert np.array_equal(got[s, c], want[j, c]), (n_sums, s, c)
        return log

    per_chunk = budget // (base + 2 * per_sum)
    assert per_chunk == 6
    log = run(7, [3, 1, 5], 2, (0, 5, 6), (0, 1))
    assert log == [(7, per_chunk)], log                   # a second, ragged item chunk; the sum list whole
    n_sums = 28
    assert base + n_sums * per_sum > budget
    per_pass = (budget - base) // per_sum
    assert per_pass == 27
    log = run(2, [3], n_sums, (0, 1), (0, 26, 27))
    assert log == [(n_sums, per_pass), (2, 1)], log       # the sum list split 27 + 1, one item per chunk
    print("HOIST_DOT_CHUNKS_OK")


def test_chunked_items_and_split_sum_list():
    run_arena_child(__file__, "HOIST_DOT_CHUNKS_OK", timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
