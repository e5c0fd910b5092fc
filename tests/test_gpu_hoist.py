"""Hoisted rotation on the device (sealhip_evaluator_apply_galois_many / _rotate_vector_many) against
the CPU restatement of tests/hoist_ref.py, word for word in the context's mode.

Shapes: the smallest that reach every path. N = 2^12 takes the tiled transforms, the explicit mod-up and the
moddown_pre / moddown_post back half; N = 2^13 dispatches like 2^12 (tests/golden/ntt_instance_classes.json starts at 2^14), so
it has no case of its own. The gathered mod-up, the CKKS fold path and the deferred top layer exist from N = 2^14, the fused
mod-down store from 2^15 (ntt_can_gather / ntt_can_fuse_moddown): one three-prime case each. The inner product's item group is
min(count, 8) on small batches: eleven ciphertexts give a full group and a short one, the other cases a single group. k = 1
is a single digit; the element list has conjugation (2N - 1) and a non-rotation element.
Seventeen digits take the inner product's loop kernel; 22 elements in one pass (the chunking case) take two launches of 16 + 6."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import hoist_ref as H
import oracle_lib as O
from support import ARENA_MB, S, child_main, compile_cpp, rows, run_arena_child, run_exe

pytestmark = pytest.mark.gpu


def _elts(n):
    return [H.elt_from_step(n, 1), H.elt_from_step(n, -3), 2 * n - 1, 3]


def _session(S, scheme, logn, bits, nsp, mode, t=0, n_keys=4, seed=0):
    """contexts on both sides and random keys: the word-for-word comparison needs no valid keys (not a BaseSession: no
    evaluator is kept, and the keys are drawn here)"""
    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits)
    ctx = S.Context(scheme, logn, mods, nsp, t, mode=mode)
    ref = O.RefContext(scheme, logn, mods, nsp=nsp, t=t, mode=mode)
    rng = np.random.default_rng(seed + logn + len(bits))
    kf = len(mods) - nsp
    nd = (kf + nsp - 1) // nsp
    keys = [rows(rng, mods, n, (nd, 2)) for _ in range(n_keys)]
    dkeys = [S.KSwitchKeys(ctx, key) for key in keys]
    return ctx, ref, mods, rng, keys, dkeys


def _compare(S, ctx, ref, mods, rng, keys, dkeys, k, count, elts, tag):
    n = ref.n
    ct = rows(rng, mods[:k], n, (count, 2))
    d = ctx.upload(ct)
    out = ctx.alloc(len(elts) * count * 2 * k * n)
    S.Evaluator(ctx).apply_galois_many(d, k, count, elts, dkeys, out)
    got = out.download((len(elts), count, 2, k, n))
    assert np.array_equal(d.download(ct.shape), ct), (tag, "the input was modified")
    want = H.hoisted_many(ref, k, ct, elts, keys)
    for i in range(len(elts)):
        for c in range(count):
            assert np.array_equal(got[i, c], want[i, c]), (tag, "element", elts[i], "item", c)
    return ct, got


@pytest.mark.parametrize("bits", [[40, 40, 40, 40], [55, 55, 56, 55]])
def test_ckks_parity_words(S, bits):
    """the FP64 and the integer transform instances; first level and a single digit"""
    ctx, ref, mods, rng, keys, dkeys = _session(S, S.SCHEME_CKKS, 12, bits, 1, S.MODE_PARITY)
    for k in (3, 1):
        _compare(S, ctx, ref, mods, rng, keys, dkeys, k, 3, _elts(ref.n), ("ckks", bits, k))


@pytest.mark.parametrize("mode", [0, 1])
def test_ckks_two_special_primes(S, mode):
    """five ciphertext primes in bundles of two: the last bundle is short (the explicit mod-up kernel)"""
    ctx, ref, mods, rng, keys, dkeys = _session(S, S.SCHEME_CKKS, 12, [40] * 5 + [41] * 2, 2, mode)
    for k in (5, 2):
        _compare(S, ctx, ref, mods, rng, keys, dkeys, k, 3, _elts(ref.n), ("ckks nsp 2", mode, k))


def test_more_than_one_item_group(S):
    """eleven ciphertexts: the inner product keeps its key words across groups of eight, so a second, short group of three
    (item0 > 0, the clamp at the end of the batch)"""
    ctx, ref, mods, rng, keys, dkeys = _session(S, S.SCHEME_CKKS, 12, [40, 40, 41], 1, S.MODE_PARITY, n_keys=2)
    _compare(S, ctx, ref, mods, rng, keys, dkeys, 2, 11, _elts(ref.n)[:2], "two item groups")


def test_more_digits_than_kernel_instances(S):
    """seventeen digits: past the sixteen instances of the inner product, the per-lane loop kernel"""
    ctx, ref, mods, rng, keys, dkeys = _session(S, S.SCHEME_CKKS, 12, [40] * 17 + [41], 1, S.MODE_PARITY, n_keys=2)
    _compare(S, ctx, ref, mods, rng, keys, dkeys, 17, 2, _elts(ref.n)[:2], "17 digits")


@pytest.mark.parametrize("scheme,logn,mode", [(2, 14, 0), (2, 15, 0), (2, 15, 1), (1, 14, 1)])
def test_single_pass_transform_paths(S, scheme, logn, mode):
    """gathered mod-up and target transforms, the CKKS fold (2^14) and its fused mod-down store (2^15), BFV's deferred top"""
    t = 65537 if scheme == 1 else 0
    ctx, ref, mods, rng, keys, dkeys = _session(S, scheme, logn, [40, 40, 41], 1, mode, t=t, n_keys=2)
    _compare(S, ctx, ref, mods, rng, keys, dkeys, 2, 2, _elts(ref.n)[1:3], ("single pass", scheme, logn, mode))


@pytest.mark.parametrize("nsp,bits", [(1, [40, 40, 40, 41]), (2, [40, 40, 40, 41, 41])])
def test_bfv_strict_decrypts_with_the_budget_of_the_sequential_rotation(S, nsp, bits):
    """real keys and ciphertexts: words equal the restatement; the device Decryptor returns the rotated plaintext; the
    invariant noise budget is at least that of the sequential apply_galois minus one bit (a floor of a log2 of terms with
    equal bounds)"""
    logn, n, t = 12, 1 << 12, 65537
    mods = O.coeff_modulus_create(n, bits)
    ctx = S.Context(S.SCHEME_BFV, logn, mods, nsp, t, mode=S.MODE_STRICT)
    ref = O.RefContext(1, logn, mods, nsp=nsp, t=t, mode=1)
    cl = O.Client(ref, seed=9)
    k, count = cl.k, 3
    rng = np.random.default_rng(nsp)
    plains = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    ct = np.stack([cl.encrypt_bfv(plains[c]) for c in range(count)])
    elts = _elts(n)
    keys = [cl.galois_key(g) for g in elts]
    dkeys = [S.KSwitchKeys(ctx, key) for key in keys]
    ev = S.Evaluator(ctx)
    d = ctx.upload(ct)
    out = ctx.alloc(len(elts) * count * 2 * k * n)
    ev.apply_galois_many(d, k, count, elts, dkeys, out)
    got = out.download((len(elts), count, 2, k, n))
    want = H.hoisted_many(ref, k, ct, elts, keys)
    assert np.array_equal(got, want)
    sk = ctx.upload(cl.sk_powers(1))
    total = len(elts) * count
    plain = ctx.alloc(total * n)
    ctx.decrypt(out, 2, k, total, sk, False, plain)
    dec = plain.download((len(elts), count, n))
    hoisted = ctx.invariant_noise_budget(out, 2, k, total, sk).reshape(len(elts), count)
    for i, g in enumerate(elts):
        tab = (np.arange(n, dtype=np.int64) * g) % (2 * n)
        for c in range(count):
            exp = np.zeros(n, dtype=np.uint64)
            exp[tab % n] = np.where(tab >= n, (t - plains[c]) % t, plains[c])
            assert np.array_equal(dec[i, c], exp), (g, c)
        seq = ctx.upload(ct)
        ev.apply_galois_inplace(seq, k, count, g, dkeys[i])
        sequential = ctx.invariant_noise_budget(seq, 2, k, count, sk)
        print("bfv nsp=%d g=%d budgets: hoisted %s sequential %s" % (nsp, g, hoisted[i].tolist(), sequential.tolist()))
        assert np.all(hoisted[i] >= sequential - 1), (g, hoisted[i], sequential)


def test_refusals(S):
    """BFV in PARITY mode; an even element, one >= 2N, a key with fewer digits than the level (the checks that need a key
    handle and so a device, tests/test_hoist_host.py); overlapping buffers"""
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
        d = ctx.upload(ct)
        out = ctx.alloc(2 * count * 2 * k * n)
        sentinel = np.full(out.words, 7, dtype=np.uint64)
        out.upload(sentinel)
        if scheme == S.SCHEME_BFV:
            with pytest.raises(ValueError, match="STRICT"):
                ev.apply_galois_many(d, k, count, [3], [dkey], out)
            with pytest.raises(ValueError, match="STRICT"):
                ev.rotate_vector_many(d, k, count, [1], {H.elt_from_step(n, 1): dkey}, out)
        else:
            for bad in (4, 2 * n, 2 * n + 1, 0):
                with pytest.raises(ValueError, match="Galois element is not valid"):
                    ev.apply_galois_many(d, k, count, [3, bad], [dkey, dkey], out)
            with pytest.raises(ValueError, match="kswitch_keys is not valid"):
                ev.apply_galois_many(d, k, count, [3, 5], [dkey, short], out)
            ev.apply_galois_many(d, 2, count, [3, 5], [dkey, short], out)  # (two digits are enough one level below)
            out.upload(sentinel)
            with pytest.raises(ValueError, match="overlap"):
                ev.apply_galois_many(d, k, count, [3], [dkey], d)
            with pytest.raises(ValueError, match="overlap"):
                ev.apply_galois_many(d.ptr + 8 * k * n, k, count, [3, 5], [dkey, dkey], d)
        assert np.array_equal(out.download(), sentinel) and np.array_equal(d.download(ct.shape), ct)


def test_rotate_vector_many(S):
    """steps {1, 0, -2}: the mapped elements' results, the input in the slot of step 0, a missing key raises, the input is
    bit-identical afterwards"""
    ctx, ref, mods, rng, keys, dkeys = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY, n_keys=2)
    n, k, count = ref.n, 3, 2
    ev = S.Evaluator(ctx)
    e1, e2 = H.elt_from_step(n, 1), H.elt_from_step(n, -2)
    gk = {e1: dkeys[0], e2: dkeys[1]}
    ct = rows(rng, mods[:k], n, (count, 2))
    d = ctx.upload(ct)
    out = ctx.alloc(3 * count * 2 * k * n)
    ctx.profile_enable(True)
    ev.rotate_vector_many(d, k, count, [1, 0, -2], gk, out)
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    assert prof["hoist_mac"]["launches"] == 1, prof  # one decomposition for both rotations: the step 0 between them is a copy
    got = out.download((3, count, 2, k, n))
    many = ctx.alloc(2 * count * 2 * k * n)
    ev.apply_galois_many(d, k, count, [e1, e2], dkeys, many)
    exp = many.download((2, count, 2, k, n))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[2], exp[1])
    assert np.array_equal(got[1], ct)
    assert np.array_equal(exp, H.hoisted_many(ref, k, ct, [e1, e2], keys))
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.rotate_vector_many(d, k, count, [1, 3], gk, out)
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.rotate_vector_many(d, k, count, [3], {}, out)
    assert np.array_equal(d.download(ct.shape), ct)


def test_transparency_flags_in_output_order(S):
    """a ciphertext with c1 = 0 is transparent under every element: one flag per output, element-major; step 0 included"""
    ctx, ref, mods, rng, keys, dkeys = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY, n_keys=2)
    n, k, count = ref.n, 3, 3
    ev = S.Evaluator(ctx)
    ct = rows(rng, mods[:k], n, (count, 2))
    ct[1, 1] = 0
    d = ctx.upload(ct)
    e1, e2 = H.elt_from_step(n, 1), H.elt_from_step(n, -2)
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
        out = ctx.alloc(3 * count * 2 * k * n)
        ev.apply_galois_many(d, k, count, [e1, e2], dkeys, out)
        got = flags.download().view(np.uint32)
        assert (got[:6] != 0).tolist() == [True, False, True] * 2 and np.all(got[6:] == 5)
        with_sink = out.download()[: 2 * count * 2 * k * n].copy()
        ev.rotate_vector_many(d, k, count, [1, 0, -2], {e1: dkeys[0], e2: dkeys[1]}, out)
        got = flags.download().view(np.uint32)
        assert (got[:9] != 0).tolist() == [True, False, True] * 3 and np.all(got[9:] == 5)
        ctx.transparency_sink(flags, 5)
        with pytest.raises(ValueError, match="sink"):
            ev.apply_galois_many(d, k, count, [e1, e2], dkeys, out)
    finally:
        ctx.transparency_sink(None, 0)
    ev.apply_galois_many(d, k, count, [e1, e2], dkeys, out)
    assert np.array_equal(out.download()[: with_sink.size], with_sink)


def test_graph_capture(S):
    """warm the Galois tables, capture one call, replay it twice on new inputs: the words of the eager call"""
    ctx, ref, mods, rng, keys, dkeys = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 41], 1, S.MODE_PARITY, n_keys=2)
    n, k, count = ref.n, 3, 2
    ev = S.Evaluator(ctx)
    elts = _elts(n)[:2]
    d = ctx.upload(rows(rng, mods[:k], n, (count, 2)))
    out = ctx.alloc(2 * count * 2 * k * n)
    g = ctx.capture(lambda: ev.apply_galois_many(d, k, count, elts, dkeys, out))
    for _ in range(2):
        ct = rows(rng, mods[:k], n, (count, 2))
        d.upload(ct)
        g.launch()
        got = out.download((2, count, 2, k, n))
        assert np.array_equal(got, H.hoisted_many(ref, k, ct, elts, keys))


def test_cpp_adapter(S, tmp_path):
    """tests/host_adapter_hoist_check.cpp: the host-ciphertext and the DeviceCiphertext overloads give the ABI's words on the
    same seeded inputs, with the operand's metadata; the deferred transparency exception arrives"""
    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_hoist_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", *mods, timeout=120)
    sm = O.SplitMix(0x4015)
    ct = sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n)
    keys = [sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n) for _ in range(2)]
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ev = S.Evaluator(ctx)
    e1, e2 = H.elt_from_step(n, 1), H.elt_from_step(n, -2)
    dkeys = [S.KSwitchKeys(ctx, key) for key in keys]
    d = ctx.upload(ct)
    many = ctx.alloc(2 * 2 * k * n)
    ev.apply_galois_many(d, k, 1, [e1, e2], dkeys, many)
    rot = ctx.alloc(3 * 2 * k * n)
    ev.rotate_vector_many(d, k, 1, [1, 0, -2], {e1: dkeys[0], e2: dkeys[1]}, rot)
    for name, buf, count in (("apply_galois_many", many, 2), ("rotate_vector_many", rot, 3)):
        for side in ("host", "device"):
            line = "%s %s digest %016x count %d meta 1" % (side, name, O.fnv(buf.download()), count)
            assert line in stdout, (line, stdout)
    assert "deferred transparency ok" in stdout, stdout


# ---------------------------------------------------------------- arena chunks (a child process with the smallest arena)
LOGN, N = 13, 1 << 13


def _child():
    """N = 2^13, 8 + 1 primes, k = 8: the digits of one item take 5 MiB of the 64 MiB arena, every element 2.625 MiB more
    (w_ext + w_coeff, and w_prod + w_temp + k N). Two elements: 10.25 MiB per item, 6 items per chunk, so 7 items need a
    second, ragged chunk (one back half per element there). 23 elements: 65.4 MiB for one item, so the element list is split
    22 + 1 with the digits kept; the chunk is then a single item by construction (a pass takes all the arena the digits
    leave), so the split shows with a second item chunk but never a ragged one -- the two are separate calls."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    mods = O.coeff_modulus_create(N, [50] * 8 + [60])
    ctx = S.Context(S.SCHEME_CKKS, LOGN, mods, 1, 0)
    ref = O.RefContext(2, LOGN, mods, nsp=1)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(64)
    k = 8
    elts = [2 * i + 3 for i in range(23)]
    keys = [rows(rng, mods, N, (8, 2)) for _ in elts]
    dkeys = [S.KSwitchKeys(ctx, key) for key in keys]

    def run(count, n_elts, items, which):
        ct = rows(rng, mods[:k], N, (count, 2))
        d = ctx.upload(ct)
        out = ctx.alloc(n_elts * count * 2 * k * N)
        ctx.chunk_log()
        ev.apply_galois_many(d, k, count, elts[:n_elts], dkeys[:n_elts], out)
        log = ctx.chunk_log()
        got = out.download((n_elts, count, 2, k, N))
        for i in which:
            kinv = H.hoisted_key(ref, keys[i], elts[i])
            for c in items:
                assert np.array_equal(got[i, c], H.hoisted_rotation(ref, k, ct[c], elts[i], keys[i], kinv)), (n_elts, i, c)
        d.free()
        out.free()
        return log

    log = run(7, 2, (0, 5, 6), (0, 1))
    assert log == [(7, 6)], log                      # a second, ragged item chunk; the element list whole
    log = run(2, 23, (0, 1), (0, 15, 16, 21, 22))
    assert log == [(23, 22), (2, 1)], log            # the element list split 22 + 1, one item per chunk
    print("HOIST_CHUNKS_OK")


def test_chunked_items_and_split_element_list():
    run_arena_child(__file__, "HOIST_CHUNKS_OK", timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
