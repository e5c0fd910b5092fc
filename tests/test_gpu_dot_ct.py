"""Ciphertext inner products on the device (sealhip_evaluator_dot_product) against the oracle: CKKS word
for word against the composition ref_ckks_multiply / ref_evaluator_add / ref_relinearize, BFV (STRICT) against the restatement
of tests/dot_ct_ref.py.

Shapes: the smallest that reach every path. N = 2^12 takes the tiled transforms and the copy + lift front; N = 2^14 the
gathered forward transform and the deferred top layer of the inverse. tensor_dot_kernel sums up to 16 terms per launch: 1, 2
and 5 terms are one group, 17 a full group and a group of one that adds the partial sum in, 33 three groups. The kernel does
not group items; three items with an odd row count give a last block that is not full."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import dot_ct_ref as D
import oracle_lib as O
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe, session_memo

pytestmark = pytest.mark.gpu


class Session(BaseSession):
    """contexts on both sides and a random key: the word-for-word comparison needs no valid key"""

    def __init__(self, S, scheme, logn, bits, nsp, mode, t=0, seed=0):
        super().__init__(S, scheme, logn, bits, nsp, mode, t, seed + logn + len(bits))
        self.key_host = rows(self.rng, self.mods, self.n, (self.nd, 2))
        self.key = S.KSwitchKeys(self.ctx, self.key_host)

    def run(self, k, count, a_idx, b_idx, pool, keys):
        """the call over device copies of pool[i] (count x 2 x k x N each), terms (a_idx[j], b_idx[j]); returns the result
        and checks that no operand changed"""
        n = self.n
        dev = [self.ctx.upload(p) for p in pool]
        out = self.ctx.alloc(count * (2 if keys else 3) * k * n)
        self.ev.dot_product([dev[i] for i in a_idx], [dev[i] for i in b_idx], k, count, out, [self.key] if keys else None)
        got = out.download((count, 2 if keys else 3, k, n))
        for d, p in zip(dev, pool):
            assert np.array_equal(d.download(p.shape), p), "an operand was modified"
            d.free()
        out.free()
        return got

    def compare(self, k, count, n_terms, keys, tag, items=None, a_idx=None, b_idx=None):
        pool_size = 2 * n_terms if a_idx is None else 1 + max(a_idx + b_idx)
        pool = [rows(self.rng, self.mods[:k], self.n, (count, 2)) for _ in range(pool_size)]
        a_idx = list(range(n_terms)) if a_idx is None else a_idx
        b_idx = list(range(n_terms, 2 * n_terms)) if b_idx is None else b_idx
        got = self.run(k, count, a_idx, b_idx, pool, keys)
        for c in (range(count) if items is None else items):
            want = D.dot_product(self.ref, k, [pool[i][c] for i in a_idx], [pool[i][c] for i in b_idx],
                                 self.key_host if keys else None)
            assert np.array_equal(got[c], want), (tag, "item", c)
        return pool, got


_session = session_memo(Session)


@pytest.mark.parametrize("keys", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bits", [(40, 40, 40, 40), (55, 55, 56, 55)])
def test_ckks_words(S, bits, mode, keys):
    """the first level and the last; one group, two groups with a short second, three groups; three items"""
    se = _session(S, S.SCHEME_CKKS, 12, list(bits), 1, mode)
    for k in (3, 1):
        for n_terms in (1, 2, 5, 17, 33):
            se.compare(k, 3, n_terms, keys, ("ckks", bits, mode, k, n_terms, keys), items=(0, 2) if n_terms > 5 else None)


@pytest.mark.parametrize("keys", [False, True])
def test_ckks_two_special_primes(S, keys):
    se = _session(S, S.SCHEME_CKKS, 12, [40] * 5 + [41] * 2, 2, 0)
    for k in (5, 2):
        se.compare(k, 3, 17, keys, ("ckks nsp 2", k, keys), items=(0, 2))


@pytest.mark.parametrize("keys", [False, True])
@pytest.mark.parametrize("logn", [12, 14])
def test_bfv_strict_words(S, logn, keys):
    """2^12: tiled transforms, copy + lift; 2^14: the gathered forward transform and the inverse's deferred top layer"""
    bits, k = ([40, 40, 40, 41], 3) if logn == 12 else ([40, 40, 41], 2)
    se = _session(S, S.SCHEME_BFV, logn, bits, 1, S.MODE_STRICT, t=65537)
    for n_terms in (1, 2, 17):
        count = 3 if n_terms < 17 else 2
        pool, got = se.compare(k, count, n_terms, keys, ("bfv", logn, n_terms, keys), items=(count - 1,))
        if n_terms == 1 and not keys:
            # one term is Evaluator::multiply: the reference's words, and the device's own multiply
            a, b = se.ctx.upload(pool[0]), se.ctx.upload(pool[1])
            prod = se.ctx.alloc(count * 3 * k * se.n)
            se.ev.multiply(a, 2, b, 2, k, count, prod)
            assert np.array_equal(prod.download(got.shape), got)
            want = np.zeros((3, k, se.n), dtype=np.uint64)
            for c in range(count):
                assert O.lib().ref_bfv_multiply(C.byref(se.ref.c), k, O.ptr(pool[0][c]), 2, O.ptr(pool[1][c]), 2, O.ptr(want)) == 0
                assert np.array_equal(got[c], want)


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_repeated_pointers_and_squares(S, scheme):
    """a_terms[i] == b_terms[i] (a sum of squares) and the same buffer in several terms"""
    if scheme == "bfv":
        se, k = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537), 3
    else:
        se, k = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 40], 1, 0), 3
    for keys in (False, True):
        se.compare(k, 2, 4, keys, (scheme, "repeats", keys), a_idx=[0, 1, 0, 2], b_idx=[0, 2, 0, 2])


def test_bfv_semantics_with_a_real_key(S):
    """five encrypted pairs, the sum and ONE relinearization on the device: decrypts to sum m_a m_b mod (x^N + 1, t)"""
    logn, n, t = 12, 1 << 12, 65537
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT)
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    cl = O.Client(ref, seed=18)
    ev, k = S.Evaluator(ctx), cl.k
    rng = np.random.default_rng(18)
    ma = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(5)]
    mb = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(5)]
    a, b = [cl.encrypt_bfv(m) for m in ma], [cl.encrypt_bfv(m) for m in mb]
    want = np.zeros(n, dtype=np.uint64)
    for x, y in zip(ma, mb):
        want = (want + O.negacyclic_mod_t(x, y, t)) % np.uint64(t)
    key_host = cl.relin_key()
    key = S.KSwitchKeys(ctx, key_host)
    da, db = [ctx.upload(c) for c in a], [ctx.upload(c) for c in b]
    out3, out2 = ctx.alloc(3 * k * n), ctx.alloc(2 * k * n)
    ev.dot_product(da, db, k, 1, out3)
    ev.dot_product(da, db, k, 1, out2, [key])
    got3, got2 = out3.download((3, k, n)), out2.download((2, k, n))
    assert np.array_equal(cl.decrypt_bfv(got3), want)
    assert np.array_equal(cl.decrypt_bfv(got2), want)
    assert np.array_equal(got3, D.bfv_dot_product(ref, k, a, b))
    assert np.array_equal(got2, D.bfv_dot_product(ref, k, a, b, key_host))


def test_refusals_that_need_a_device(S):
    """a key with fewer digits than the level; too small a sink; each leaves the output untouched"""
    se = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 40], 1, 0)
    ctx, ev, n, k = se.ctx, se.ev, se.n, 3
    short = S.KSwitchKeys(ctx, rows(se.rng, se.mods, n, (2, 2)))
    a, b = ctx.upload(rows(se.rng, se.mods[:k], n, (1, 2))), ctx.upload(rows(se.rng, se.mods[:k], n, (1, 2)))
    sentinel = np.full(2 * k * n, 0x5A5A5A5A, dtype=np.uint64)
    out = ctx.upload(sentinel)
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        ev.dot_product([a], [b], k, 1, out, [short])
    ev.dot_product([a], [b], 2, 1, out, [short])  # (two digits do one level below)
    out.upload(sentinel)
    with pytest.raises(ValueError, match="not enough relinearization keys"):
        ev.dot_product([a], [b], k, 1, out, [])
    flags = ctx.alloc(8)
    ctx.transparency_sink(flags, 1)
    try:
        with pytest.raises(ValueError, match="sink"):
            ev.dot_product([a, a], [b, b], k, 2, out, [se.key])
    finally:
        ctx.transparency_sink(None, 0)
    assert np.array_equal(out.download(), sentinel)


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_transparency_flags(S, scheme):
    """one flag per output ciphertext: set for ordinary inputs, clear for the item whose c_1 operands are all zero -- written
    by the new kernel (CKKS) or the floor (BFV) without keys, by the key switch's storing kernel with them"""
    if scheme == "bfv":
        se, k = _session(S, S.SCHEME_BFV, 12, [40, 40, 40, 41], 1, S.MODE_STRICT, t=65537), 3
    else:
        se, k = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 40], 1, 0), 3
    ctx, ev, n, count, n_terms = se.ctx, se.ev, se.n, 3, 17
    pool = [rows(se.rng, se.mods[:k], n, (count, 2)) for _ in range(2 * n_terms)]
    for p in pool:
        p[1, 1] = 0
    dev = [ctx.upload(p) for p in pool]
    flags = ctx.alloc(8)  # 16 uint32 words
    ctx.transparency_sink(flags, 16)
    try:
        for keys in (False, True):
            out = ctx.alloc(count * (2 if keys else 3) * k * n)
            flags.upload(np.full(8, 0x0000000500000005, dtype=np.uint64))
            ev.dot_product(dev[:n_terms], dev[n_terms:], k, count, out, [se.key] if keys else None)
            got = flags.download().view(np.uint32)
            assert (got[:3] != 0).tolist() == [True, False, True] and np.all(got[3:] == 5), (keys, got)
            res = out.download((count, 2 if keys else 3, k, n))
            assert not res[1, 1:].any() and res[0, 1:].any()
    finally:
        ctx.transparency_sink(None, 0)


def _profile(ctx, fn):
    fn()  # (arena and tables in place)
    ctx.profile_enable(True)
    fn()
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    return prof


def _units(prof, prefix):
    return {tag: v["units"] for tag, v in prof.items() if tag.startswith(prefix)}


@pytest.mark.parametrize("logn", [12, 14])
def test_work_done_once(S, logn):
    """BFV, 5 terms, two items, relinearized: the inverse transforms walk the rows of ONE product (3 (k + |Bsk|) per item) and
    of one key switch, the forward transforms those of five; three floors, one tensor_dot launch, one key-switch inner product.
    Counted per transform kernel against multiply and relinearize profiled on their own (at 2^12, where multiply takes the same
    unfused launches), and as the plain number where a transform is one launch (2^14)."""
    bits, k = ([40, 40, 40, 41], 3) if logn == 12 else ([40, 40, 41], 2)
    se = _session(S, S.SCHEME_BFV, logn, bits, 1, S.MODE_STRICT, t=65537)
    ctx, ev, n, count, n_terms = se.ctx, se.ev, se.n, 2, 5
    kb = k + len(D.bsk_primes(n, se.mods[:k], 65537))
    dev = [ctx.upload(rows(se.rng, se.mods[:k], n, (count, 2))) for _ in range(2 * n_terms)]
    out2, out3 = ctx.alloc(count * 2 * k * n), ctx.alloc(count * 3 * k * n)
    dot = _profile(ctx, lambda: ev.dot_product(dev[:n_terms], dev[n_terms:], k, count, out2, [se.key]))
    plain = _profile(ctx, lambda: ev.dot_product(dev[:n_terms], dev[n_terms:], k, count, out3))
    mul = _profile(ctx, lambda: ev.multiply(dev[0], 2, dev[1], 2, k, count, out3))
    rel = _profile(ctx, lambda: ev.relinearize_inplace(out3, 3, k, count, [se.key]))
    print(dot, plain, mul, rel)
    assert dot["bfv_floor_sk"]["launches"] == 3 and plain["bfv_floor_sk"]["launches"] == 3
    assert dot["tensor_dot"]["launches"] == 1 and dot["ks_mac"]["launches"] == 1 and "ks_mac" not in plain
    assert dot["bfv_lift"]["launches"] == 4 * n_terms and "tensor_product" not in dot
    inv_dot, inv_plain, inv_rel = _units(dot, "ntt_inv"), _units(plain, "ntt_inv"), _units(rel, "ntt_inv")
    for tag in set(inv_dot) | set(inv_plain) | set(inv_rel):
        assert inv_dot.get(tag, 0) == inv_plain.get(tag, 0) + inv_rel.get(tag, 0), (tag, dot, plain, rel)
    if "ntt_inv_pass" not in inv_plain:  # (every transform is one launch: the units are the rows)
        assert sum(inv_plain.values()) == 3 * kb * count, plain
    if logn == 12:
        assert inv_plain == _units(mul, "ntt_inv"), (plain, mul)
        fwd_plain, fwd_mul = _units(plain, "ntt_fwd"), _units(mul, "ntt_fwd")
        assert fwd_plain == {tag: n_terms * v for tag, v in fwd_mul.items()}, (plain, mul)


def test_graph_capture(S):
    """one CKKS call with three terms and keys, captured after a warm-up and replayed on new inputs"""
    se = _session(S, S.SCHEME_CKKS, 12, [40, 40, 40, 40], 1, 0)
    ctx, ev, n, k, count = se.ctx, se.ev, se.n, 3, 2
    dev = [ctx.upload(rows(se.rng, se.mods[:k], n, (count, 2))) for _ in range(6)]
    out = ctx.alloc(count * 2 * k * n)
    run = lambda: ev.dot_product(dev[:3], dev[3:], k, count, out, [se.key])
    run()
    g = ctx.capture(run)
    for _ in range(2):
        pool = [rows(se.rng, se.mods[:k], n, (count, 2)) for _ in range(6)]
        for d, p in zip(dev, pool):
            d.upload(p)
        g.launch()
        replayed = out.download((count, 2, k, n)).copy()
        out.upload(np.zeros(count * 2 * k * n, dtype=np.uint64))
        run()
        assert np.array_equal(out.download((count, 2, k, n)), replayed)
        for c in range(count):
            want = D.ckks_dot_product(se.ref, k, [p[c] for p in pool[:3]], [p[c] for p in pool[3:]], se.key_host)
            assert np.array_equal(replayed[c], want)


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_cpp_adapter(S, tmp_path, scheme):
    """tests/host_adapter_dot_ct_check.cpp: the host-ciphertext and the DeviceCiphertext forms, with and without keys, give the
    ABI's words on the same seeded inputs, with the operands' level and form and, for CKKS, the product of the scales"""
    logn, n, k = 12, 1 << 12, 3
    mods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    exe = compile_cpp(tmp_path, "host_adapter_dot_ct_check.cpp", link_sealhip=True)
    stdout = run_exe(exe, "0", scheme, *mods, timeout=120)
    sm = O.SplitMix(0x4018)
    terms = [sm.fill(2 * k, n, mods[:k] * 2).reshape(1, 2, k, n) for _ in range(6)]
    key = sm.fill(3 * 2 * 4, n, mods * 6).reshape(3, 2, 4, n)
    if scheme == "ckks":
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    else:
        ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, 65537, mode=S.MODE_STRICT)
    ev = S.Evaluator(ctx)
    dev = [ctx.upload(t) for t in terms]
    dkey = S.KSwitchKeys(ctx, key)
    out3, out2 = ctx.alloc(3 * k * n), ctx.alloc(2 * k * n)
    ev.dot_product(dev[:3], dev[3:], k, 1, out3)
    ev.dot_product(dev[:3], dev[3:], k, 1, out2, [dkey])
    for name, buf in (("size3", out3), ("relin", out2)):
        for side in ("host", "device"):
            line = "%s %s digest %016x meta 1" % (side, name, O.fnv(buf.download()))
            assert line in stdout, (line, stdout)


# ---------------------------------------------------------------- the term list walked in passes (a child process with the
# smallest arena)
LOGN, N, T = 15, 1 << 15, 65537


def _child():
    """BFV STRICT, N = 2^15, [40, 40, 40, 41], k = 3: a term in the extended base is 4 (k + |Bsk|) rows of 256 KiB, the sum 3
    (k + |Bsk|) rows. Nine terms and the sum do not fit 64 MiB, so the term list is walked in passes of
    (64 MiB - sum - c_2) / term, each pass adding into the canonical partial sum: the words are unchanged."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    mods = O.coeff_modulus_create(N, [40, 40, 40, 41])
    ctx = S.Context(S.SCHEME_BFV, LOGN, mods, 1, T, mode=S.MODE_STRICT)
    ref = O.RefContext(1, LOGN, mods, nsp=1, t=T, mode=1)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(64)
    k, n_terms = 3, 9
    kb = k + len(D.bsk_primes(N, mods[:k], T))
    budget, row = int(ARENA_MB) << 20, N * 8
    key_host = rows(rng, mods, N, (3, 2))
    key = S.KSwitchKeys(ctx, key_host)
    pool = [rows(rng, mods[:k], N, (1, 2)) for _ in range(2 * n_terms)]
    dev = [ctx.upload(p) for p in pool]
    for keys in (False, True):
        fixed = (3 * kb + (k if keys else 0)) * row
        per_pass = (budget - fixed) // (4 * kb * row)
        assert 1 <= per_pass < n_terms
        out = ctx.alloc((2 if keys else 3) * k * N)
        ctx.chunk_log()
        ev.dot_product(dev[:n_terms], dev[n_terms:], k, 1, out, [key] if keys else None)
        log = ctx.chunk_log()
        assert log[:2] == [(n_terms, per_pass), (1, 1)], log  # the term split ahead of the item chunks
        assert log[2:] == ([(1, 1)] if keys else []), log     # (the key switch's own chunk)
        got = out.download((2 if keys else 3, k, N))
        want = D.bfv_dot_product(ref, k, [p[0] for p in pool[:n_terms]], [p[0] for p in pool[n_terms:]], key_host if keys else None)
        assert np.array_equal(got, want), keys
    print("DOT_CT_PASSES_OK")


def test_term_list_walked_in_passes():
    run_arena_child(__file__, "DOT_CT_PASSES_OK", timeout=300)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
