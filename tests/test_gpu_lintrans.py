"""Matrix-vector products from a caller's matrix on the device (sealhip_linear_transform_* and
sealhip_evaluator_linear_transform).

1. The occupancy scan and the gather kernel, bit for bit against the numpy restatement (tests/lintrans_ref.py): N = 16 is a
   ring below a workgroup (d = 1, 2 and the full d = n = 8), N = 2^10 has d = 1, a d of several blocks and the full d = n = 512
   at the strides 1, default and d, N = 2^13 a d = 64 tiled 64 times. Planted: a -0.0, a single non-zero entry on the last
   diagonal, a NaN.
2. The transform's words: those of rotate_vector_bsgs_plain[_rescale] fed with tables the test builds itself -- the
   restatement's values through sealhip_ckks_encode at k = n_key, the restatement's steps -- at N = 2^10 and 2^13, both
   modes, one and three ciphertexts, two levels served by one tables object, for a dense matrix, a band, diagonal 0 alone
   (no key, no key-switch term) and one non-identity diagonal.
3. The tables built in chunks under the smallest arena: the same words, more than one chunk.
4. Boundary behaviour: the checks and their order, transparency flags, graph capture, the pool."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import hoist_ref as H
import lintrans_ref as R
import oracle_lib as O
from support import ARENA_MB, BaseSession, S, child_main, compile_cpp, rows, run_arena_child, run_exe, session_memo

pytestmark = pytest.mark.gpu


def _download(S, ctx, ptr, shape):
    out = np.empty(shape, dtype=np.uint64)
    ctx.synchronize()
    S._check(S.lib().sealhip_memcpy_d2h(ctx.handle, out.ctypes.data, ptr, out.nbytes))
    return out


def _upload_matrix(ctx, M):
    return ctx.upload(np.ascontiguousarray(M, dtype=np.complex128).view(np.uint64))


class Session(BaseSession):
    """CKKS contexts on both sides; the Galois keys are random words"""

    def __init__(self, S, logn, bits, nsp, mode=0, seed=0):
        super().__init__(S, S.SCHEME_CKKS, logn, bits, nsp, mode, 0, seed + 37 * logn + nsp)
        self.n_key, self.slots = len(self.mods), self.n // 2
        self.host_keys, self.dev_keys = {}, {}

    def random_keys(self, steps):
        elts = [H.elt_from_step(self.n, s) for s in steps]
        for g in elts:
            if g not in self.dev_keys:
                self.host_keys[g] = rows(self.rng, self.mods, self.n, (self.nd, 2))
                self.dev_keys[g] = self.S.KSwitchKeys(self.ctx, self.host_keys[g])
        return {g: self.dev_keys[g] for g in elts}

    def own_tables(self, M, mask, n1, scale, gain=1.0):
        """(device plaintexts [n_giant][n_baby][n_key][N], plan): the restatement's values through sealhip_ckks_encode"""
        W, pl = R.values(M, self.slots, mask, n1, gain)
        plains = self.ctx.ckks_encode(W.reshape(-1, self.slots), self.n_key, scale)
        return plains, pl


_made = session_memo(Session)


def _session(S, logn, bits, nsp, mode=0):
    return _made(S, logn, list(bits), nsp, mode)


def _matrices(d, rng):
    """(name, matrix, mask of its non-zero diagonals): dense, band, diagonal 0 alone, one non-identity diagonal"""
    named = R.masks(d, rng, 0)
    out = [("dense", named[0]), ("diag0", named[1])]
    if d > 1:
        out += [("single", named[2]), ("band", named[3])]
    return [(name, R.masked_matrix(d, mask, rng), mask) for name, mask in out]


# ------------------------------------------------------------------ 1. the scan and the gather
@pytest.mark.parametrize("logn,d", [(4, 1), (4, 2), (4, 8), (10, 1), (10, 32), (10, 512), (13, 64)])
def test_occupancy_and_values(S, logn, d):
    se = _session(S, logn, [40] * 4, 1)
    ev, n = se.ev, se.slots
    rng = np.random.default_rng(1000 * logn + d)
    cases = _matrices(d, rng)
    planted = np.zeros((d, d), dtype=np.complex128)  # -0.0 everywhere it shows, one tiny entry on the last diagonal
    planted.real[::2] = -0.0
    planted.imag[:, ::3] = -0.0
    planted[d - 1, (2 * d - 2) % d] = complex(0.0, -5e-324) if d > 1 else complex(-0.0, 3.0)
    cases.append(("planted", planted, None))
    default = R.default_n1(np.ones(d, dtype=np.uint8))
    for name, M, mask in cases:
        dM = _upload_matrix(se.ctx, M)
        want_occ, finite = R.occupancy(M)
        assert finite
        got_occ = ev.linear_transform_diagonals(dM, d)
        assert np.array_equal(got_occ, want_occ), (name, got_occ, want_occ)
        if mask is not None:
            assert np.array_equal(want_occ, mask)
        else:
            assert list(np.flatnonzero(want_occ)) == [d - 1]
        # the diagonals found at the strides 1, default of the dense grid, d and the mask's own default; every diagonal once
        for use_mask, n1, gain in [(want_occ, s, g) for s in sorted({0, 1, default, d}) for g in (1.0, -0.8125)] + [(None, default, 3.0)]:
            got = ev.linear_transform_values(dM, d, use_mask, n1, gain)
            want, _ = R.values(M, n, use_mask, n1, gain)
            assert got.shape == want.shape
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, n1, gain)
            host = ev.linear_transform_values(M, d, use_mask, n1, gain, host=True)
            assert np.array_equal(got.view(np.uint64), host.view(np.uint64))
        dM.free()
    # a NaN, an infinity: refused by the scan and by the tables
    for bad in (float("nan"), float("inf")):
        M = cases[0][1].copy()
        M[d - 1, 0] = complex(1.0, bad)
        dM = _upload_matrix(se.ctx, M)
        with pytest.raises(ValueError, match="not finite"):
            ev.linear_transform_diagonals(dM, d)
        with pytest.raises(ValueError, match="not finite"):
            S.LinearTransform(se.ctx, dM, d, 2.0 ** 30)
        dM.free()


# ------------------------------------------------------------------ 2. the words
@pytest.mark.parametrize("mode", [0, 1], ids=["parity", "strict"])
@pytest.mark.parametrize("logn,d", [(10, 16), (13, 32)])
def test_transform_words(S, logn, d, mode):
    se = _session(S, logn, [40] * 5, 1, mode)
    ctx, ev, n = se.ctx, se.ev, se.n
    rng = np.random.default_rng(77 * logn + mode)
    scale = 2.0 ** 30
    cts = {(k, count): rows(se.rng, se.mods[:k], n, (count, 2)) for k in (4, 3) for count in (1, 3)}
    d_cts = {key: ctx.upload(ct) for key, ct in cts.items()}
    for name, M, mask in _matrices(d, rng):
        dM = _upload_matrix(ctx, M)
        tables = S.LinearTransform(ctx, dM, d, scale)
        plains, pl = se.own_tables(M, mask, 0, scale)
        assert tables.scale == scale
        for key in ("d", "n_diagonals", "n1", "n_baby", "n_giant", "baby_steps", "giant_steps", "key_steps"):
            assert tables.plan[key] == pl[key], (name, key)
        shape = (pl["n_giant"], pl["n_baby"], se.n_key, n)
        table_words = _download(S, ctx, tables.plain_ptr(), shape)
        assert np.array_equal(table_words, plains.download(shape)), name
        gk = se.random_keys(pl["key_steps"])
        if name == "diag0":
            assert gk == {} and pl["baby_steps"] == [0] and pl["giant_steps"] == [0]
        for (k, count), d_ct in d_cts.items():  # one tables object serves both levels
            for rescale in (False, True):
                ko = k - 1 if rescale else k
                got, want = ctx.alloc(count * 2 * ko * n), ctx.alloc(count * 2 * ko * n)
                ev.linear_transform(tables, d_ct, k, count, gk, got, rescale=rescale)
                bsgs = ev.rotate_vector_bsgs_plain_rescale if rescale else ev.rotate_vector_bsgs_plain
                bsgs(d_ct, k, count, pl["baby_steps"], pl["giant_steps"], gk, plains, want)
                assert np.array_equal(got.download(), want.download()), (name, k, count, rescale)
                assert np.array_equal(d_ct.download(cts[(k, count)].shape), cts[(k, count)]), "the input was modified"
        assert np.array_equal(_download(S, ctx, tables.plain_ptr(), shape), table_words), "the tables were modified"
        tables.free()
        dM.free()


# ------------------------------------------------------------------ 3. the tables in chunks (a child process with the
# smallest arena)
def _child():
    """N = 2^13, three primes, a dense d = 512 matrix at the default stride: 512 cells. A cell takes n complex values (64 KiB,
    a pool block) and the encoder N complex coefficients (128 KiB of the arena): 341 cells fit 64 MiB, so the grid is built
    in chunks of 341 + 171 cells. The words are those of the restatement's values through sealhip_ckks_encode."""
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    logn, N, n, d, scale = 13, 1 << 13, 1 << 12, 512, 2.0 ** 30
    mods = O.coeff_modulus_create(N, [40, 40, 41])
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    rng = np.random.default_rng(512)
    M = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    dM = _upload_matrix(ctx, M)
    per_chunk = (int(ARENA_MB) << 20) // (n * 16 + N * 16)
    assert 1 <= per_chunk < d
    ctx.chunk_log()
    tables = S.LinearTransform(ctx, dM, d, scale, gain=0.5)
    log = ctx.chunk_log()
    assert (d, per_chunk) in log, log  # (the encoder's own entries follow it, one chunk each)
    assert tables.plan["n_baby"] * tables.plan["n_giant"] == d
    W, pl = R.values(M, n, None, 0, 0.5)
    shape = (d, len(mods), N)
    got = _download(S, ctx, tables.plain_ptr(), shape)
    for lo in range(0, d, 128):
        want = ctx.ckks_encode(W.reshape(d, n)[lo:lo + 128], len(mods), scale)
        assert np.array_equal(got[lo:lo + 128], want.download((128, len(mods), N))), lo
        want.free()
    tables.free()
    print("LINTRANS_CHUNKS_OK")


def test_tables_built_in_chunks():
    run_arena_child(__file__, "LINTRANS_CHUNKS_OK", timeout=300)


# ------------------------------------------------------------------ 4. boundary behaviour
def test_checks_flags_capture_pool(S):
    se = _session(S, 10, [40] * 5, 1)
    ctx, ev, n, d, k, count, scale = se.ctx, se.ev, se.n, 16, 4, 3, 2.0 ** 30
    rng = np.random.default_rng(4)
    M = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    dM = _upload_matrix(ctx, M)
    start = ctx.pool_stats()["bytes_in_use"]
    tables = S.LinearTransform(ctx, dM, d, scale)
    gk = se.random_keys(tables.plan["key_steps"])
    ct = rows(se.rng, se.mods[:k], n, (count, 2))
    d_ct = ctx.upload(ct)
    out = ctx.alloc(count * 2 * k * n)
    L = S.lib()
    E = lambda hr: hr & 0xFFFFFFFF
    ea, ka, nk = S._galois_arrays(gk)
    # E_POINTER before everything else
    assert E(L.sealhip_evaluator_linear_transform(ctx.handle, tables.handle, 9, None, count, ea, ka, nk, 0, out.ptr)) == S.E_POINTER
    assert E(L.sealhip_evaluator_linear_transform(ctx.handle, tables.handle, 9, d_ct.ptr, count, None, ka, nk, 0, out.ptr)) == S.E_POINTER
    # tables of another context; a step whose key is absent; a short key; the level; overlap
    other = S.Context(S.SCHEME_CKKS, 10, se.mods, 1, 0)
    with pytest.raises(ValueError, match="another context"):
        S.Evaluator(other).linear_transform(tables, d_ct, k, count, gk, out)
    drop = H.elt_from_step(n, tables.plan["key_steps"][-1])
    with pytest.raises(ValueError, match="Galois key not present"):
        ev.linear_transform(tables, d_ct, k, count, {g: key for g, key in gk.items() if g != drop}, out)
    short = S.KSwitchKeys(ctx, se.host_keys[drop][:2])
    with pytest.raises(ValueError, match="kswitch_keys is not valid"):
        ev.linear_transform(tables, d_ct, k, count, {**gk, drop: short}, out)
    for bad_k, rescale in ((0, False), (5, False), (1, True)):
        with pytest.raises(ValueError):
            ev.linear_transform(tables, d_ct, bad_k, count, gk, out, rescale=rescale)
    with pytest.raises(ValueError, match="overlap ct"):
        ev.linear_transform(tables, d_ct, k, count, gk, d_ct)
    # the tables' refusals: an all-zero matrix, the encoder's own two
    zero = _upload_matrix(ctx, np.zeros((d, d), dtype=np.complex128))
    with pytest.raises(ValueError, match="transparent"):
        S.LinearTransform(ctx, zero, d, scale)
    with pytest.raises(ValueError, match="scale out of bounds"):
        S.LinearTransform(ctx, dM, d, 2.0 ** 300)
    with pytest.raises(ValueError, match="encoded values are too large"):
        S.LinearTransform(ctx, dM, d, 2.0 ** 100, gain=2.0 ** 120)
    assert ctx.pool_stats()["bytes_in_use"] == start, "a refused create kept pool memory"
    # the empty batch launches nothing, also without keys
    ev.linear_transform(tables, d_ct, k, 0, gk, out)
    # transparency flags: one per output ciphertext
    flags = ctx.alloc(2)
    zeroed = ct.copy()
    zeroed[1] = 0
    d_z = ctx.upload(zeroed)
    ctx.transparency_sink(flags, 4)
    for rescale in (False, True):
        ev.linear_transform(tables, d_z, k, count, gk, out, rescale=rescale)
        f = flags.download().view(np.uint32)[:count]
        assert list(f != 0) == [True, False, True], f
    ctx.transparency_sink(None, 0)
    # graph capture after one warm-up: a replay gives the eager words; creating tables cannot be captured
    ev.linear_transform(tables, d_ct, k, count, gk, out)
    want = out.download().copy()
    graph = ctx.capture(lambda: ev.linear_transform(tables, d_ct, k, count, gk, out))
    ctx.memset_zero(out, out.words * 8)
    graph.launch()
    assert np.array_equal(out.download(), want)
    with pytest.raises(S.LogicError):
        ctx.capture(lambda: S.LinearTransform(ctx, dM, d, scale))
    with pytest.raises(S.LogicError):
        ctx.capture(lambda: ev.linear_transform_diagonals(dM, d))
    # the pool: what the tables took for their making is back, and nothing is held after destroy
    tables.free()
    assert ctx.pool_stats()["bytes_in_use"] == start


def test_cpp_adapter(tmp_path):
    """tests/host_adapter_lintrans_check.cpp: LinearTransform from host and from device memory gives the C ABI's digests;
    the scale bookkeeping; a missing key throws; the decrypted result against M z is printed"""
    exe = compile_cpp(tmp_path, "host_adapter_lintrans_check.cpp", link_sealhip=True)
    mods = O.coeff_modulus_create(1024, [50, 40, 40, 60])
    out = run_exe(exe, "0", *mods, timeout=120)
    print(out)
    assert "lintrans adapter checks ok" in out


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
