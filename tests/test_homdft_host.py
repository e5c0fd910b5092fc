"""Homomorphic DFT (sealhip_evaluator_coeffs_to_slots / _slots_to_coeffs and the sealhip_dft_* entries):
what can be checked without a GPU. The numpy restatement (tests/homdft_ref.py) builds every stage from its butterfly LAYERS; here
the factorisation it rests on is checked against the encoder's embedding, the library's plan against what is read off those
matrices, the BSGS grid against M v, and the host restatement of the generator (the closed form the kernel evaluates) against
the layer products. Then the refusals on host-only contexts, and the planner header under the sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

import homdft_ref as R
import oracle_lib as O
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_evaluator_dft_plan", "sealhip_dft_stage_steps", "sealhip_dft_stage_values", "sealhip_dft_stage_values_host",
       "sealhip_dft_tables_create", "sealhip_dft_tables_destroy", "sealhip_dft_tables_plan", "sealhip_dft_tables_stage",
       "sealhip_evaluator_coeffs_to_slots", "sealhip_evaluator_slots_to_coeffs")
LOGNS = (4, 5, 6, 7, 8)


def _ctx(S, logn, scheme=None, n_primes=5):
    mods = O.coeff_modulus_create(1 << logn, [40] * n_primes)
    return S.Context(scheme or S.SCHEME_CKKS, logn, mods, 1, 0 if (scheme or S.SCHEME_CKKS) == S.SCHEME_CKKS else 65537, device=-1), mods


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("dft_plan", "dft_stage_values", "coeffs_to_slots", "slots_to_coeffs"):
        assert callable(getattr(S.Evaluator, name))
    assert callable(S.DftTables)
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert name in header
    assert "tests/homdft_ref.py" in header


@pytest.mark.parametrize("logn", LOGNS)
def test_factorisation_of_the_embedding(logn):
    """F_L ... F_1 R = U, U U^H = n I, and G z = R w for G = F_1^-1 ... F_L^-1: the definitions everything else rests on"""
    N, n, L = 1 << logn, 1 << (logn - 1), logn - 1
    U = R.embedding(N)
    assert np.allclose(U @ U.conj().T, n * np.eye(n), atol=1e-9)
    prod = np.eye(n, dtype=np.complex128)[R.bitrev_perm(n)]  # R as a matrix: (R w)_j = w_(bitrev j)
    for s in range(1, L + 1):
        assert np.allclose(R.apply_layer(np.eye(n, dtype=np.complex128), s), R.layer(n, s), atol=0)
        prod = R.layer(n, s) @ prod
    assert np.max(np.abs(prod - U)) < 1e-11
    rng = np.random.default_rng(logn)
    w = rng.normal(size=n) + 1j * rng.normal(size=n)
    z = U @ w
    for s in range(L, 0, -1):
        z = R.apply_layer(z, s, inverse=True)
    assert np.max(np.abs(z - w[R.bitrev_perm(n)])) < 1e-12
    # multiplying the polynomial by X^(N/2) multiplies every slot by i; element 2N - 1 conjugates
    m = rng.normal(size=N)
    slots = U @ (m[:n] + 1j * m[n:])
    mi = np.concatenate([-m[n:], m[:n]])
    assert np.allclose(U @ (mi[:n] + 1j * mi[n:]), 1j * slots)
    assert np.allclose(np.array([sum(m[t] * np.exp(1j * np.pi * ((2 * N - p) % (2 * N)) * t / N) for t in range(N))
                                 for p in R.pow5(N)[:4]]), np.conj(slots[:4]))


@pytest.mark.parametrize("logn", LOGNS)
def test_plan_grid_and_host_values_for_every_split(logn):
    """Every split of L into up to three stages, both directions: the stages' product is the transform; the plan's shape,
    folded top stage, step lists and diagonal sets are those read off the layer products; the BSGS grid applied by rotations
    is M v; and sealhip_dft_stage_values_host is within 2^-40 gain 2^(-r or 0) of the grid read off the matrix (an entry is a
    product of at most r + 1 table roots at 2^-52 relative error each)."""
    import sealhip as S

    N, n, L = 1 << logn, 1 << (logn - 1), logn - 1
    ctx, mods = _ctx(S, logn)
    ev = S.Evaluator(ctx)
    k, gain = 4, 0.8125
    rng = np.random.default_rng(100 + logn)
    v = rng.normal(size=n) + 1j * rng.normal(size=n)
    U = R.embedding(N)
    perm = R.bitrev_perm(n)
    worst = 0.0
    for counts in R.compositions(L, 3):
        for direction in (R.C2S, R.S2C):
            plan = ev.dft_plan(direction, k, counts)
            layout = R.stage_layout(N, direction, counts)
            assert plan["in_level"] == k and plan["out_level"] == k - len(counts)
            assert plan["needs_conjugation"] == (1 if direction == R.C2S else 0)
            total, steps, words = np.eye(n, dtype=np.complex128), set(), 0
            for t, (s0, r) in enumerate(layout):
                st = plan["stages"][t]
                M = R.stage_matrix(N, direction, s0, r)
                total = M @ total
                folded = (1 << (s0 - 1 + r)) == n
                assert (st["s0"], st["r"], st["h0"], st["level"], st["folded"]) == (s0, r, 1 << (s0 - 1), k - t, int(folded))
                assert st["scale"] == float(mods[k - t - 1])
                assert st["n_baby"] == R.default_n_baby(r) and st["n_baby"] * st["n_giant"] == (1 << r if folded else 2 << r)
                # the diagonals the matrix has: every signed c of (-2^r, 2^r), folded modulo 2^r when the stage is the top
                diags = R.read_diagonals(M, s0, r)
                assert set(diags) == set(range(-(1 << r) + 1, 1 << r))
                W, baby, giant = R.bsgs_grid(M, s0, r)
                assert st["baby_steps"] == baby and st["giant_steps"] == giant
                cells = {((g if folded else g - st["n_giant"] // 2) * st["n_baby"] + b)
                         for g in range(st["n_giant"]) for b in range(st["n_baby"])}
                assert cells == ({c % (1 << r) for c in diags} if folded else set(diags) | {-(1 << r)})
                if not folded:
                    assert not np.any(W[0, 0])  # the one empty cell, c = -2^r
                assert np.max(np.abs(R.bsgs_apply(W, baby, giant, v) - M @ v)) < 1e-12 * (1 << r)
                steps |= {s for s in baby + giant if s}
                words += W.shape[0] * W.shape[1] * len(mods) * N
                # the closed form against the layers
                got = ev.dft_stage_values(direction, k, counts, t, gain=gain, host=True)
                f = R.stage_gain(direction, t, len(counts), gain)
                bar = 2.0 ** -40 * abs(f) * (2.0 ** -r if direction == R.C2S else 1.0)
                err = np.max(np.abs(got - W * f))
                worst = max(worst, err / bar)
                assert err <= bar, (counts, direction, t, err, bar)
                assert np.array_equal(got == 0, W == 0)
            assert plan["key_steps"] == sorted(steps) and plan["table_words"] == words
            if direction == R.S2C:
                assert np.max(np.abs(total @ np.eye(n)[perm] - U)) < 1e-10
            else:
                assert np.max(np.abs(total @ U - np.eye(n)[perm])) < 1e-10
    print("logn %d: host generator's worst error / bar = %.3g" % (logn, worst))


def test_n_baby_override_and_gain():
    import sealhip as S

    ctx, _ = _ctx(S, 6)
    ev = S.Evaluator(ctx)
    for direction in (R.C2S, R.S2C):
        for n_baby in ([1, 2], [8, 4], [2, 1]):
            plan = ev.dft_plan(direction, 3, [3, 2], n_baby=n_baby)
            for t in range(2):
                s0, r = R.stage_layout(64, direction, [3, 2])[t]
                W, baby, giant = R.bsgs_grid(R.stage_matrix(64, direction, s0, r), s0, r, n_baby[t])
                assert plan["stages"][t]["baby_steps"] == baby and plan["stages"][t]["giant_steps"] == giant
                got = ev.dft_stage_values(direction, 3, [3, 2], t, n_baby=n_baby, gain=-3.0, host=True)
                want = R.stage_values(64, direction, [3, 2], t, n_baby=n_baby, gain=-3.0)
                assert np.max(np.abs(got - want)) <= 2.0 ** -40 * 3.0


def test_refusals_on_host_only_contexts():
    """E_POINTER first; the plan's refusals are E_INVALIDARG on a host-only context: layer counts not summing to L, a zero
    count, more stages than levels below k, k outside the ciphertext levels, a bad n_baby, BFV. The device entries then
    refuse a host-only context (COR_E_INVALIDOPERATION) only after those."""
    import sealhip as S

    ctx, mods = _ctx(S, 6)  # L = 5, first level 4
    ev = S.Evaluator(ctx)
    L = S.lib()
    plan = S.DftPlan()
    arr = lambda *v: (C.c_uint32 * len(v))(*v)
    assert L.sealhip_evaluator_dft_plan(None, 0, 3, arr(5), 1, None, C.addressof(plan), None, 0) & 0xFFFFFFFF == S.E_POINTER
    assert L.sealhip_evaluator_dft_plan(ctx.handle, 0, 3, arr(5), 1, None, None, None, 0) & 0xFFFFFFFF == S.E_POINTER
    for direction in (R.C2S, R.S2C):
        for bad in ([4], [3, 3], [5, 1], [2, 0, 3], []):
            with pytest.raises(ValueError):
                ev.dft_plan(direction, 4, bad)
        with pytest.raises(ValueError, match="more stages than levels"):
            ev.dft_plan(direction, 3, [2, 2, 1])
        with pytest.raises(ValueError, match="more stages than levels"):
            ev.dft_plan(direction, 1, [5])
        for k in (0, 5, 6):
            with pytest.raises(ValueError):
                ev.dft_plan(direction, k, [5])
        for n_baby in ([3], [64]):
            with pytest.raises(ValueError, match="n_baby"):
                ev.dft_plan(direction, 4, [5], n_baby=n_baby)
        assert ev.dft_plan(direction, 4, [2, 2, 1])["out_level"] == 1
    with pytest.raises(ValueError):
        ev.dft_plan(2, 4, [5])
    steps = arr(*([0] * 64))
    assert L.sealhip_evaluator_dft_plan(ctx.handle, 0, 4, arr(5), 1, None, C.addressof(plan), steps, 1) & 0xFFFFFFFF == S.E_INVALIDARG
    bfv, _ = _ctx(S, 6, scheme=S.SCHEME_BFV)
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).dft_plan(0, 3, [5])
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).dft_stage_values(0, 3, [5], 0, host=True)
    with pytest.raises(ValueError, match="CKKS only"):
        S.DftTables(bfv, 0, 3, [5])
    # stage out of range, gain
    buf = np.zeros(4, dtype=np.complex128)
    with pytest.raises(ValueError, match="stage out of range"):
        S._check(L.sealhip_dft_stage_values_host(ctx.handle, 0, 4, arr(3, 2), 2, None, 1.0, 2, buf.ctypes.data))
    for gain in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="gain"):
            ev.dft_stage_values(0, 4, [5], 0, gain=gain, host=True)
        with pytest.raises(ValueError, match="gain"):
            S.DftTables(ctx, 0, 4, [5], gain=gain)
    # argument errors first, then the device
    with pytest.raises(ValueError):
        S.DftTables(ctx, 0, 4, [4])
    with pytest.raises(S.LogicError):
        S.DftTables(ctx, 0, 4, [5])
    with pytest.raises(S.LogicError):
        ev.dft_stage_values(0, 4, [5], 0)
    p = np.zeros(8, dtype=np.uint64).ctypes.data
    assert L.sealhip_evaluator_coeffs_to_slots(ctx.handle, None, p, 1, None, None, 0, p, p) & 0xFFFFFFFF == S.E_POINTER
    assert L.sealhip_evaluator_slots_to_coeffs(ctx.handle, None, p, p, 1, None, None, 0, p) & 0xFFFFFFFF == S.E_POINTER
    assert L.sealhip_dft_tables_destroy(None) & 0xFFFFFFFF == S.E_POINTER


def test_planner_program_under_sanitizers(tmp_path):
    """gemini-seal_amd/csrc/homdft_plan.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = compile_cpp(tmp_path, "homdft_plan_check.cpp", sanitize=True)
    assert "homdft_plan_check: OK" in run_exe(exe, timeout=300)


def test_reference_chain_decrypts_on_the_cpu():
    """The chain the GPU end-to-end test measures against, at N = 2^6 on the CPU restatement (tests/ks_rescale_ref.py) with
    real keys: numpy-made, oracle-encoded diagonals; Delta = 2^40, q_0 of 50 bits, 40-bit primes and a
    special prime of 60 bits. CoeffToSlot [3,2] from level 5 to 3 puts m_(bitrev j) / Delta and m_(bitrev j + n) / Delta into the slots;
    SlotToCoeff [2,3] from 3 to 1 returns the message; both to better than 2^-16 max|m| / Delta."""
    import hoist_ref as H
    import ks_rescale_ref as KR

    logn, N, n, delta = 6, 64, 32, 2.0 ** 40
    mods = O.coeff_modulus_create(N, [50, 40, 40, 40, 40, 60])
    ref = O.RefContext(2, logn, mods, nsp=1, t=0)
    cl = O.Client(ref, seed=7)
    enc = O.CkksRef(ref)
    L = O.lib()
    rng = np.random.default_rng(3)
    m = rng.integers(-(1 << 39), 1 << 39, size=N).astype(np.int64)
    bound = 2.0 ** -16 * float(np.max(np.abs(m))) / delta
    keys = {}

    def key(g):
        if g != 1 and g not in keys:
            keys[g] = cl.galois_key(g)
        return keys.get(g)

    def chain(cts, direction, counts, k):
        for t, (s0, r) in enumerate(R.stage_layout(N, direction, counts)):
            W, baby, giant = R.bsgs_grid(R.stage_matrix(N, direction, s0, r), s0, r)
            W = W * R.stage_gain(direction, t, len(counts))
            plains = np.zeros(W.shape[:2] + (len(mods), N), dtype=np.uint64)
            for g in range(W.shape[0]):
                for b in range(W.shape[1]):
                    rc, plains[g, b] = enc.encode(W[g, b], len(mods), float(mods[k - t - 1]))
                    assert rc == 0
            be = [1 if s == 0 else H.elt_from_step(N, s) for s in baby]
            ge = [1 if s == 0 else H.elt_from_step(N, s) for s in giant]
            cts = KR.bsgs_plain_rescale(ref, k - t, cts, be, [key(g) for g in be], ge, [key(g) for g in ge], plains)
        return cts

    def decrypt(ct, k):
        dot = np.zeros((k, N), dtype=np.uint64)
        L.ref_dot_product_ct_sk(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(ct)), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
        return dot

    ct = cl.encrypt_poly_ntt([int(v) for v in m])[None]
    mid = chain(ct, R.C2S, [3, 2], 5)[0]
    conj = mid.copy()
    assert L.ref_apply_galois_inplace(C.byref(ref.c), 3, O.ptr(conj), 2 * N - 1, O.ptr(key(2 * N - 1))) == 0
    xh = np.zeros((3, N), dtype=np.uint64)
    xh[:, N // 2] = 1
    for r in range(3):
        L.ref_ntt_forward(O.ptr(xh[r]), ref.tables(r), 0)
    re, diff, im, merged = (np.zeros_like(mid) for _ in range(4))
    L.ref_evaluator_add(C.byref(ref.c), 3, O.ptr(mid), 2, O.ptr(conj), 2, O.ptr(re))
    L.ref_evaluator_sub(C.byref(ref.c), 3, O.ptr(conj), 2, O.ptr(mid), 2, O.ptr(diff))
    for p in range(2):
        for r in range(3):
            L.ref_dyadic_product_coeffmod(O.ptr(diff[p, r]), O.ptr(xh[r]), N, C.byref(ref.c.key_mod[r]), O.ptr(im[p, r]))
    perm = R.bitrev_perm(n)
    zr, zi = enc.decode(decrypt(re, 3), delta), enc.decode(decrypt(im, 3), delta)
    err = max(np.max(np.abs(zr - m[perm] / delta)), np.max(np.abs(zi - m[perm + n] / delta)))
    print("CPU reference chain, N = 64: CoeffToSlot max slot error %.3g (bound %.3g)" % (err, bound))
    assert err < bound
    for p in range(2):
        for r in range(3):
            L.ref_dyadic_product_coeffmod(O.ptr(im[p, r]), O.ptr(xh[r]), N, C.byref(ref.c.key_mod[r]), O.ptr(merged[p, r]))
    L.ref_evaluator_add(C.byref(ref.c), 3, O.ptr(re), 2, O.ptr(merged), 2, O.ptr(merged))
    back = chain(merged[None], R.S2C, [2, 3], 3)[0]
    vals, _ = cl.centered_from_ntt_rows(decrypt(back, 1))
    err = max(abs(int(a) - int(b)) for a, b in zip(vals, m)) / delta
    print("CPU reference chain, N = 64: round trip max coefficient error / Delta %.3g (bound %.3g)" % (err, bound))
    assert err < bound


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_homdft_check.cpp", link_sealhip=True)
    assert "host-only homdft checks ok" in run_exe(exe, "host", timeout=120)
