"""Matrix-vector products from a caller's matrix (sealhip_linear_transform_* and sealhip_evaluator_linear_transform, DESIGN.md
section 26): what can be checked without a GPU. The planner against the numpy restatement (tests/lintrans_ref.py) and as a
program of its own under the sanitizers; the host twin of the gather kernel bit for bit against the restatement, and the grid
it makes against the defining formula; one end-to-end run on the CPU restatement of the BSGS pipeline with real keys; the
refusals of every entry on a host-only context."""
import ctypes as C
import os

import numpy as np
import pytest

import lintrans_ref as R
import oracle_lib as O
from support import compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_linear_transform_plan", "sealhip_linear_transform_diagonals", "sealhip_linear_transform_values",
       "sealhip_linear_transform_values_host", "sealhip_linear_transform_create", "sealhip_linear_transform_destroy",
       "sealhip_linear_transform_tables_plan", "sealhip_linear_transform_tables_steps", "sealhip_linear_transform_tables_plain",
       "sealhip_evaluator_linear_transform")
LOG_SLOTS = (3, 4, 5, 6)


def _ctx(S, logn, scheme=None, n_primes=4):
    scheme = scheme or S.SCHEME_CKKS
    mods = O.coeff_modulus_create(1 << logn, [40] * n_primes)
    return S.Context(scheme, logn, mods, 1, 0 if scheme == S.SCHEME_CKKS else 65537, device=-1), mods


def _strides(d):
    return [0] + [1 << j for j in range(d.bit_length())]


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS and name in header
    for name in ("linear_transform_plan", "linear_transform_diagonals", "linear_transform_values", "linear_transform"):
        assert callable(getattr(S.Evaluator, name))
    assert callable(S.LinearTransform) and "tests/lintrans_ref.py" in header


@pytest.mark.parametrize("log_slots", LOG_SLOTS)
def test_plan_against_the_restatement(log_slots):
    """every d, every n1 (0 = default), the named masks and 200 seeded random ones per d: the library's plan is the
    restatement's; the steps are sorted and distinct; every c of D sits in exactly one cell; the dense default is
    2^ceil((r+1)/2) (d = 1, r = 0, has the one stride 1)"""
    import sealhip as S

    n = 1 << log_slots
    ctx, mods = _ctx(S, log_slots + 1)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(2600 + log_slots)
    d = 1
    while d <= n:
        for mi, mask in enumerate(R.masks(d, rng, 200)):
            for n1 in _strides(d):
                got = ev.linear_transform_plan(d, None if mi == 0 else mask, n1)
                want = R.plan(n, d, mask, n1)
                for key in ("d", "n_diagonals", "n1", "n_baby", "n_giant", "baby_steps", "giant_steps", "key_steps"):
                    assert got[key] == want[key], (d, n1, mask, key)
                assert got["table_words"] == want["n_baby"] * want["n_giant"] * len(mods) * 2 * n
                for steps in (got["baby_steps"], got["giant_steps"], got["key_steps"]):
                    assert steps == sorted(set(steps))
                cells = [g + b for g in got["giant_steps"] for b in got["baby_steps"]]
                assert len(cells) == len(set(cells)) and all(c < d for c in cells)
                assert all(cells.count(c) == 1 for c in range(d) if mask[c])
                if mi == 0 and n1 == 0 and d >= 2:
                    r = d.bit_length() - 1
                    assert got["n1"] == 1 << ((r + 2) // 2)  # 2^ceil((r+1)/2), the homomorphic DFT's default
        d *= 2
    assert ev.linear_transform_plan(1)["n1"] == 1


def test_planner_program_under_sanitizers(tmp_path):
    """gemini-seal_amd/csrc/lintrans_plan.hpp compiled for the host with AddressSanitizer and UBSan into a program of its
    own: its sweep, then a few plans printed and compared with the restatement's"""
    exe = compile_cpp(tmp_path, "lintrans_plan_check.cpp", sanitize=True)
    assert "lintrans_plan_check: OK" in run_exe(exe, timeout=300)
    rng = np.random.default_rng(5)
    for log_slots, d in ((3, 8), (5, 16), (6, 64), (6, 1)):
        for mask in R.masks(d, rng, 3):
            for n1 in (0, 1, d):
                p = R.plan(1 << log_slots, d, mask, n1)
                line = run_exe(exe, log_slots, d, n1, "".join(str(int(v)) for v in mask), timeout=60).split()
                want = (["n1", str(p["n1"]), "baby"] + [str(s) for s in p["baby_steps"]] + ["giant"] +
                        [str(s) for s in p["giant_steps"]] + ["keys"] + [str(s) for s in p["key_steps"]])
                assert line == want


@pytest.mark.parametrize("log_slots", LOG_SLOTS)
def test_host_values_bits_and_the_defining_formula(log_slots):
    """sealhip_linear_transform_values_host on a host-only context: the bits of the restatement (a -0.0 and signed gains
    included), and the grid applied by rotations, sum_g rot(sum_b values[g][b] * rot(z, b), g), is gain times the defining
    formula within 2^-40 |gain| sum_c |u_c[p]| |z[(p + c) mod n]| per slot -- for a d-periodic z that is
    2^-40 |gain| sum_j |M_ij| |z_j|, the bound of the DFT generator's test for the same kind of sum -- for periodic and
    non-periodic z."""
    import sealhip as S

    n = 1 << log_slots
    ctx, _ = _ctx(S, log_slots + 1)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(2700 + log_slots)
    worst = 0.0
    d = 1
    while d <= n:
        for mask in R.masks(d, rng, 4):
            M = R.masked_matrix(d, mask, rng)
            c0 = int(np.flatnonzero(mask)[0])
            if d > 1:
                M[1, (1 + c0) % d] = complex(-0.0, 2.5)  # a -0.0 on a diagonal in use
            for n1 in _strides(d):
                for gain in (1.0, -0.8125, 3.0e-3):
                    got = ev.linear_transform_values(M, d, mask, n1, gain, host=True)
                    want, pl = R.values(M, n, mask, n1, gain)
                    assert got.shape == want.shape
                    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (d, n1, gain)
                    tile = rng.normal(size=d) + 1j * rng.normal(size=d)
                    for z in (np.tile(tile, n // d), rng.normal(size=n) + 1j * rng.normal(size=n)):
                        ref = R.apply_definition(M, z, mask)
                        bar = 2.0 ** -40 * abs(gain) * R.apply_definition(np.abs(M), np.abs(z), mask).real
                        err = np.abs(R.apply_grid(got, pl["baby_steps"], pl["giant_steps"], z) - gain * ref)
                        assert np.all(err <= bar), (d, n1, gain, float(np.max(err)))
                        worst = max(worst, float(np.max(err / np.maximum(bar, 1e-300))))
                    if d > 1:
                        Mz = (M @ tile) * gain
                        full = R.apply_grid(got, pl["baby_steps"], pl["giant_steps"], np.tile(tile, n // d))
                        assert np.allclose(full, np.tile(Mz, n // d), rtol=0, atol=1e-9 * np.max(np.abs(Mz)) + 1e-300)
        d *= 2
    print("log n %d: grid against the defining formula, worst error / bar = %.3g" % (log_slots, worst))


def test_end_to_end_on_the_cpu():
    """N = 64 over tests/hoist_bsgs_ref.py with real keys, the oracle's encoder and decryptor: a dense 32 x 32 matrix at the
    default stride (8 babies, 4 giants) against the same diagonals un-grouped (n1 = d: every diagonal a baby, no giant). The
    BSGS result's error against the defining formula is at most 8 times the un-grouped sum's in the same run (the factor
    allows for the giants' extra half mod-downs)."""
    import sealhip as S

    import hoist_bsgs_ref as HB
    import hoist_ref as H

    logn, N, n, delta = 6, 64, 32, 2.0 ** 40
    mods = O.coeff_modulus_create(N, [50, 40, 40, 60])
    ref = O.RefContext(2, logn, mods, nsp=1, t=0)
    cl = O.Client(ref, seed=11)
    enc = O.CkksRef(ref)
    L = O.lib()
    host, _ = _ctx(S, logn)
    ev = S.Evaluator(host)
    rng = np.random.default_rng(26)
    d, k = 32, 3
    M = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    z = rng.normal(size=n) + 1j * rng.normal(size=n)
    want = R.apply_definition(M, z)
    rc, plain = enc.encode(z, k, delta)
    assert rc == 0
    ct = np.zeros((2, k, N), dtype=np.uint64)
    L.ref_encrypt_zero_symmetric(C.byref(ref.c), k, O.ptr(cl.sk), 1, C.byref(cl.state), O.ptr(ct))
    for r in range(k):
        L.ref_add_poly_coeffmod(O.ptr(ct[0, r]), O.ptr(plain[r]), N, C.byref(ref.c.key_mod[r]), O.ptr(ct[0, r]))
    keys = {}

    def key(g):
        if g != 1 and g not in keys:
            keys[g] = cl.galois_key(g)
        return keys.get(g)

    errs = {}
    for name, n1 in (("bsgs", 0), ("ungrouped", d)):
        W = ev.linear_transform_values(M, d, None, n1, host=True)
        pl = ev.linear_transform_plan(d, None, n1)
        assert (pl["n_baby"], pl["n_giant"]) == ((8, 4) if n1 == 0 else (32, 1))
        plains = np.zeros(W.shape[:2] + (len(mods), N), dtype=np.uint64)
        for g in range(W.shape[0]):
            for b in range(W.shape[1]):
                rc, plains[g, b] = enc.encode(W[g, b], len(mods), delta)
                assert rc == 0
        be = [1 if s == 0 else H.elt_from_step(N, s) for s in pl["baby_steps"]]
        ge = [1 if s == 0 else H.elt_from_step(N, s) for s in pl["giant_steps"]]
        out = HB.bsgs(ref, k, ct[None], be, [key(g) for g in be], ge, [key(g) for g in ge], plains)[0]
        dot = np.zeros((k, N), dtype=np.uint64)
        L.ref_dot_product_ct_sk(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(out)), 2, 1, O.ptr(cl.sk_powers(1)), O.ptr(dot))
        errs[name] = float(np.max(np.abs(enc.decode(dot, delta * delta) - want)))
    print("CPU end to end, N = 64, dense d = 32: max slot error BSGS %.3g, un-grouped %.3g (max |M z| %.3g)"
          % (errs["bsgs"], errs["ungrouped"], float(np.max(np.abs(want)))))
    assert errs["ungrouped"] < 2.0 ** -20 * float(np.max(np.abs(want)))  # (the run means something)
    assert errs["bsgs"] <= 8 * errs["ungrouped"]


def test_refusals_on_host_only_contexts():
    """E_POINTER first; then the argument errors, E_INVALIDARG on a host-only context: BFV, a d that is no power of two in
    [1, n], a bad n1, an empty mask, a bad gain, a short capacity, a misaligned matrix; the device entries refuse a host-only
    context (COR_E_INVALIDOPERATION) only after those"""
    import sealhip as S

    ctx, mods = _ctx(S, 6)  # n = 32
    ev = S.Evaluator(ctx)
    L = S.lib()
    plan = S.LintransPlan()
    E = lambda hr: hr & 0xFFFFFFFF
    buf = np.zeros(2 * 32 * 32 * 8 + 2, dtype=np.float64)
    if buf.ctypes.data % 16:
        buf = buf[1:]
    p, odd = buf.ctypes.data, buf.ctypes.data + 8
    mask8 = np.ones(8, dtype=np.uint8)
    handle = C.c_void_p()
    assert E(L.sealhip_linear_transform_plan(None, 8, None, 0, C.addressof(plan), None, None, None, 0)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_plan(ctx.handle, 8, None, 0, None, None, None, None, 0)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_diagonals(ctx.handle, None, 8, mask8.ctypes.data)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_diagonals(ctx.handle, p, 8, None)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_values(ctx.handle, None, 8, None, 0, 1.0, p)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_values(ctx.handle, p, 8, None, 0, 1.0, None)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_values_host(ctx.handle, None, 8, None, 0, 1.0, p)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_create(ctx.handle, None, 8, 0, 2.0 ** 30, 1.0, C.byref(handle))) == S.E_POINTER
    assert E(L.sealhip_linear_transform_create(ctx.handle, p, 8, 0, 2.0 ** 30, 1.0, None)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_destroy(None)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_tables_plan(None, C.addressof(plan), None)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_tables_steps(None, None, None)) == S.E_POINTER
    assert E(L.sealhip_linear_transform_tables_plain(None, C.byref(handle))) == S.E_POINTER
    assert E(L.sealhip_evaluator_linear_transform(ctx.handle, None, 2, p, 1, None, None, 0, 0, p)) == S.E_POINTER
    for d in (0, 3, 6, 64):
        with pytest.raises(ValueError, match="power of two"):
            ev.linear_transform_plan(d)
        assert E(L.sealhip_linear_transform_diagonals(ctx.handle, p, d, mask8.ctypes.data)) == S.E_INVALIDARG
        assert E(L.sealhip_linear_transform_values(ctx.handle, p, d, None, 0, 1.0, p)) == S.E_INVALIDARG
        assert E(L.sealhip_linear_transform_values_host(ctx.handle, p, d, None, 0, 1.0, p)) == S.E_INVALIDARG
        assert E(L.sealhip_linear_transform_create(ctx.handle, p, d, 0, 2.0 ** 30, 1.0, C.byref(handle))) == S.E_INVALIDARG
    for n1 in (3, 16, 6):
        with pytest.raises(ValueError, match="n1"):
            ev.linear_transform_plan(8, None, n1)
        assert E(L.sealhip_linear_transform_create(ctx.handle, p, 8, n1, 2.0 ** 30, 1.0, C.byref(handle))) == S.E_INVALIDARG
    with pytest.raises(ValueError, match="transparent"):
        ev.linear_transform_plan(8, np.zeros(8))
    with pytest.raises(ValueError, match="transparent"):
        ev.linear_transform_values(np.zeros((8, 8)), 8, np.zeros(8), host=True)
    steps = (C.c_int32 * 8)()
    assert E(L.sealhip_linear_transform_plan(ctx.handle, 8, None, 2, C.addressof(plan), steps, None, None, 1)) == S.E_INVALIDARG
    assert E(L.sealhip_linear_transform_plan(ctx.handle, 8, None, 2, C.addressof(plan), steps, None, None, 2)) == S.S_OK
    assert (plan.n_baby, plan.n_giant, list(steps[:2])) == (2, 4, [0, 1])
    for gain in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="gain"):
            ev.linear_transform_values(np.eye(8), 8, gain=gain, host=True)
        assert E(L.sealhip_linear_transform_values(ctx.handle, p, 8, None, 0, gain, p)) == S.E_INVALIDARG
        assert E(L.sealhip_linear_transform_create(ctx.handle, p, 8, 0, 2.0 ** 30, gain, C.byref(handle))) == S.E_INVALIDARG
    assert E(L.sealhip_linear_transform_diagonals(ctx.handle, odd, 8, mask8.ctypes.data)) == S.E_INVALIDARG
    assert E(L.sealhip_linear_transform_values(ctx.handle, odd, 8, None, 0, 1.0, p)) == S.E_INVALIDARG
    assert E(L.sealhip_linear_transform_values(ctx.handle, p, 8, None, 0, 1.0, odd)) == S.E_INVALIDARG
    assert E(L.sealhip_linear_transform_create(ctx.handle, odd, 8, 0, 2.0 ** 30, 1.0, C.byref(handle))) == S.E_INVALIDARG
    bfv, _ = _ctx(S, 6, scheme=S.SCHEME_BFV)
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).linear_transform_plan(8)
    with pytest.raises(ValueError, match="CKKS only"):
        S.Evaluator(bfv).linear_transform_values(np.eye(8), 8, host=True)
    assert E(L.sealhip_linear_transform_create(bfv.handle, p, 8, 0, 2.0 ** 30, 1.0, C.byref(handle))) == S.E_INVALIDARG
    assert E(L.sealhip_linear_transform_diagonals(bfv.handle, p, 8, mask8.ctypes.data)) == S.E_INVALIDARG
    # argument errors first, then the device
    assert E(L.sealhip_linear_transform_diagonals(ctx.handle, p, 8, mask8.ctypes.data)) == S.COR_E_INVALIDOPERATION
    assert E(L.sealhip_linear_transform_values(ctx.handle, p, 8, None, 0, 1.0, p)) == S.COR_E_INVALIDOPERATION
    assert E(L.sealhip_linear_transform_create(ctx.handle, p, 8, 0, 2.0 ** 30, 1.0, C.byref(handle))) == S.COR_E_INVALIDOPERATION
    assert not handle.value


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_lintrans_check.cpp", link_sealhip=True)
    assert "host-only lintrans checks ok" in run_exe(exe, "host", timeout=120)
