"""RGSW ciphertexts, the external product, CMux and the CMux tree (sealhip_generate_rgsw, sealhip_rgsw_*,
sealhip_evaluator_external_product / _cmux / _select): what can be checked without a GPU. The
restatement of tests/rgsw_ref.py against the definition (decryption under real keys, the phase in Python integers), the
argument checks of every entry on host-only contexts in the header's order, the 128-bit capacity of the inner product's
accumulators (tests/ext_mac_bounds_check.cpp), the selector (tests/ext_select_check.cpp against the rule restated here)
and the C++ adapter's own checks (tests/host_adapter_rgsw_check.cpp)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import rgsw_ref as G
from support import CSRC, compile_cpp, run_exe

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("sealhip_generate_rgsw", "sealhip_rgsw_create", "sealhip_rgsw_export", "sealhip_rgsw_destroy",
       "sealhip_evaluator_external_product", "sealhip_evaluator_cmux", "sealhip_evaluator_select", "sealhip_debug_ext_mac_plan")
LOGN, N = 4, 16
CASES_16 = {"bfv": (1, [30, 35, 40, 45, 50], 1, 65537), "ckks": (2, [40] * 5 + [41] * 2, 2, 0)}
NOISE_MAX = 41  # the largest |e| a key's error polynomial can have (the clipped Gaussian's bound, and the tests' samples)


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    header = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in S.SYMBOLS and name in header
    for name in ("external_product", "cmux", "select"):
        assert callable(getattr(S.Evaluator, name))
    for name in ("generate_rgsw", "rgsw_create", "rgsw_export", "debug_ext_mac_plan"):
        assert callable(getattr(S.Context, name))
    assert isinstance(S.Rgsw, type)


# ---------------------------------------------------------------- the restatement against the definition
_sessions = {}


def session(name):
    if name not in _sessions:
        scheme, bits, nsp, t = CASES_16[name]
        mods = O.coeff_modulus_create(N, bits)
        ref = O.RefContext(scheme, LOGN, mods, nsp=nsp, t=t, mode=1)
        _sessions[name] = (mods, ref, O.Client(ref, seed=29))
    return _sessions[name]


def fresh(name, seed):
    """a client of its own: what a test measures must not depend on which tests drew from the shared client before it"""
    scheme, bits, nsp, t = CASES_16[name]
    mods = O.coeff_modulus_create(N, bits)
    ref = O.RefContext(scheme, LOGN, mods, nsp=nsp, t=t, mode=1)
    return mods, ref, O.Client(ref, seed=seed)


def messages():
    """0, 1, -1, X, -X^(N-1) and one ternary polynomial"""
    zero = np.zeros(N, dtype=np.int8)
    tern = np.random.default_rng(29).integers(-1, 2, size=N).astype(np.int8)
    return {"0": zero, "1": G.monomial(N, 0), "-1": G.monomial(N, 0, -1), "X": G.monomial(N, 1), "-X^(N-1)": G.monomial(N, N - 1, -1),
            "ternary": tern}


def ks_error_bound(ref, k):
    """|e_ks| of ONE external product at level k. Digit j's term is <D_j, e_j> / P with |D_j| below nsp B_j (B_j the
    bundle's modulus; the fast base conversion of the mod-up may add up to nsp - 1 multiples of it), |e_j| <= NOISE_MAX and N
    coefficients: 2 nd terms of N * NOISE_MAX * nsp * B_j / P; the mod-down rounds each of the two components by at most
    nsp, and c_1's rounding meets the ternary secret: (1 + N) * nsp."""
    nsp = ref.nsp
    nd = (k + nsp - 1) // nsp
    P = 1
    for p in ref.key_moduli[ref.k_first:]:
        P *= p
    total = 0
    for j in range(nd):
        B = 1
        for p in ref.key_moduli[j * nsp:min((j + 1) * nsp, k)]:
            B *= p
        total += 2 * N * NOISE_MAX * nsp * -(-B // P)
    return total + (1 + N) * nsp


@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_external_product_multiplies_the_phase(name):
    """for every message: the phase of ct (x) RGSW(m) is m * phase(ct) up to one key switch's error, with and without a
    base, at the first level and at level 1; BFV decrypts to m * plain exactly"""
    mods, ref, cl = session(name)
    scheme, _, _, t = CASES_16[name]
    rng = np.random.default_rng(4)
    for tag, m in messages().items():
        g = G.rgsw(cl, m)
        if scheme == 1:
            plain = rng.integers(0, t, size=N, dtype=np.uint64)
            ct, base_plain = cl.encrypt_bfv(plain), rng.integers(0, t, size=N, dtype=np.uint64)
            base = cl.encrypt_bfv(base_plain)
        else:
            msg = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
            ct, base = cl.encrypt_poly_ntt(msg), cl.encrypt_poly_ntt(msg[::-1])
        for k in (cl.k, 1):
            c, b = np.ascontiguousarray(ct[:, :k]), np.ascontiguousarray(base[:, :k])
            for with_base in (False, True):
                out = G.external_product(ref, k, c, g, base=b if with_base else None)
                err = G.phase_error(cl, out, c, m, scheme == 2, base=b if with_base else None)
                assert err <= ks_error_bound(ref, k), (name, tag, k, with_base, err)
        if scheme == 1:
            want = O.negacyclic_mod_t([int(v) % t for v in m], [int(v) for v in plain], t)
            assert cl.decrypt_bfv(G.external_product(ref, cl.k, ct, g)).tolist() == [int(v) for v in want], (name, tag)
            both = [(a + b) % t for a, b in zip(want, base_plain.tolist())]
            assert cl.decrypt_bfv(G.external_product(ref, cl.k, ct, g, base=base)).tolist() == [int(v) for v in both], (name, tag)


def ckks_rel_error(cl, out, want, scale_of):
    got, _ = G.phase(cl, out, True)
    return max(abs(a - b) for a, b in zip(got, want)) / max(abs(v) for v in scale_of)


@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_cmux_picks_the_operand(name):
    mods, ref, cl = fresh(name, 41)
    scheme, _, _, t = CASES_16[name]
    rng = np.random.default_rng(5)
    for bit in (0, 1):
        g = G.rgsw(cl, G.monomial(N, 0) * bit)
        if scheme == 1:
            plains = rng.integers(0, t, size=(2, N), dtype=np.uint64)
            out = G.cmux(ref, mods, cl.k, cl.encrypt_bfv(plains[0]), cl.encrypt_bfv(plains[1]), g)
            assert np.array_equal(cl.decrypt_bfv(out), plains[bit]), bit
        else:
            msgs = [[int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)] for _ in range(2)]
            out = G.cmux(ref, mods, cl.k, cl.encrypt_poly_ntt(msgs[0]), cl.encrypt_poly_ntt(msgs[1]), g)
            assert ckks_rel_error(cl, out, msgs[bit], msgs[0] + msgs[1]) <= G.CKKS_REL_MEASURED, bit  # (one level of the tree's three)


@pytest.mark.parametrize("name", ["bfv", "ckks"])
def test_tree_picks_each_of_its_8_leaves(name):
    mods, ref, cl = fresh(name, 31)
    scheme, _, _, t = CASES_16[name]
    rng = np.random.default_rng(6)
    one, zero = G.rgsw(cl, G.monomial(N, 0)), G.rgsw(cl, np.zeros(N, dtype=np.int8))
    if scheme == 1:
        plains = rng.integers(0, t, size=(8, N), dtype=np.uint64)
        cts = [cl.encrypt_bfv(p) for p in plains]
    else:
        plains = [[int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)] for _ in range(8)]
        cts = [cl.encrypt_poly_ntt(p) for p in plains]
    worst = 0.0
    for idx in range(8):
        out = G.select(ref, mods, cl.k, cts, [one if (idx >> b) & 1 else zero for b in range(3)])
        if scheme == 1:
            assert np.array_equal(cl.decrypt_bfv(out), plains[idx]), idx
        else:
            worst = max(worst, ckks_rel_error(cl, out, plains[idx], [v for p in plains for v in p]))
    if scheme == 2:
        print("ckks restatement select(l = 3): relative error 2^%.1f (%r)" % (np.log2(worst) if worst else -np.inf, worst))
        assert worst == G.CKKS_REL_MEASURED, worst  # (the recorded figure IS this measurement)


def test_restatement_ckks_error():
    """the figure rgsw_ref.CKKS_REL_MEASURED records: the external product by X^3 (the phase rotates) at scale 2^40"""
    mods, ref, cl = fresh("ckks", 37)
    rng = np.random.default_rng(7)
    g = G.rgsw(cl, G.monomial(N, 3))
    worst = 0.0
    for _ in range(4):
        msg = [int(round(float(v) * 2.0 ** 40)) for v in rng.uniform(-1, 1, size=N)]
        out = G.external_product(ref, cl.k, cl.encrypt_poly_ntt(msg), g)
        want = [-v for v in msg[N - 3:]] + msg[:N - 3]
        worst = max(worst, ckks_rel_error(cl, out, want, msg))
    print("ckks restatement external product: relative error 2^%.1f (%r)" % (np.log2(worst) if worst else -np.inf, worst))
    assert worst <= G.CKKS_REL_MEASURED, worst
    assert G.CKKS_REL_BOUND == G.CKKS_REL_MEASURED * 2.0 ** 10


# ---------------------------------------------------------------- the entries on host-only contexts
def test_entries_on_host_only_context():
    """the header's order: E_POINTER; then the E_INVALIDARG checks that need no handle (the level, l, the mode, alignment,
    overlap), which hold for an empty call too; then the host-only context (COR_E_INVALIDOPERATION), also for an empty call.
    An RGSW handle cannot exist without a device: the pointer handed in here is never followed, and the checks that read a
    handle are in tests/test_gpu_rgsw.py."""
    import sealhip as S

    n = 256
    mods = O.coeff_modulus_create(n, [30, 40, 50, 60])
    parity = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, device=-1)
    strict = S.Context(S.SCHEME_BFV, 8, mods, 2, 65537, mode=S.MODE_STRICT, device=-1)
    ckks = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, device=-1)
    ckks_parity = S.Context(S.SCHEME_CKKS, 8, mods, 2, 0, mode=S.MODE_PARITY, device=-1)
    L = S.lib()
    big = np.zeros(1 << 16, dtype=np.uint64)
    base = big.ctypes.data
    base += (-base) % 16
    a, b, out = base, base + (1 << 15), base + (1 << 17)  # disjoint for count = 1, k = 2, l <= 1
    fake = base + (1 << 18)  # stands for a handle: never followed on a host-only context
    bits = (C.c_void_p * 2)(fake, fake)
    nobits = (C.c_void_p * 2)(fake, None)

    def ext(h, k=2, ct=a, count=1, g=fake, bs=None, o=out):
        return L.sealhip_evaluator_external_product(h, k, ct, count, g, bs, o)

    def cmux(h, k=2, c0=a, c1=b, count=1, g=fake, o=out):
        return L.sealhip_evaluator_cmux(h, k, c0, c1, count, g, o)

    def sel(h, k=2, cts=a, count=1, l=1, gs=bits, o=out):
        return L.sealhip_evaluator_select(h, k, cts, count, l, gs, o)

    ok = (strict.handle, ckks.handle, ckks_parity.handle)
    every = ok + (parity.handle,)
    # 1. null pointers, before anything else (k = 9 would be E_INVALIDARG)
    for h in every:
        for kw in ({"ct": None}, {"g": None}, {"o": None}):
            with pytest.raises(TypeError):
                S._check(ext(h, k=9, **kw))
        for kw in ({"c0": None}, {"c1": None}, {"g": None}, {"o": None}):
            with pytest.raises(TypeError):
                S._check(cmux(h, k=9, **kw))
        for kw in ({"cts": None}, {"o": None}, {"gs": None}, {"l": 2, "gs": nobits}):
            with pytest.raises(TypeError):
                S._check(sel(h, k=9, **kw))
    for fn in (ext, cmux, sel):
        with pytest.raises(TypeError):
            S._check(fn(None))
    # 2. invalid arguments, also for an empty call, in the documented order (each call also breaks every LATER rule)
    for h in every:
        for count in (1, 0):
            for k in (0, 3, 4):
                for fn in (ext, cmux, sel):
                    with pytest.raises(ValueError, match="level k out of range"):
                        S._check(fn(h, k=k, count=count, o=a + 8))
            with pytest.raises(ValueError, match="l out of range"):
                S._check(sel(h, count=count, l=17, o=a + 8))
    for count in (1, 0):
        for fn in (ext, cmux, sel):
            with pytest.raises(ValueError, match="STRICT"):  # (the mode before alignment and overlap)
                S._check(fn(parity.handle, count=count, o=a + 8))
    for h in ok:
        for count in (1, 0):
            for fn, operands in ((ext, ("ct", "bs")), (cmux, ("c0", "c1")), (sel, ("cts",))):
                with pytest.raises(ValueError, match="16-byte aligned"):
                    S._check(fn(h, count=count, o=a + 8))
                for name in operands:
                    with pytest.raises(ValueError, match="16-byte aligned"):
                        S._check(fn(h, count=count, o=a, **{name: b + 8}))
        with pytest.raises(ValueError, match="overlap"):
            S._check(ext(h, o=a))
        with pytest.raises(ValueError, match="overlap"):
            S._check(ext(h, bs=b, o=b + 16 * 10))
        with pytest.raises(ValueError, match="overlap"):
            S._check(cmux(h, o=b + 16))
        with pytest.raises(ValueError, match="overlap"):
            S._check(sel(h, o=a + 8 * 2 * 2 * n))  # (the second leaf)
        assert sel(h, l=0, gs=None, o=a + 8 * 2 * 2 * n) & 0xFFFFFFFF == S.COR_E_INVALIDOPERATION  # (l = 0 reads one)
    # 3. a valid call, with work to do or without, is refused as host-only
    for h in ok:
        for count in (1, 0):
            for fn in (ext, cmux, sel):
                with pytest.raises(S.LogicError, match="host-only"):
                    S._check(fn(h, count=count))
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(ext(h, count=count, bs=b))
            with pytest.raises(S.LogicError, match="host-only"):
                S._check(sel(h, count=count, l=0, gs=None))


def test_object_entries_on_host_only_context():
    """sealhip_generate_rgsw: E_POINTER, then the level, then host-only; create / export / destroy: E_POINTER, then
    host-only. Every out handle is NULL afterwards."""
    import sealhip as S

    mods = O.coeff_modulus_create(256, [30, 40, 50, 60])
    ctx = S.Context(S.SCHEME_CKKS, 8, mods, 1, 0, device=-1)
    L = S.lib()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data

    def gen(h=ctx.handle, sk=p, m=p, n=2, level=3, seeds=p, noise=p, out=True):
        handles = (C.c_void_p * 2)(1, 2)
        return L.sealhip_generate_rgsw(h, sk, m, n, level, seeds, noise, handles if out else None), list(handles)

    for kw in ({"h": None}, {"sk": None}, {"m": None}, {"seeds": None}, {"noise": None}, {"out": False}):
        with pytest.raises(TypeError):
            S._check(gen(level=9, **kw)[0])
    for level in (0, 4):
        hr, handles = gen(level=level)
        with pytest.raises(ValueError, match="level k out of range"):
            S._check(hr)
        assert handles == [None, None]
    for n in (2, 0):
        hr, handles = gen(n=n)
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(hr)
        assert handles == ([None, None] if n else [1, 2])
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(gen(n=0, m=None, seeds=None, noise=None, out=False)[0])  # (an empty list needs no arrays)
    one, two = C.c_void_p(5), (C.c_void_p * 2)(5, 6)
    for args in ((None, p, p, C.byref(one)), (ctx.handle, None, p, C.byref(one)), (ctx.handle, p, None, C.byref(one)),
                 (ctx.handle, p, p, None)):
        with pytest.raises(TypeError):
            S._check(L.sealhip_rgsw_create(*args))
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(L.sealhip_rgsw_create(ctx.handle, p, p, C.byref(one)))
    assert one.value is None
    for args in ((None, p, two), (ctx.handle, None, two), (ctx.handle, p, None)):
        with pytest.raises(TypeError):
            S._check(L.sealhip_rgsw_export(*args))
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(L.sealhip_rgsw_export(ctx.handle, p, two))
    assert list(two) == [None, None]
    for args in ((None, p), (ctx.handle, None)):
        with pytest.raises(TypeError):
            S._check(L.sealhip_rgsw_destroy(*args))
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(L.sealhip_rgsw_destroy(ctx.handle, p))
    out4 = (C.c_int32 * 4)()
    with pytest.raises(TypeError):
        S._check(L.sealhip_debug_ext_mac_plan(ctx.handle, 1, 1, None))
    with pytest.raises(ValueError, match="level k out of range"):
        S._check(L.sealhip_debug_ext_mac_plan(ctx.handle, 4, 1, out4))
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(L.sealhip_debug_ext_mac_plan(ctx.handle, 1, 1, out4))


# ---------------------------------------------------------------- the accumulators and the selector
def test_bounds_check_program(tmp_path):
    exe = compile_cpp(tmp_path, "ext_mac_bounds_check.cpp")
    assert "ext_mac_bounds_check: OK" in run_exe(exe, timeout=120)


def test_bounds_check_program_under_sanitizers(tmp_path):
    exe = compile_cpp(tmp_path, "ext_mac_bounds_check.cpp", sanitize=True)
    assert "ext_mac_bounds_check: OK" in run_exe(exe, timeout=300)


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_rgsw_check.cpp", link_sealhip=True)
    assert "host-only rgsw checks ok" in run_exe(exe, "host", timeout=120)


K_THREADS = 256        # kThreads: lanes of a workgroup
INSTANCES = 16         # the items family is instantiated for ND2 = 2 nd up to 16
FULL_ROUNDS = 4096     # workgroups a larger item group must still leave
KEY_CACHE = 48 << 20   # bytes of key slices above which groups of up to 64 are tried


def blocks_for(lanes):
    return -(-lanes // K_THREADS)


def select_ext_mac(logn, nd, rows, count):
    """the rule of mac_select.hpp's select_ext_mac, restated: from 16 items on, on rings of a workgroup or more and while
    2 nd has an instance, ext_mac_items_kernel<2 nd> with the key switch's item group for a key of 2 nd slices; else the loop
    kernel; (family, nd2, group, n_groups, blocks)"""
    if nd < 1:
        return ("refused", 0, 0, 0, 0)
    if count >= 16 and (1 << logn) >= K_THREADS and 2 * nd <= INSTANCES:
        key_bytes = (2 * (2 * nd) * rows) << (logn + 3)
        group = 64 if key_bytes > KEY_CACHE else 16
        while group > 8 and ((-(-count // group) * rows) << logn) // K_THREADS < FULL_ROUNDS:
            group >>= 1
        n_groups = -(-count // group)
        return ("items", 2 * nd, group, n_groups, blocks_for((n_groups * rows) << logn))
    return ("loop", 0, 0, 0, blocks_for((count * rows) << logn))


def sum_is_split(nd, pmax):
    """ext_mac_plan's other decision (rgsw.hip; bounds::ext_mac_sum_fits): 2 nd products of a digit word (any 64-bit word) by
    a key word (at most pmax - 1), and one more such word, do not fit 128 bits -- the sum is reduced between its halves"""
    return 2 * nd > ((1 << 128) - 1 - (pmax - 1)) // (((1 << 64) - 1) * (pmax - 1))


def test_the_gpu_comparisons_reach_every_instance():
    """the (chain, log N, level, batch) tuples tests/test_gpu_rgsw.py compares word for word -- its COMPARED, which its
    Session.compare enforces -- through the rule above: every even ND2 = 2..16 of the items family, the loop kernel for each
    of its three reasons, and the split sum in both families"""
    import test_gpu_rgsw as R  # (it imports this module: resolved at the call)

    items, loop_reasons, split = set(), set(), set()
    for chain, logn, k, count in R.COMPARED:
        _, bits, nsp, _, _ = R.CHAINS[chain]
        assert 1 <= k <= len(bits) - nsp, (chain, k)
        nd = -(-k // nsp)
        mods = [int(p) for p in O.coeff_modulus_create(1 << logn, bits)]
        family, nd2 = select_ext_mac(logn, nd, k + nsp, count)[:2]
        if family == "items":
            assert nd2 == 2 * nd
            items.add(nd2)
        else:
            assert family == "loop"
            # (the first reason that applies, in the selector's order)
            loop_reasons.add("small batch" if count < 16 else ("ring below a workgroup" if 1 << logn < K_THREADS else "no instance"))
            assert count < 16 or 1 << logn < K_THREADS or 2 * nd > INSTANCES
        if sum_is_split(nd, max(mods[:k] + mods[len(bits) - nsp:])):
            split.add(family)
    assert items == set(range(2, INSTANCES + 1, 2)), sorted(items)
    assert loop_reasons == {"small batch", "ring below a workgroup", "no instance"}
    assert split == {"items", "loop"}
    # each reason alone: a full batch on a small ring, a full batch on a full ring at nine digits
    assert any(count >= 16 and logn < 8 for _, logn, _, count in R.COMPARED)
    assert ("nd9", 8, 9, 17) in R.COMPARED and select_ext_mac(8, 9, 10, 17)[0] == "loop"
    assert {t[2:] for t in R.SEVEN_DIGITS} == {(7, 17), (6, 17), (7, 1)} <= {t[2:] for t in R.COMPARED if t[0] == "nd7"}
    assert not sum_is_split(8, (1 << 60) - 1) and sum_is_split(5, (1 << 61) - 1) and not sum_is_split(4, (1 << 61) - 1)


def test_the_selector_and_the_rule_here_agree_call_by_call(tmp_path):
    exe = compile_cpp(tmp_path, "ext_select_check.cpp", extra=("-I", CSRC))
    assert "ext_select_check: OK" in run_exe(exe, timeout=120)
    lines = [(logn, nd, nd * nsp + nsp, count) for logn in range(3, 17) for nd in range(0, 18) for nsp in (1, 3)
             for count in (1, 15, 16, 17, 33, 64, 256, 1000, 4096, 5000)]
    path = tmp_path / "calls.txt"
    path.write_text("".join(" ".join(str(v) for v in line) + "\n" for line in lines))
    got = run_exe(exe, "--calls", path, timeout=120).splitlines()
    assert len(got) == len(lines)
    seen = set()
    for line, out in zip(lines, got):
        want = select_ext_mac(*line)
        assert out == " ".join(str(v) for v in want), (line, out, want)
        seen.add((want[0], want[2]))
    assert seen == {("refused", 0), ("loop", 0), ("items", 8), ("items", 16), ("items", 32), ("items", 64)}
