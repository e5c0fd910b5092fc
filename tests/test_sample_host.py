"""RLWE samples from seeds (sealhip_sample_polys and its host form, sealhip_debug_sample_map, sealhip_generate_secret_key;
DESIGN.md section 22): what can be checked without a GPU. The exports and mirror methods exist and check their arguments in
the order of the neighbouring entries; the numpy restatement of the rule (tests/sample_ref.py) equals the library's host
sampler word for word; the committed thresholds are the formula's; and the samples follow the law the reference draws from
(tests/sample_law_check.cpp draws it the reference's way)."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import sample_ref as R
from support import compile_cpp, run_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(1, 0), (0, 1), (1, 2), (0, 3), (2, 2)]


def host_ctx(logn):
    import sealhip as S

    n = 1 << logn
    return S.Context(S.SCHEME_CKKS, logn, O.coeff_modulus_create(n, [30, 30]), 1, 0, device=-1)


def test_exports_and_argument_checks_on_a_host_only_context():
    import sealhip as S

    L = S.lib()
    for name in ("sealhip_sample_polys", "sealhip_sample_polys_host", "sealhip_sample_polys_split", "sealhip_debug_sample_map",
                 "sealhip_generate_secret_key", "sealhip_memset_zero"):
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("sample_polys", "sample_polys_host", "sample_polys_split", "debug_sample_map", "generate_secret_key", "memset_zero"):
        assert callable(getattr(S.Context, name))
    ctx = host_ctx(6)
    n = ctx.n
    seeds = np.zeros((2, 8), dtype=np.uint64)
    out = np.zeros(2 * 16 * n + 4, dtype=np.int32)
    base = out.ctypes.data + (-out.ctypes.data % 16)  # 16-byte aligned
    words = np.zeros(4, dtype=np.uint64)
    # null pointers first, before the context is looked at
    for fn in (L.sealhip_sample_polys, L.sealhip_sample_polys_host):
        with pytest.raises(TypeError):
            S._check(fn(None, seeds.ctypes.data, 1, 1, 2, base, 0))
        with pytest.raises(TypeError):
            S._check(fn(ctx.handle, None, 1, 99, 99, base, 0))  # (ahead of the bad counts)
        with pytest.raises(TypeError):
            S._check(fn(ctx.handle, seeds.ctypes.data, 1, 99, 99, None, 0))
    with pytest.raises(TypeError):
        S._check(L.sealhip_debug_sample_map(ctx.handle, None, 4, 7, base))
    with pytest.raises(TypeError):
        S._check(L.sealhip_debug_sample_map(ctx.handle, words.ctypes.data, 4, 7, None))
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_secret_key(ctx.handle, None, base))
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_secret_key(ctx.handle, seeds.ctypes.data, None))
    with pytest.raises(TypeError):
        S._check(L.sealhip_memset_zero(ctx.handle, None, 8))
    # then bad arguments, also on a host-only context (so ahead of "host-only")
    for fn in (L.sealhip_sample_polys, L.sealhip_sample_polys_host):
        for nt, nn, stride in ((0, 0, 0), (9, 8, 0), (16, 1, 0), (1, 2, 3 * n - 4), (1, 0, 4)):
            with pytest.raises(ValueError):
                S._check(fn(ctx.handle, seeds.ctypes.data, 1, nt, nn, base, stride))
    with pytest.raises(ValueError, match="aligned"):
        S._check(L.sealhip_sample_polys(ctx.handle, seeds.ctypes.data, 1, 1, 2, base + 4, 0))
    with pytest.raises(ValueError, match="multiple of 4"):
        S._check(L.sealhip_sample_polys(ctx.handle, seeds.ctypes.data, 1, 1, 2, base, 3 * n + 2))
    with pytest.raises(TypeError):
        S._check(L.sealhip_sample_polys_split(ctx.handle, seeds.ctypes.data, 1, 1, 2, base, None))
    with pytest.raises(ValueError):
        S._check(L.sealhip_sample_polys_split(ctx.handle, seeds.ctypes.data, 1, 0, 0, None, None))
    with pytest.raises(ValueError, match="aligned"):
        S._check(L.sealhip_sample_polys_split(ctx.handle, seeds.ctypes.data, 1, 1, 2, base, base + 4))
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.sample_polys_split(seeds, 0, 1, None, base)
    with pytest.raises(ValueError, match="kind"):
        S._check(L.sealhip_debug_sample_map(ctx.handle, words.ctypes.data, 4, 2, base))
    # then the host-only context: the device entries have no CPU fallback, count 0 included
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.sample_polys(seeds, 1, 2, base)
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.sample_polys(seeds[:0], 1, 2, base)
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(L.sealhip_debug_sample_map(ctx.handle, words.ctypes.data, 4, 1, base))
    with pytest.raises(S.LogicError, match="host-only"):
        S._check(L.sealhip_generate_secret_key(ctx.handle, seeds.ctypes.data, base))
    with pytest.raises(S.LogicError, match="host-only"):
        ctx.memset_zero(base, 8)
    # the host form works there: layout out[i][p][N], a padded stride leaves the words between items alone
    got = ctx.sample_polys_host(seeds, 1, 2)
    assert got.shape == (2, 3 * n) and set(np.unique(got[:, :n])) <= {-1, 0, 1}
    assert ctx.sample_polys_host(seeds[:0], 1, 2).shape == (0, 3 * n)
    out[:] = 77
    S._check(L.sealhip_sample_polys_host(ctx.handle, seeds.ctypes.data, 2, 1, 2, base, 3 * n + 5))
    view = out[(base - out.ctypes.data) // 4 :][: 2 * (3 * n + 5)].reshape(2, 3 * n + 5)
    assert np.array_equal(view[:, : 3 * n], got) and np.all(view[:, 3 * n :] == 77)


@pytest.mark.parametrize("logn", [3, 6, 9, 10, 12])
def test_restated_rule_equals_the_host_sampler(logn):
    """buffer / leaf / word of the stream, polynomial p from words [pN, (p+1)N), the two maps: word for word"""
    import sealhip as S

    ctx = host_ctx(logn)
    rng = np.random.default_rng(100 + logn)
    seeds = np.stack([np.zeros(8, dtype=np.uint64), np.full(8, 2**64 - 1, dtype=np.uint64),
                      rng.integers(0, 2**64, size=8, dtype=np.uint64), rng.integers(0, 2**64, size=8, dtype=np.uint64)])
    for nt, nn in KINDS:
        want = R.sample_polys(S, seeds, ctx.n, nt, nn)
        got = ctx.sample_polys_host(seeds, nt, nn).reshape(want.shape)
        assert np.array_equal(got, want), (logn, nt, nn)
        assert np.abs(got[:, :nt]).max(initial=0) <= 1 and np.abs(got).max() <= 19


def header_thresholds():
    with open(os.path.join(ROOT, "gemini-seal_amd", "csrc", "sample_map.hpp")) as f:
        text = f.read()
    body = re.search(r"kNoiseCdt\[kNoiseCdtSize\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    return [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", body)]


def test_threshold_table_is_the_formula():
    """header = fixture; T_m = 2^63 - round(2^63 tail_m) for a tail_m within a relative 2^-40 of math.erfc's (good to about
    2^-50): |(2^63 - T_m) - 2^63 tail_m| <= 2^-40 x 2^63 tail_m + 1/2, the half being the formula's own round() -- an integer
    threshold cannot sit closer than that to a real number (at m = 17 the mass 2^63 tail_m is 2^37.2, so 2^-40 of it is 0.14
    of a unit, and the committed T_17 is 0.46 from it as every rounded value may be). The 19 roundings move at most
    19 x 2^-64 of probability, so the statistical distance from the reference's law stays below 2^-40. Strictly increasing."""
    T = R.thresholds()
    assert len(T) == 19 and header_thresholds() == T
    assert T[0] == 0x1F67485E1414E400 and T[18] == 0x7FFFFFFE05C3F8AD
    for m, t in enumerate(T):
        mass = 2.0**63 * R.tail(m)
        assert abs(((1 << 63) - t) - mass) <= 2.0**-40 * mass + 0.5, m
    assert all(a < b for a, b in zip(T, T[1:])) and 0 < T[0] and T[18] < 1 << 63
    P = R.magnitude_probabilities(T)
    assert abs(P[0] - 0.2453) < 5e-5
    sd = sum(m * m * p for m, p in enumerate(P)) ** 0.5
    assert abs(sd - 2.83) < 5e-3  # truncation toward zero: not 3.2


def test_samples_follow_the_law():
    """2^20 noise and 2^20 ternary samples of the host sampler with fixed seeds: chi-square against the table's
    probabilities (28 cells) and against thirds (3 cells), bound = the 1 - 10^-6 quantile"""
    ctx = host_ctx(12)
    seeds = np.arange(16 * 8, dtype=np.uint64).reshape(16, 8) + np.uint64(0x5EED0000)
    noise = ctx.sample_polys_host(seeds, 0, 16).reshape(-1)
    tern = ctx.sample_polys_host(seeds + np.uint64(1 << 32), 16, 0).reshape(-1)
    assert noise.size == tern.size == 1 << 20
    assert np.abs(noise).max() <= 19
    values, counts = np.unique(noise, return_counts=True)
    stat, cells = R.noise_chi2(dict(zip(values.tolist(), counts.tolist())), noise.size)
    print("noise chi-square", stat, "cells", cells, "bound", R.chi2_bound(cells))
    assert cells == 28 and stat <= R.chi2_bound(cells)
    assert set(np.unique(tern)) == {-1, 0, 1}
    exp = tern.size / 3
    tstat = sum((int(np.sum(tern == v)) - exp) ** 2 / exp for v in (-1, 0, 1))
    print("ternary chi-square", tstat, "bound", R.chi2_bound(3))
    assert tstat <= R.chi2_bound(3)


def test_table_is_the_reference_law(tmp_path):
    """normal_distribution(0, 3.2), redraw beyond 19.2, truncate (tests/sample_law_check.cpp): its histogram of 2^20 samples
    against the table, same cells and bound"""
    exe = compile_cpp(tmp_path, "sample_law_check.cpp")
    stdout = run_exe(exe, timeout=120)
    hist = {}
    for line in stdout.splitlines():
        a, b = line.split()
        if a != "samples_per_second":
            hist[int(a)] = int(b)
    assert sorted(hist) == list(range(-19, 20)) and sum(hist.values()) == 1 << 20
    stat, cells = R.noise_chi2(hist, 1 << 20)
    print("reference-style chi-square", stat, "cells", cells, "bound", R.chi2_bound(cells))
    assert cells == 28 and stat <= R.chi2_bound(cells)


def test_cpp_seed_source_checks_on_host_only_context(tmp_path):
    """tests/host_adapter_sample_check.cpp without a device: an empty seed source is refused, a pair of seeds is drawn public
    seed first and a repeated seed is refused, generate_secret_key draws one seed and has no host fallback. (With a device
    the same program counts the draws of every operation and searches the seeded save for noise seeds:
    tests/test_gpu_sample.py.)"""
    exe = compile_cpp(tmp_path, "host_adapter_sample_check.cpp", link_sealhip=True, opt="-O1")
    assert "host-only sample checks ok" in run_exe(exe, timeout=120)
