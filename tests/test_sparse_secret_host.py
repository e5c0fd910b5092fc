"""Fixed-weight secrets and sparse-secret encapsulation: what can be checked without a GPU. The new
exports exist everywhere they are documented; the numpy restatement of the rule (tests/fixed_weight_ref.py) equals the
library's host sampler word for word and the weight is exactly h; the polynomials follow the law the rule claims (uniform
support, fair independent signs); and, on the oracle alone, the raise under a weight-32 secret keeps ModRaise's integer
polynomial inside K = 12 where the raise under the library's dense secret does not."""
import os

import numpy as np
import pytest

import bootstrap_ref as B
import fixed_weight_ref as F
import oracle_lib as O
import sample_ref as R
from support import compile_cpp, run_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_ctx(logn):
    import sealhip as S

    n = 1 << logn
    return S.Context(S.SCHEME_CKKS, logn, O.get_primes(n, 30, 2), 1, 0, device=-1)


def section_25():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    start = text.index("\n## 25.")
    end = text.find("\n## 26.", start)
    return text[start : end if end > 0 else None]


def test_new_exports():
    import sealhip as S

    with open(os.path.join(ROOT, "include", "sealhip.h")) as f:
        header = f.read()
    design = section_25()
    L = S.lib()
    for name in ("sealhip_sample_fixed_weight", "sealhip_sample_fixed_weight_host", "sealhip_debug_fixed_weight_map",
                 "sealhip_generate_sparse_secret_key", "sealhip_generate_switching_keys", "sealhip_evaluator_switch_secret",
                 "sealhip_evaluator_bootstrap_encapsulated"):
        assert hasattr(L, name) and name in S.SYMBOLS and name in header and name in design, name
    for name in ("sample_fixed_weight", "sample_fixed_weight_host", "debug_fixed_weight_map", "generate_sparse_secret_key",
                 "generate_switching_keys"):
        assert callable(getattr(S.Context, name)), name
    for name in ("switch_secret", "bootstrap_encapsulated"):
        assert callable(getattr(S.Evaluator, name)), name
    for word in ("N^2 / 2^64", "rank_i", "(h + 1) / 2 + 1", "level = 1"):
        assert word in design, word
    assert "does not sample sparse secrets" in header and "sealhip_generate_sparse_secret_key makes" in header
    adapter = ""
    for name in ("evaluator.hpp", "crypto.hpp"):  # Evaluator; KeyGenerator
        with open(os.path.join(ROOT, "gemini-seal_amd", "host", name)) as f:
            adapter += f.read()
    for word in ("generate_sparse_secret_key(const Context &context, const SeedSource &seeds, std::uint32_t h)",
                 "Keys switching_keys(", "void switch_secret(const C &encrypted, const KSwitchKeys &key, C &destination)",
                 "const KSwitchKeys &to_sparse, const KSwitchKeys &to_dense"):
        assert word in adapter, word


def test_argument_checks_on_a_host_only_context():
    """the order of sealhip_sample_polys' checks: null pointers, then bad arguments (also here), then "host-only" """
    import sealhip as S

    L = S.lib()
    ctx = host_ctx(6)
    n = ctx.n
    seeds = np.zeros((2, 8), dtype=np.uint64)
    out = np.zeros(2 * 2 * n + 4, dtype=np.int32)
    base = out.ctypes.data + (-out.ctypes.data % 16)
    for fn in (L.sealhip_sample_fixed_weight, L.sealhip_sample_fixed_weight_host):
        with pytest.raises(TypeError):
            S._check(fn(None, seeds.ctypes.data, 1, 8, base, 0))
        with pytest.raises(TypeError):
            S._check(fn(ctx.handle, None, 1, 0, base, 0))  # (ahead of the bad weight)
        with pytest.raises(TypeError):
            S._check(fn(ctx.handle, seeds.ctypes.data, 1, 0, None, 0))
        for h, stride in ((0, 0), (n + 1, 0), (8, n - 4)):
            with pytest.raises(ValueError):
                S._check(fn(ctx.handle, seeds.ctypes.data, 1, h, base, stride))
    with pytest.raises(ValueError, match="aligned"):
        S._check(L.sealhip_sample_fixed_weight(ctx.handle, seeds.ctypes.data, 1, 8, base + 4, 0))
    with pytest.raises(ValueError, match="multiple of 4"):
        S._check(L.sealhip_sample_fixed_weight(ctx.handle, seeds.ctypes.data, 1, 8, base, n + 2))
    with pytest.raises(TypeError):
        S._check(L.sealhip_debug_fixed_weight_map(ctx.handle, None, 1, 8, base))
    with pytest.raises(ValueError, match="1 .. N"):
        S._check(L.sealhip_debug_fixed_weight_map(ctx.handle, base, 1, 0, base))
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_sparse_secret_key(ctx.handle, None, 8, base))
    with pytest.raises(ValueError, match="1 .. N"):
        S._check(L.sealhip_generate_sparse_secret_key(ctx.handle, seeds.ctypes.data, n + 1, base))
    for call in (lambda: ctx.sample_fixed_weight(seeds, 8, base), lambda: ctx.sample_fixed_weight(seeds[:0], 8, base),
                 lambda: S._check(L.sealhip_debug_fixed_weight_map(ctx.handle, base, 1, 8, base)),
                 lambda: ctx.generate_sparse_secret_key(seeds[0], 8, base)):
        with pytest.raises(S.LogicError, match="host-only"):
            call()
    # the switching keys' checks, as the relin keys': null pointers, the level, the count; then "host-only", empty included
    keys = (S.C.c_void_p * 2)(1, 2)
    nd = 1
    noise = np.zeros((2, nd, n), dtype=np.int32)
    sp, npn = seeds.ctypes.data, noise.ctypes.data
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_switching_keys(ctx.handle, None, base, 1, 1, sp, npn, 0, keys))
    with pytest.raises(TypeError):
        S._check(L.sealhip_generate_switching_keys(ctx.handle, base, None, 1, 1, sp, npn, 0, keys))
    for level in (0, 2):  # n_ct = 1 here
        keys = (S.C.c_void_p * 2)(1, 2)
        with pytest.raises(ValueError, match="level"):
            S._check(L.sealhip_generate_switching_keys(ctx.handle, base, base, 2, level, sp, npn, 0, keys))
        assert list(keys) == [None, None]
    with pytest.raises(ValueError, match="invalid count"):
        S._check(L.sealhip_generate_switching_keys(ctx.handle, base, base, 15, 1, sp, npn, 0, (S.C.c_void_p * 15)()))
    for count in (0, 1):
        with pytest.raises(S.LogicError, match="host-only"):
            S._check(L.sealhip_generate_switching_keys(ctx.handle, base, base, count, 1, sp, npn, 0, keys))
    # the host form works here: a padded stride leaves the words between the items alone
    got = ctx.sample_fixed_weight_host(seeds, 8)
    assert got.shape == (2, n) and ctx.sample_fixed_weight_host(seeds[:0], 8).shape == (0, n)
    out[:] = 77
    S._check(L.sealhip_sample_fixed_weight_host(ctx.handle, seeds.ctypes.data, 2, 8, base, n + 5))
    view = out[(base - out.ctypes.data) // 4 :][: 2 * (n + 5)].reshape(2, n + 5)
    assert np.array_equal(view[:, :n], got) and np.all(view[:, n:] == 77)


@pytest.mark.parametrize("logn", [3, 8, 12, 16])
def test_restated_rule_equals_the_host_sampler(logn):
    import sealhip as S

    ctx = host_ctx(logn)
    n = ctx.n
    rng = np.random.default_rng(250 + logn)
    seeds = np.stack([np.zeros(8, dtype=np.uint64), np.full(8, 2**64 - 1, dtype=np.uint64),
                      rng.integers(0, 2**64, size=8, dtype=np.uint64)])
    words = np.stack([R.stream_words(S, s, n) for s in seeds])
    assert np.array_equal(words[0, : min(n, 64)], R.stream_words(S, seeds[0], 2 * n)[: min(n, 64)])
    for h in (1, 2, n // 2, n - 1, n):
        want = F.fixed_weight_map(words, h)
        got = ctx.sample_fixed_weight_host(seeds, h)
        assert np.array_equal(got, want), (logn, h)
        assert np.all(np.count_nonzero(got, axis=1) == h) and set(np.unique(got)) <= {-1, 0, 1}, (logn, h)
    # the ternary polynomial 0 of the same seed consumes the same words
    assert np.array_equal(R.ternary_map(words), ctx.sample_polys_host(seeds, 1, 0))


def test_restatement_on_ties():
    """the stable sort is the rule's tie-break: equal words rank by index"""
    w = np.array([[5, 3, 5, 3, 9, 3, 0, 5]], dtype=np.uint64)
    assert F.fixed_weight_map(w, 4).tolist() == [[0, -1, 0, -1, 0, -1, 1, 0]]
    assert F.fixed_weight_map(w, 5).tolist() == [[-1, -1, 0, -1, 0, -1, 1, 0]]
    assert F.fixed_weight_map(np.full((1, 8), 7, dtype=np.uint64), 3).tolist() == [[-1, -1, -1, 0, 0, 0, 0, 0]]


def test_polynomials_follow_the_law():
    """N = 64, h = 8, 2^14 fixed seeds through the host entry. Chi-square of the support counts over the 64 positions (expected
    2048 each) and of the 2 x 64 signed cells (1024 each), bound = the 1 - 10^-6 quantile for cells - 1 degrees of freedom
    (a fixed weight only lowers the statistic: the counts' covariance is (N - h) / (N - 1) of the multinomial's). Adjacent
    pairs: the number of polynomials with i and i + 1 both in the support, against the hypergeometric
    2^14 h (h - 1) / (N (N - 1)) = 227.6 for each of the 63 pairs; the pairs' counts have no fixed sum, so 63 degrees of
    freedom, the same quantile."""
    n, h, count = 64, 8, 1 << 14
    ctx = host_ctx(6)
    seeds = np.arange(count * 8, dtype=np.uint64).reshape(count, 8) + np.uint64(0xF1DED0000)
    got = ctx.sample_fixed_weight_host(seeds, h)
    assert np.all(np.count_nonzero(got, axis=1) == h)
    inside = got != 0
    exp = count * h / n
    stat = float(np.sum((inside.sum(axis=0) - exp) ** 2 / exp))
    print("support chi-square", stat, "bound", R.chi2_bound(n))
    assert stat <= R.chi2_bound(n)
    signed = np.concatenate([(got == 1).sum(axis=0), (got == -1).sum(axis=0)])
    sstat = float(np.sum((signed - exp / 2) ** 2 / (exp / 2)))
    print("signed chi-square", sstat, "bound", R.chi2_bound(2 * n))
    assert sstat <= R.chi2_bound(2 * n)
    pairs = (inside[:, :-1] & inside[:, 1:]).sum(axis=0)
    pexp = count * h * (h - 1) / (n * (n - 1))
    pstat = float(np.sum((pairs - pexp) ** 2 / pexp))
    print("adjacent pairs chi-square", pstat, "bound", R.chi2_bound(n))
    assert pairs.size == n - 1 and pstat <= R.chi2_bound(n)  # (chi2_bound(cells) has cells - 1 = 63 degrees of freedom)


def primes_next_to(value, logn, count):
    """`count` NTT primes next to `value`, alternately above and below (the list of tests/test_gpu_bootstrap.py)"""
    below, above = O.ntt_primes_around(value, logn)
    while len(below) + len(above) < count + 2:
        below += O.ntt_primes_around(below[-1] - 1, logn)[0]
        above += O.ntt_primes_around(above[-1], logn)[1]
    out = []
    for lo, hi in zip(below, above):
        out += [hi, lo]
    assert len(set(out)) == len(out)
    return out[:count]


def bootstrap_mods(logn=12):
    n = 1 << logn
    q0 = O.get_primes(n, 50, 1)[0]
    return [q0] + primes_next_to(12 * q0, logn, 15) + O.get_primes(n, 59, 2)


def raise_overflows(cl, raised, m, q0):
    """I of a raised ciphertext (2, k, N) that decrypts under cl to m + q_0 I + noise: (max|I|, max|noise|)"""
    c, _ = F.decrypt_centred(cl, raised)
    I = [(c[j] - int(m[j]) + q0 // 2) // q0 for j in range(len(m))]
    return max(abs(v) for v in I), max(abs(c[j] - int(m[j]) - q0 * I[j]) for j in range(len(m)))


def test_why_the_feature_matters():
    """Oracle only, N = 2^12, the primes of test_bootstrap_end_to_end. The dense secret is the library's
    sample_polys_host(seed, 1, 0), the weight-32 one sealhip_sample_fixed_weight_host's. m is encrypted under the dense one.
    The encapsulated raise -- ref_switch_key_inplace at level 1 with an oracle-made dense -> sparse key, bootstrap_ref.mod_raise,
    ref_switch_key_inplace at level 16 with the sparse -> dense key -- decrypts under the DENSE secret to m + q_0 I with
    max|I| <= 11 (K = 12 covers it: h = 32 gives a standard deviation of about 1.7), where the plain raise of the same
    ciphertext has max|I| > 11 (h about 2730: a standard deviation of about 15).
    Measured: encapsulated max|I| = 6, plain max|I| = 57."""
    logn, n, k_top = 12, 1 << 12, 16
    mods = bootstrap_mods(logn)
    q0 = mods[0]
    host = host_ctx(logn)
    seed = np.arange(8, dtype=np.uint64) + np.uint64(0x5A2E5EED)
    dense = host.sample_polys_host(seed, 1, 0)[0]
    sparse = host.sample_fixed_weight_host(seed + np.uint64(8), 32)[0]
    assert np.count_nonzero(sparse) == 32 and abs(np.count_nonzero(dense) - 2 * n / 3) < 150
    ref = O.RefContext(2, logn, mods, nsp=2, t=0, mode=0)
    cd, cs = F.SecretClient(ref, dense, seed=21), F.SecretClient(ref, sparse, seed=22)
    to_sparse, to_dense = cs.kswitch_key(cd.sk), cd.kswitch_key(cs.sk)
    rng = np.random.default_rng(78)
    m = rng.integers(-(1 << 39), 1 << 39, size=n).astype(np.int64)
    low = np.ascontiguousarray(cd.encrypt_poly_ntt([int(v) for v in m])[:, :1])  # (2, 1, N): the q_0 rows
    plain_I, plain_noise = raise_overflows(cd, B.mod_raise(ref, low[None], k_top)[0], m, q0)
    low_sparse = F.switch_secret(ref, low, to_sparse)
    sparse_I, _ = raise_overflows(cs, low_sparse, m, q0)
    assert sparse_I == 0, "the level-1 switch carries m"
    raised = F.switch_secret(ref, B.mod_raise(ref, low_sparse[None], k_top)[0], to_dense)
    enc_I, enc_noise = raise_overflows(cd, raised, m, q0)
    print("max|I|: encapsulated %d (noise %d), plain %d (noise %d)" % (enc_I, enc_noise, plain_I, plain_noise))
    assert enc_noise < 1 << 20, "what is left next to m + q_0 I is the two key switches' noise"
    assert enc_I <= 11
    assert plain_I > 11


def test_cpp_adapter_checks_on_host_only_context(tmp_path):
    """tests/host_adapter_sparse_secret_check.cpp without a device: a weight outside 1..N and the switching keys' count, null
    source and level are refused before any seed is drawn; valid calls draw their seeds (one for a secret key, two per digit
    of a switching key) and are then refused by the host-only context"""
    exe = compile_cpp(tmp_path, "host_adapter_sparse_secret_check.cpp", link_sealhip=True, opt="-O1")
    assert "host-only sparse secret checks ok" in run_exe(exe, "host", timeout=120)
