"""transform_to_ntt(Plaintext) and mod_switch_to(Plaintext) on the device: sealhip_evaluator_transform_plain_to_ntt and
sealhip_evaluator_mod_switch_plain_to. Every word against the oracle (the lift restated as in tests/test_plain_ntt_host.py,
then ref_ntt_forward per row), against the coefficient-form multiply_plain, and end to end through encryption and
decryption on parameters without fast plain lift, where no other plaintext product exists."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from test_plain_ntt_host import build_plain_adapter
from support import S, run_exe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = json.load(open(os.path.join(HERE, "golden", "ntt_instance_classes.json")))
T40 = (1 << 40) - 87  # odd, coprime to every NTT prime used here
T_VALUES = (2, 1 << 16, 786433, T40)


def lift(plain, t, q):
    """(v - t [v >= thr]) mod q on uint64 words v < t (tests/test_plain_ntt_host.py: both reference branches)"""
    v = np.asarray(plain, dtype=np.uint64)
    r = v % np.uint64(q)
    tq = np.uint64(t % q)
    neg = v >= np.uint64((t + 1) >> 1)
    r[neg] = (r[neg] + (np.uint64(q) - tq)) % np.uint64(q)
    return r


_TABLES = {}


def tables(logn, q):
    if (logn, q) not in _TABLES:
        if len(_TABLES) > 16:
            _TABLES.clear()
        _TABLES[(logn, q)] = O.Tables(logn, q)
    return _TABLES[(logn, q)]


def expected(plains, coeff_count, t, mods, logn, strict):
    """[count][k][N]: each plaintext zero-padded to N, lifted per prime, ref_ntt_forward per row"""
    n = 1 << logn
    out = np.zeros((len(plains), len(mods), n), dtype=np.uint64)
    L = O.lib()
    for c, p in enumerate(plains):
        full = np.zeros(n, dtype=np.uint64)
        full[:coeff_count] = p[:coeff_count]
        for i, q in enumerate(mods):
            out[c, i] = lift(full, t, q)
            L.ref_ntt_forward(O.ptr(out[c, i]), C.byref(tables(logn, q).t), 1 if strict else 0)
    return out


def rand_plain(rng, t, n):
    """random words below t with both halves planted: 0, thr - 1, thr, t - 1 at the ends and the middle"""
    p = rng.integers(0, t, n, dtype=np.uint64)
    thr = (t + 1) >> 1
    for i, v in zip((0, 1, n // 2 - 1, n // 2, n - 2, n - 1), (0, thr - 1, thr, t - 1, thr, t - 1)):
        if i < n:
            p[i] = v
    return p


def primes_for(logn, cls):
    """three NTT primes per class (at 2^14..2^16 the largest ones the class admits, below the auxiliary primes for the
    60-bit class); with T40 the 30-bit prime added to every set makes the lift non-fast (q_0 < t)"""
    if logn < 14:
        top = O.ntt_primes_around((1 << 36) - 1, logn)[0]
        return top[:2] + [O.ntt_primes_around((1 << 30) - 1, logn)[0][0]]
    top = CLASSES[str(logn)][cls]
    if cls == "fwd_dense":
        top -= 1 << 50  # (60-bit primes clear of the BFV context's auxiliary primes, the largest 60-bit ones)
    below = O.ntt_primes_around(top, logn)[0]
    assert cls != "fwd_dense" or min(below) > CLASSES[str(logn)]["fwd_canon"]
    return below[:2] + [O.ntt_primes_around((1 << 30) - 1, logn)[0][0]]


def run_transform(S, ctx, plains_host, coeff_count, k, count, stride):
    ev = S.Evaluator(ctx)
    n = ctx.n
    words = max(1, (count - 1) * (stride or coeff_count) + coeff_count) if count else 1
    flat = np.zeros(max(words, 1), dtype=np.uint64)
    for c in range(count):
        base = c * (stride or coeff_count)
        flat[base:base + coeff_count] = plains_host[c][:coeff_count]
    d_plain = ctx.upload(flat)
    d_out = ctx.alloc(max(1, count * k * n))
    ev.transform_plain_to_ntt(d_plain, coeff_count, k, count, d_out, plain_stride=stride)
    return d_out.download()[:count * k * n].reshape(count, k, n)


RINGS = [(logn, "any") for logn in range(3, 14)] + [(logn, c) for logn in (14, 15, 16) for c in ("fp64", "fwd_canon", "fwd_dense")]


@pytest.mark.parametrize("strict", [False, True], ids=["parity", "strict"])
@pytest.mark.parametrize("logn,cls", RINGS, ids=["%d-%s" % r for r in RINGS])
def test_transform_plain_to_ntt_matches_oracle(S, logn, cls, strict):
    n = 1 << logn
    mods = primes_for(logn, cls)
    rng = np.random.default_rng(logn * 7 + len(cls) + strict)
    mode = S.MODE_STRICT if strict else S.MODE_PARITY
    for t in T_VALUES:
        ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=mode, device=0)
        assert (t > min(mods)) == (t == T40)  # T40: no fast plain lift; the others: fast
        plains = [rand_plain(rng, t, n) for _ in range(3)]
        # every level, the full plaintext
        for k in range(1, len(mods) + 1):
            got = run_transform(S, ctx, plains, n, k, 1, 0)
            assert np.array_equal(got, expected(plains[:1], n, t, mods[:k], logn, strict)), (logn, cls, t, k)
        # coefficient counts 0, 1, N/2 (and N above); back to back and with a larger (odd, then even) stride
        k = len(mods)
        for cc, count, stride in ((0, 1, 0), (1, 3, 0), (max(n // 2, 1), 3, 0), (max(n // 2, 1), 3, n + 1), (n, 3, n + 2)):
            got = run_transform(S, ctx, plains, cc, k, count, stride)
            assert np.array_equal(got, expected(plains[:count], cc, t, mods, logn, strict)), (logn, cls, t, cc, stride)
        ctx.close()


@pytest.mark.parametrize("logn", [10, 14])
def test_transform_plain_to_ntt_large_batch(S, logn):
    """count 257 plaintexts back to back"""
    n = 1 << logn
    mods = primes_for(logn, "fwd_canon")
    rng = np.random.default_rng(257 + logn)
    t = 786433
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, device=0)
    plains = [rand_plain(rng, t, n) for _ in range(257)]
    got = run_transform(S, ctx, plains, n, 2, 257, 0)
    assert np.array_equal(got, expected(plains, n, t, mods[:2], logn, False))


def _multiply_paths(S, ctx, k, ct, plain, strict_note):
    ev = S.Evaluator(ctx)
    n, count, size = ctx.n, ct.shape[0], ct.shape[1]
    a = ctx.upload(ct)
    ev.multiply_plain_inplace(a, size, k, count, ctx.upload(plain), plain_stride=n, ntt_form=False)
    want = a.download(ct.shape)
    b = ctx.upload(ct)
    ev.transform_to_ntt_inplace(b, size, k, count)
    pn = ctx.alloc(count * k * n)
    ev.transform_plain_to_ntt(ctx.upload(plain), n, k, count, pn)
    ev.multiply_plain_inplace(b, size, k, count, pn, plain_stride=k * n, ntt_form=True)
    ev.transform_from_ntt_inplace(b, size, k, count)
    assert np.array_equal(b.download(ct.shape), want), strict_note


EQUIV = [(logn, c, s) for logn in (14, 15, 16) for c in ("fp64", "fwd_canon", "fwd_dense") for s in (True, False)
         if s or c != "fwd_dense"] + [(12, "any", True), (12, "any", False)]


@pytest.mark.parametrize("logn,cls,strict", EQUIV, ids=["%d-%s-%s" % (l, c, "strict" if s else "parity") for l, c, s in EQUIV])
def test_ntt_form_product_equals_multiply_plain(S, logn, cls, strict):
    """fast lift: transform_to_ntt(ct) -> transform_plain_to_ntt -> multiply_plain_ntt -> transform_from_ntt is the
    coefficient-form multiply_plain, bit for bit"""
    n = 1 << logn
    mods = primes_for(logn, cls)[:2] + [O.ntt_primes_around((1 << 40) - 1, logn)[0][0]]  # (every q_i > t)
    t = 786433
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT if strict else S.MODE_PARITY, device=0)
    rng = np.random.default_rng(logn + 100 * strict)
    k, count = 2, 2
    ct = np.stack([np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in mods[:k]]) for _ in range(2)])
                   for _ in range(count)])
    plain = np.stack([rand_plain(rng, t, n) for _ in range(count)])
    _multiply_paths(S, ctx, k, ct, plain, (logn, cls, strict))


def test_plaintext_product_without_fast_plain_lift(S):
    """N = 2^12, key primes of 30, 50, 50 bits + a 51-bit special prime, t a 40-bit odd number (q_0 < t): multiply_plain
    refuses these parameters; the NTT-form product decrypts to m * p in Z_t[x]/(x^N + 1)"""
    logn, n, t = 12, 1 << 12, T40
    p50 = O.ntt_primes_around((1 << 50) - 1, logn)[0]
    kmods = [O.ntt_primes_around((1 << 30) - 1, logn)[0][0], p50[0], p50[1], O.ntt_primes_around((1 << 51) - 1, logn)[0][0]]
    assert kmods[0] < t
    ctx = S.Context(S.SCHEME_BFV, logn, kmods, 1, t, device=0)
    ev = S.Evaluator(ctx)
    ref = O.RefContext(1, logn, kmods, nsp=1, t=t)
    cl = O.Client(ref, seed=7)
    rng = np.random.default_rng(12)
    m = rng.integers(0, t, n, dtype=np.uint64)
    p = rand_plain(rng, t, n)
    assert (p >= np.uint64((t + 1) >> 1)).sum() > n // 4  # the negative half is exercised
    k = cl.k
    ct = cl.encrypt_bfv(m)
    d = ctx.upload(ct)
    with pytest.raises(S.LogicError, match="fast plain lift"):
        ev.multiply_plain_inplace(d, 2, k, 1, ctx.upload(p), plain_stride=n, ntt_form=False)
    ev.transform_to_ntt_inplace(d, 2, k, 1)
    pn = ctx.alloc(k * n)
    ev.transform_plain_to_ntt(ctx.upload(p), n, k, 1, pn)
    ev.multiply_plain_inplace(d, 2, k, 1, pn, plain_stride=0, ntt_form=True)
    ev.transform_from_ntt_inplace(d, 2, k, 1)
    assert np.array_equal(cl.decrypt_bfv(d.download(ct.shape)), O.negacyclic_mod_t(m, p, t))


def test_mod_switch_plain_to(S):
    logn, n, t = 14, 1 << 14, 786433
    mods = primes_for(logn, "fwd_canon")[:2] + [O.ntt_primes_around((1 << 40) - 1, logn)[0][0]]
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, device=0)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(3)
    count = 3
    plains = [rand_plain(rng, t, n) for _ in range(count)]
    full = run_transform(S, ctx, plains, n, 3, count, 0)
    d_full = ctx.upload(full)
    for k_to in (3, 2, 1):
        out = ctx.alloc(count * k_to * n)
        ev.mod_switch_plain_to(d_full, 3, count, k_to, out)
        got = out.download((count, k_to, n))
        assert np.array_equal(got, full[:, :k_to])
        assert np.array_equal(got, run_transform(S, ctx, plains, n, k_to, count, 0))
    # a level-2 ciphertext times the switched plaintext = times the plaintext transformed at level 2
    k = 2
    ct = np.stack([np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in mods[:k]]) for _ in range(2)])
                   for _ in range(count)])
    sw = ctx.alloc(count * k * n)
    ev.mod_switch_plain_to(d_full, 3, count, k, sw)
    direct = ctx.upload(run_transform(S, ctx, plains, n, k, count, 0))
    a, b = ctx.upload(ct), ctx.upload(ct)
    ev.multiply_plain_inplace(a, 2, k, count, sw, plain_stride=k * n, ntt_form=True)
    ev.multiply_plain_inplace(b, 2, k, count, direct, plain_stride=k * n, ntt_form=True)
    assert np.array_equal(a.download(), b.download())
    # in place, one plaintext
    one = ctx.upload(full[:1])
    ev.mod_switch_plain_to(one, 3, 1, 2, one)
    assert np.array_equal(one.download()[:2 * n].reshape(2, n), full[0, :2])
    with pytest.raises(ValueError, match="cannot switch to higher level modulus"):
        ev.mod_switch_plain_to(d_full, 2, 1, 3, out)
    with pytest.raises(ValueError, match="end of modulus switching chain reached"):
        ev.mod_switch_plain_to(d_full, 1, 1, 0, out)


@pytest.mark.parametrize("logn", [10, 14, 15, 16])
def test_empty_batches(S, logn):
    """count 0: S_OK, nothing launched, nothing written -- at every ring size, both entries"""
    n = 1 << logn
    mods = primes_for(logn, "fwd_canon" if logn >= 14 else "any")
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, 786433, device=0)
    ev, L = S.Evaluator(ctx), S.lib()
    sentinel = np.full(3 * n, 0xDEADBEEFCAFEF00D, dtype=np.uint64)
    src = ctx.upload(np.ones(3 * n, dtype=np.uint64))
    out = ctx.upload(sentinel)
    assert L.sealhip_evaluator_transform_plain_to_ntt(ctx.handle, 3, src.ptr, n, 0, 0, out.ptr) == S.S_OK
    assert L.sealhip_evaluator_mod_switch_plain_to(ctx.handle, 3, src.ptr, 0, 2, out.ptr) == S.S_OK
    assert np.array_equal(out.download(), sentinel)


def test_transform_plain_to_ntt_in_a_graph(S):
    """the entry synchronises nothing: it can be captured and replayed"""
    logn, n, t = 14, 1 << 14, 786433
    mods = primes_for(logn, "fwd_canon")
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, device=0)
    ev = S.Evaluator(ctx)
    plains = [rand_plain(np.random.default_rng(9), t, n) for _ in range(2)]
    src = ctx.upload(np.stack(plains))
    out = ctx.alloc(2 * 3 * n)
    g = ctx.capture(lambda: ev.transform_plain_to_ntt(src, n, 3, 2, out))
    src.upload(np.stack(plains[::-1]))
    g.launch()
    assert np.array_equal(out.download((2, 3, n)), expected(plains[::-1], n, t, mods, logn, False))


def _splitmix(state):
    state = (state + 0x9E3779B97F4A7C15) & (2**64 - 1)
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return state, z ^ (z >> 31)


def test_cpp_adapter_plain_methods_match_the_abi(S, tmp_path):
    """tests/host_adapter_plain_check.cpp on the device: its digests equal those of the ABI's outputs on the same inputs"""
    stdout = run_exe(build_plain_adapter(tmp_path), "0", timeout=300)
    mods = [68719230977, 68719403009, 137438822401]
    t, n, cc = 786433, 4096, 3000
    state, plain = 0x9A17 + 5, []
    for _ in range(cc):
        state, z = _splitmix(state)
        plain.append(z % t)
    plain = np.array(plain, dtype=np.uint64)
    ctx = S.Context(S.SCHEME_BFV, 12, mods, 1, t, device=0)
    res = {k: run_transform(S, ctx, [plain], cc, k, 1, 0)[0] for k in (1, 2, 3)}
    for k in (1, 2, 3):
        assert "transform_to_ntt k=%d digest %016x" % (k, O.fnv(res[k])) in stdout, stdout
    assert "transform_to_ntt_inplace k=3 digest %016x words %d ntt 1" % (O.fnv(res[3]), 3 * n) in stdout, stdout
    assert "mod_switch_to_next digest %016x words %d" % (O.fnv(res[2]), 2 * n) in stdout, stdout
    assert "mod_switch_to k=1 digest %016x words %d" % (O.fnv(res[1]), n) in stdout, stdout
    assert "in-place switches agree" in stdout
    # and the oracle agrees with the ABI
    assert np.array_equal(res[3][None], expected([plain], cc, t, mods, 12, False))
