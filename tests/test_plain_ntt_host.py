"""transform_to_ntt(Plaintext) on the device (sealhip_evaluator_transform_plain_to_ntt, sealhip_evaluator_mod_switch_plain_to):
what can be checked without a GPU. The lift formula of the device path (poly.hip plain_lift_centered_kernel) against a
literal restatement of the reference's two branches (evaluator.cpp:1682-1737) in Python integers; the new entries on a
host-only context; and the C++ adapter's host checks with the reference's messages."""
import numpy as np
import pytest

import oracle_lib as O
from support import compile_cpp, run_exe


# ------------------------------------------------------------------ the reference's two branches, restated literally
def ref_lift_fast(v, t, qs):
    """using_fast_plain_lift (every q_i > t): plain_upper_half_increment holds q_i - t per prime (context.cpp:316-340);
    row i = v + (increment_i & -(v >= thr)) (evaluator.cpp:1721-1736)"""
    thr = (t + 1) >> 1
    assert all(q > t for q in qs)
    return [v + ((q - t) if v >= thr else 0) for q in qs]


def ref_lift_general(v, t, qs):
    """otherwise: the multi-word increment Q - t added to v (add_uint over coeff_modulus_size words) for v >= thr, else v
    itself, then base_q->decompose_array: the residues of that integer (evaluator.cpp:1691-1714)"""
    thr = (t + 1) >> 1
    Q = 1
    for q in qs:
        Q *= q
    words = len(qs)
    val = (v + (Q - t)) if v >= thr else v
    assert val < 1 << (64 * words)  # the k-word temporary holds it
    return [val % q for q in qs]


def formula(v, t, q):
    """the canonical residue of the centred value"""
    return (v - t * (v >= (t + 1) >> 1)) % q


def barrett_reduce_63(x, q):
    """devmath.hpp barrett_reduce_63 with cr1 = the high word of floor(2^128 / q) (modulus.cpp:85-96)"""
    assert x < 1 << 63
    cr1 = ((1 << 128) // q) >> 64
    r = x - ((x * cr1) >> 64) * q
    return r - q if r >= q else r


def kernel_lift(v, t, q):
    """what the kernels compute: barrett_reduce_63(v + (q - t mod q) [v >= thr])"""
    inc = q - barrett_reduce_63(t, q)
    x = v + (inc if v >= (t + 1) >> 1 else 0)
    return barrett_reduce_63(x, q)


def _prime_sets():
    top = lambda bits, logn=12: O.ntt_primes_around((1 << bits) - 1, logn)[0]
    return {
        "30bit": top(30)[:2],
        "36_37": top(36)[:2] + top(37)[:1],
        "50bit": top(50),
        "60bit": top(60),
        "61bit": top(61)[:2],
        "mixed": [top(30)[0], top(60)[0], top(61)[0]],
        "tiny": [O.ntt_primes_around(1 << 17, 3)[0][0], O.ntt_primes_around(1 << 20, 3)[0][0]],
    }


T_VALUES = {"2": 2, "2^20": 1 << 20, "786433": 786433, "40bit": (1 << 40) - 87, "60bit": (1 << 60) - 93, "2^61-1": (1 << 61) - 1}


@pytest.mark.parametrize("tname", sorted(T_VALUES))
def test_lift_formula_equals_both_reference_branches(tname):
    t = T_VALUES[tname]
    thr = (t + 1) >> 1
    rng = np.random.default_rng(len(tname) * 1009 + t % 997)
    vals = sorted({0, max(thr - 1, 0), thr, t - 1, 1 % t} | {int(x) for x in rng.integers(0, t, 40, dtype=np.uint64)})
    fast_seen = general_seen = 0
    for name, qs in _prime_sets().items():
        fast = all(q > t for q in qs)
        for v in vals:
            want = [formula(v, t, q) for q in qs]
            assert ref_lift_general(v, t, qs) == want, (name, t, v)
            if fast:
                assert ref_lift_fast(v, t, qs) == want, (name, t, v)
            assert [kernel_lift(v, t, q) for q in qs] == want, (name, t, v)
        fast_seen += fast
        general_seen += not fast
    if t > 1 << 17:
        assert general_seen > 0  # the larger t meet prime sets without fast plain lift
    if t < 1 << 29:
        assert fast_seen > 0


def test_lift_formula_covers_the_negative_half():
    """thr - 1 maps to itself, thr to thr - t (negative, so q - (t - thr)): the two sides of the split differ"""
    t, q = 786433, O.ntt_primes_around((1 << 36) - 1, 12)[0][0]
    thr = (t + 1) >> 1
    assert kernel_lift(thr - 1, t, q) == thr - 1
    assert kernel_lift(thr, t, q) == q - (t - thr)
    assert kernel_lift(t - 1, t, q) == q - 1


# ------------------------------------------------------------------ the ABI on a host-only context
def _host_ctx(S, scheme=None, t=65537):
    logn, n = 6, 64
    mods = O.coeff_modulus_create(n, [30, 30, 30])
    scheme = S.SCHEME_BFV if scheme is None else scheme
    return S.Context(scheme, logn, mods, 1, t if scheme == S.SCHEME_BFV else 0, device=-1), n


def test_new_exports_exist():
    import sealhip as S

    L = S.lib()
    for name in ("sealhip_evaluator_transform_plain_to_ntt", "sealhip_evaluator_mod_switch_plain_to"):
        assert hasattr(L, name) and name in S.SYMBOLS
    for name in ("transform_plain_to_ntt", "mod_switch_plain_to"):
        assert callable(getattr(S.Evaluator, name))


def test_transform_plain_to_ntt_on_host_only_context():
    import sealhip as S

    ctx, n = _host_ctx(S)
    ev, L = S.Evaluator(ctx), S.lib()
    plain = np.zeros(4 * n, dtype=np.uint64)
    out = np.zeros(4 * 3 * n, dtype=np.uint64)
    pp, po = plain.ctypes.data, out.ctypes.data
    # null pointers first, before anything else is looked at (also with otherwise invalid arguments)
    with pytest.raises(TypeError):
        S._check(L.sealhip_evaluator_transform_plain_to_ntt(None, 2, pp, n, 0, 1, po))
    with pytest.raises(TypeError):
        S._check(L.sealhip_evaluator_transform_plain_to_ntt(ctx.handle, 99, None, n, 0, 1, po))
    with pytest.raises(TypeError):
        S._check(L.sealhip_evaluator_transform_plain_to_ntt(ctx.handle, 99, pp, n + 1, 0, 1, None))
    # the argument errors need no device
    for k in (0, 4):
        with pytest.raises(ValueError, match="level k out of range"):
            ev.transform_plain_to_ntt(pp, n, k, 1, po)
    with pytest.raises(ValueError, match="plain is not valid for encryption parameters"):
        ev.transform_plain_to_ntt(pp, n + 1, 2, 1, po)
    with pytest.raises(ValueError, match="plain_stride is smaller than one plaintext"):
        ev.transform_plain_to_ntt(pp, n // 2, 2, 2, po, plain_stride=n // 2 - 1)
    with pytest.raises(ValueError, match="overlap"):
        ev.transform_plain_to_ntt(pp, n, 1, 2, pp + 8 * n)
    # valid arguments, count 0 included: the entry itself needs a device
    for count in (1, 0):
        with pytest.raises(S.LogicError, match="host-only"):
            ev.transform_plain_to_ntt(pp, n, 2, count, po)
    with pytest.raises(S.LogicError, match="host-only"):
        ev.transform_plain_to_ntt(pp, 3, 3, 2, po, plain_stride=5)


def test_transform_plain_to_ntt_ckks_rejects_coefficient_plaintexts():
    import sealhip as S

    ctx, n = _host_ctx(S, S.SCHEME_CKKS)
    ev = S.Evaluator(ctx)
    plain = np.zeros(n, dtype=np.uint64)
    out = np.zeros(3 * n, dtype=np.uint64)
    with pytest.raises(ValueError, match="plain is not valid for encryption parameters"):
        ev.transform_plain_to_ntt(plain.ctypes.data, 1, 2, 1, out.ctypes.data)
    with pytest.raises(S.LogicError, match="host-only"):  # an empty plaintext is valid (zero rows)
        ev.transform_plain_to_ntt(plain.ctypes.data, 0, 2, 1, out.ctypes.data)


def test_mod_switch_plain_to_on_host_only_context():
    import sealhip as S

    ctx, n = _host_ctx(S)
    ev, L = S.Evaluator(ctx), S.lib()
    plain = np.zeros(2 * 3 * n, dtype=np.uint64)
    out = np.zeros(2 * 3 * n, dtype=np.uint64)
    pp, po = plain.ctypes.data, out.ctypes.data
    with pytest.raises(TypeError):
        S._check(L.sealhip_evaluator_mod_switch_plain_to(None, 3, pp, 1, 2, po))
    with pytest.raises(TypeError):
        S._check(L.sealhip_evaluator_mod_switch_plain_to(ctx.handle, 3, None, 1, 9, po))
    with pytest.raises(TypeError):
        S._check(L.sealhip_evaluator_mod_switch_plain_to(ctx.handle, 3, pp, 1, 9, None))
    with pytest.raises(ValueError, match="cannot switch to higher level modulus"):
        ev.mod_switch_plain_to(pp, 2, 1, 3, po)
    with pytest.raises(ValueError, match="end of modulus switching chain reached"):
        ev.mod_switch_plain_to(pp, 2, 1, 0, po)
    with pytest.raises(ValueError, match="level k out of range"):
        ev.mod_switch_plain_to(pp, 4, 1, 1, po)
    with pytest.raises(ValueError, match="overlap"):
        ev.mod_switch_plain_to(pp, 3, 2, 2, pp + 8)
    for count in (1, 0):
        with pytest.raises(S.LogicError, match="host-only"):
            ev.mod_switch_plain_to(pp, 3, count, 1, po)
    with pytest.raises(S.LogicError, match="host-only"):  # in place, one plaintext: every word stays where it is
        ev.mod_switch_plain_to(pp, 3, 1, 2, pp)


# ------------------------------------------------------------------ the C++ adapter
def build_plain_adapter(tmp_path):
    return compile_cpp(tmp_path, "host_adapter_plain_check.cpp", link_sealhip=True)


def test_cpp_adapter_plain_checks_on_host_only_context(tmp_path):
    """transform_to_ntt(_inplace) / mod_switch_to(_next)(_inplace) of plaintexts: is_valid_for (valcheck.cpp:236-281), "plain
    is already in NTT form", "plain is not in NTT form", "cannot switch to higher level modulus", "end of modulus switching
    chain reached" as std::invalid_argument; a valid call is refused by the host-only context"""
    assert "host-only plain checks ok" in run_exe(build_plain_adapter(tmp_path), timeout=120)
