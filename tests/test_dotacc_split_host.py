"""csrc/dotacc.hpp with the split position as a parameter, on the host: DotAccSplit<S, ...> at S = 30 and S = 31 is plain
64-bit arithmetic, so the header the kernels include runs here against unsigned __int128 (tests/dotacc_split_check.cpp):
every dot product of every exact-k BEHZ instance and every term count 1..17, operands at the maxima of each operand
class (the floor rows' x at 2p - 1 for the largest 60-bit prime), zero, alternating and seeded random; every accumulator
below 2^64, the assembled sum exact, the accumulator counts the fewest the bounds function admits; the level predicate
at its edge (the widest primes admitted at S = 30 run without a wrap, the narrowest refused wrap an accumulator and get
S = 31); the packed constant round-trips at both splits."""
import pytest

from support import CSRC, compile_cpp, run_exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_dotacc_split_against_int128(tmp_path, sanitize):
    """both flavours with warnings as errors; the plain one sees csrc/ too"""
    extra = ("-Wall", "-Werror") + (() if sanitize else ("-I", CSRC))
    exe = compile_cpp(tmp_path, "dotacc_split_check.cpp", sanitize=sanitize, extra=extra)
    assert "dotacc_split_check: OK" in run_exe(exe, timeout=300)


# ---- the selection restated in plain integers (ntt_bounds.hpp section 5), independent of the header
def _parts(bits, s):
    return (1 << min(bits, s)) - 1, ((1 << (bits - s)) - 1 if bits > s else 0)


def _worst(s, shape, counts):
    """largest worst-case accumulator sum per part (L, M, H) of a dot product {nterms, first, lane, const bits} whose
    products are dealt round-robin over `counts` accumulators per part"""
    nterms, first, lane, cst = shape
    c0, c1 = _parts(cst, s)
    acc = [[0] * c for c in counts]
    for i in range(nterms):
        t0, t1 = _parts(first if i == 0 else lane, s)
        acc[0][i % counts[0]] += t0 * c0
        acc[1][(2 * i) % counts[1]] += t0 * c1
        acc[1][(2 * i + 1) % counts[1]] += t1 * c0
        acc[2][i % counts[2]] += t1 * c1
    return [max(a) for a in acc]


def _fewest(s, shape):
    counts = []
    for part in range(3):
        c = 1
        while _worst(s, shape, [c] * 3)[part] >= 1 << 64:
            c += 1
        counts.append(c)
    return counts


def _shapes(k, qb, bb):
    """lift row, floor Bsk row (x below 2 b), conv_sk, floor q row"""
    return (k + 1, bb, qb, bb), (k + 1, bb + 1, qb, bb), (k + 1, bb, bb, bb), (k + 2, bb, bb, qb)


def select_split(k, qb, bb=60):
    """30 where the S = 30 instances -- accumulators sized for 59-bit ciphertext and 60-bit auxiliary primes -- cannot wrap
    on primes of qb and bb bits; the exact-k instances end at k = 15"""
    if k > 15:
        return 31
    for built, have in zip(_shapes(k, 59, 60), _shapes(k, qb, bb)):
        if max(_worst(30, have, _fewest(30, built))) >= 1 << 64:
            return 31
    return 30


def test_split_selected_per_level_on_host_only_contexts():
    """sealhip_debug_behz_dot_split on host-only contexts at N = 2^14 (60-bit auxiliary primes) against the restatement
    above, for ciphertext primes of 50, 58, 59 (the fused tensor path's widest), 60 and 61 bits at every level 1..16.
    58- and 59-bit primes take S = 30 at every exact-k level; at 60 bits the floor rows' 2 k + 3 cross products of 2^60
    pass 16 from k = 7 on, where S = 31 is kept. The plan entry keeps its thirteen fields."""
    import oracle_lib as O
    import sealhip as S

    n, nkey = 1 << 14, 17
    aux = set(int(p) for p in O.aux_primes(n, nkey + 3))
    assert [select_split(k, 58) for k in (1, 7, 8, 15, 16)] == [30, 30, 30, 30, 31]
    assert [select_split(k, 59) for k in range(1, 16)] == [30] * 15
    assert [select_split(k, 60) for k in (1, 6, 7, 8, 15)] == [30, 30, 31, 31, 31]
    for bits in (50, 58, 59, 60, 61):
        mods = [p for p in O.ntt_primes_below(n, 1 << bits, 2 * nkey + 3) if int(p) not in aux][:nkey]
        assert all(int(p).bit_length() == bits for p in mods)
        ctx = S.Context(S.SCHEME_BFV, 14, mods, 1, O.BFV_PLAN_T[0], device=-1)
        got = [ctx.debug_behz_dot_split(k) for k in range(1, 17)]
        assert got == [select_split(k, bits) for k in range(1, 17)], (bits, got)
        assert len(ctx.debug_bfv_multiply_plan(7)) == len(S.Context.BFV_PLAN_FIELDS) == 13
