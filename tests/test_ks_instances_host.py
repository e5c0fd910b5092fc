"""The calls of tests/test_gpu_ks_instances.py cover the instance tables of the key switch's inner products, and the rules
that pick those instances are what the launchers run: checked without a device. The launchers (launch_ks_mac in keyswitch.hip;
launch_hoist_mac, launch_hoist_dot_mac and launch_hoist_giant_mac in hoist.hip; DESIGN.md sections 15 to 17) take their kernel,
item group and grid from the pure functions of gemini-seal_amd/csrc/mac_select.hpp. This file holds the second, independent
statement of those rules, in Python over plain numbers, and tests/mac_select_check.cpp prints what the header's functions
choose: the two must agree call by call, over the GPU file's CASES -- the very records its test walks, imported without the
device module -- and over a grid that reaches every family, group size and threshold. The set of kernels CASES reaches must
be exactly the table. A dropped case, a changed shape or a moved threshold, here or in the header, fails.

Whether a plain key switch takes the pair form is decided in the pipeline (ks_digits in pipeline.cpp, ntt_can_split_last,
select_fwd_half_at), not in the header: pair_admitted restates that decision over the context's own primes, launches() passes
it on as the `pair` request, and the GPU file holds sealhip_debug_ks_split_last to it on every call. The prime sizes it uses
are constants here and are held against ntt_bounds.hpp through tests/ks_split_bounds_check.cpp --bits."""
import functools

import pytest

import oracle_lib as O
import test_gpu_ks_instances as G
from support import CSRC, compile_cpp, run_exe

K_THREADS = 256        # kThreads: lanes of a workgroup
INSTANCES = 16         # template instances ND = 1..16 of each family
MAX_ELTS = 16          # kHoistMaxElts: elements of one launch
FULL_ROUNDS = 4096     # workgroups a larger item group must still leave
KEY_CACHE = 48 << 20   # bytes of key slices above which groups of up to 64 are tried
PAIR_MIN_LOGN = 14     # the pair form reads rows the single-pass NTT wrote: rings of 2^14 and more
PAIR_PREFETCH = 8      # digits up to which the pair form keeps the next ciphertext's words in flight
# bounds:: fwd_split_prime_bits / fwd_lazy_prime_bits per ring (single-pass rings only), kFpPrimeBits, kFpInputBound's size
SPLIT_BITS = {14: 58, 15: 58, 16: 58}
LAZY_BITS = {14: 58, 15: 58, 16: 57}
FP_BITS, FP_INPUT_BITS = 50, 52

REFUSED, LOOP, ITEMS, PAIR_FORM = "refused", "loop", "items", "pair"


def shape(call):
    c = G.CONTEXTS[call.ctx]
    n_ct = len(c.bits) - c.nsp
    assert 1 <= call.k <= n_ct, call
    return 1 << c.logn, -(-call.k // c.nsp), call.k + c.nsp


# ---------------------------------------------------------------- the pair form's admission (the pipeline's decision)
@functools.lru_cache(maxsize=None)
def key_primes(name):
    c = G.CONTEXTS[name]
    return tuple(int(p) for p in O.coeff_modulus_create(1 << c.logn, c.bits))


def digit_launches(name, k):
    """per digit of level k with one special prime: (the primes of the rows its transform writes -- every row of the level
    and the special row but its own --, the load treatment, approximate quotient or not). The treatment is launch-wide: none
    when no source prime exceeds another row's prime, Barrett when one reaches twice another, else one conditional
    subtraction -- which is dropped where the largest prime is inside fwd_lazy_admits."""
    c = G.CONTEXTS[name]
    primes = key_primes(name)
    level = primes[:k] + primes[-1:]
    lazy = lambda p: p.bit_length() <= LAZY_BITS[c.logn]
    pairs = [(level[a], level[b]) for a in range(k) for b in range(len(level)) if a != b]
    treatment = "barrett" if any(ps >= 2 * pd for ps, pd in pairs) else ("condsub" if any(ps > pd for ps, pd in pairs) else "none")
    if treatment == "condsub" and lazy(max(level)):
        treatment = "none"
    out = []
    for j in range(k):
        live = level[:j] + level[j + 1:]
        out.append((live, treatment, all(lazy(p) for p in live)))
    return out


def pair_admitted(name, k, count):
    """one special prime, PARITY (STRICT transforms have no split form), a single-pass ring, a batch and a digit count with a
    pair instance, every live prime of every digit launch inside fwd_split_admits (its size, and nd p < 2^64), and no digit
    launch on the floating-point schedule (every live prime below 2^50 and every key prime below 2^52), which has no split
    form either"""
    c = G.CONTEXTS[name]
    if c.nsp != 1 or c.mode != G.PARITY or c.logn not in SPLIT_BITS or not has_pair_form(c.logn, k, count, 0, k):
        return False
    fp_inputs = all(p.bit_length() <= FP_INPUT_BITS for p in key_primes(name))
    for live, _, _ in digit_launches(name, k):
        if any(p.bit_length() > SPLIT_BITS[c.logn] or k * p >= 1 << 64 for p in live):
            return False
        if fp_inputs and all(p.bit_length() <= FP_BITS for p in live):
            return False
    return True


def split_instances(call):
    """the ntt_fwd_half_kernel<LOGN, sched, treat, SPLIT = true> instances the digit transforms of an admitted call run"""
    c = G.CONTEXTS[call.ctx]
    return {(c.logn, "approx" if apx else "exact", treatment) for _, treatment, apx in digit_launches(call.ctx, call.k)}


# ---------------------------------------------------------------- the rules over plain numbers
# Each returns what the launcher runs: (family, nd, slots, prefetch, group, n_groups, blocks).
def blocks_for(lanes):
    return -(-lanes // K_THREADS) & 0xFFFFFFFF  # (an unsigned grid dimension)


def item_group(logn, nd, rows, n_elts, count):
    """min(count, 8), or 16 (64 when the launch's key slices pass 48 MiB: the largest candidate first) when that still
    leaves 4096 workgroups"""
    n = 1 << logn
    key_bytes = 2 * nd * rows * n_elts * n * 8
    g = 64 if key_bytes > KEY_CACHE else 16
    while g > 8:
        if -(-count // g) * rows * n_elts * n // K_THREADS >= FULL_ROUNDS:
            return g
        g //= 2
    return min(count, 8)


def has_pair_form(logn, nd, count, j0, j1):
    return logn >= PAIR_MIN_LOGN and count >= 16 and (j0, j1) == (0, nd) and 1 <= nd <= INSTANCES


def select_ks_mac(logn, nd, rows, count, j0, j1, pair):
    """count >= 16 over all digits: ks_mac_items_kernel<nd> while there is an instance, or, where the digit rows lack their
    last layer, ks_mac_pair_kernel<nd, nd <= 8> on half the lanes (refused where that form does not exist); else
    ks_mac_kernel"""
    if not 0 <= j0 <= j1 <= nd or (pair and not has_pair_form(logn, nd, count, j0, j1)):
        return (REFUSED, 0, 0, 0, 0, 0, 0)
    if count >= 16 and (j0, j1) == (0, nd) and nd <= INSTANCES:
        group = item_group(logn, nd, rows, 1, count)
        n_groups = -(-count // group)
        lanes = n_groups * rows << logn
        if pair:
            return (PAIR_FORM, nd, 0, int(nd <= PAIR_PREFETCH), group, n_groups, blocks_for(lanes // 2))
        return (ITEMS, nd, 0, 0, group, n_groups, blocks_for(lanes))
    return (LOOP, 0, 0, 0, 0, 0, blocks_for(count * rows << logn))


def hoist_instance(logn, nd):
    """a workgroup fits in a row and nd has an instance"""
    return 1 << logn >= K_THREADS and 1 <= nd <= INSTANCES


def select_hoist_mac(logn, nd, rows, n_elts, count):
    if not 0 <= n_elts <= MAX_ELTS:
        return (REFUSED, 0, 0, 0, 0, 0, 0)
    if not hoist_instance(logn, nd):
        return (LOOP, 0, 0, 0, 0, 0, blocks_for(count * rows * n_elts << logn))
    group = item_group(logn, nd, rows, n_elts, count)
    n_groups = -(-count // group)
    return (ITEMS, nd, 0, 0, group, n_groups, blocks_for(n_groups * rows * n_elts << logn))


def select_hoist_dot_mac(logn, nd, rows, n_elts, count, n_sums):
    """S = n_sums below 3, else 4: a lane's four slots hold S sums of 4 / S ciphertexts"""
    if not 0 <= n_elts <= MAX_ELTS or n_sums < 1:
        return (REFUSED, 0, 0, 0, 0, 0, 0)
    if not hoist_instance(logn, nd):
        return (LOOP, 0, 0, 0, 0, 0, blocks_for(n_sums * count * rows << logn))
    slots = 4 if n_sums >= 3 else n_sums
    n_groups = -(-n_sums // slots) * -(-count // (4 // slots))
    return (ITEMS, nd, slots, 0, 0, n_groups, blocks_for(n_groups * rows << logn))


def select_hoist_giant_mac(logn, nd, rows, n_elts, count):
    """four ciphertexts per lane; the loop kernel below a workgroup or above 16 digits"""
    if not 0 <= n_elts <= MAX_ELTS:
        return (REFUSED, 0, 0, 0, 0, 0, 0)
    if not hoist_instance(logn, nd):
        return (LOOP, 0, 0, 0, 0, 0, blocks_for(count * rows << logn))
    n_groups = -(-count // 4)
    return (ITEMS, nd, 0, 0, 0, n_groups, blocks_for(n_groups * rows << logn))


# a call in plain numbers: (op, logn, nd, rows, n_elts, count, n_sums, j0, j1, pair), the line tests/mac_select_check.cpp reads
SELECT = {
    "ks": lambda logn, nd, rows, n_elts, count, n_sums, j0, j1, pair: select_ks_mac(logn, nd, rows, count, j0, j1, pair),
    "hoist": lambda logn, nd, rows, n_elts, count, n_sums, j0, j1, pair: select_hoist_mac(logn, nd, rows, n_elts, count),
    "dot": lambda logn, nd, rows, n_elts, count, n_sums, j0, j1, pair: select_hoist_dot_mac(logn, nd, rows, n_elts, count, n_sums),
    "giant": lambda logn, nd, rows, n_elts, count, n_sums, j0, j1, pair: select_hoist_giant_mac(logn, nd, rows, n_elts, count),
}


def launches(call):
    """the launches of one Call of the GPU file, as lines of plain numbers: the whole batch and all digits in one launch,
    at most 16 elements each, the weighted sum over its elements other than 1. The plain key switch asks for the pair form
    where pair_admitted says the digit rows lack their last layer. The giant steps (op_apply_galois_bsgs_plain in
    pipeline.cpp, the whole giant list in one pass): an entry per giant other than 1, and per giant at all when some baby is
    not 1 (its acc_j); a launch whenever sixteen entries are gathered and one for what is left after the last."""
    n, nd, rows = shape(call)
    logn = n.bit_length() - 1
    if call.op == "switch":
        return [("ks", logn, nd, rows, 0, call.count, 0, 0, nd, int(pair_admitted(call.ctx, call.k, call.count)))]
    if call.op == "bsgs":
        acc_j = any(i >= 0 for i in call.babies)
        entries = [i for i in call.elts if i >= 0 or acc_j]
        return [("giant", logn, nd, rows, min(MAX_ELTS, len(entries) - l0), call.count, 0, 0, nd, 0)
                for l0 in range(0, len(entries), MAX_ELTS)]
    elts = [i for i in call.elts if i >= 0] if call.op == "dot" else list(call.elts)
    op = {"many": "hoist", "dot": "dot"}[call.op]
    return [(op, logn, nd, rows, min(MAX_ELTS, len(elts) - l0), call.count, call.n_sums, 0, nd, 0)
            for l0 in range(0, len(elts), MAX_ELTS)]


# ---------------------------------------------------------------- the kernels the calls of the GPU file reach
def ks_mac(call):
    """count >= 16 over all digits: ks_mac_items_kernel<nd> while there is an instance -- ks_mac_pair_kernel<nd, nd <= 8> where
    the call is admitted to the pair form, with the item group and the ring (a row's pairs span 32, 64 or 128 workgroups);
    else ks_mac_kernel"""
    n, _, _ = shape(call)
    out = set()
    for line in launches(call):
        family, nd, _, prefetch, group = SELECT[line[0]](*line[1:])[:5]
        assert family != REFUSED, call
        if family == PAIR_FORM:
            out |= {("ks_mac_pair", nd, bool(prefetch)), ("ks_mac_pair ring", n.bit_length() - 1)}
            if group > 8:
                out.add(("ks_mac_pair item group", group, "last group of", call.count % group or group))
        else:
            out.add(("ks_mac_items", nd) if family == ITEMS else ("ks_mac",))
    return out


def loop_reason(n, nd):
    return "ring below a workgroup" if n < K_THREADS else "more than 16 digits"


def hoist_mac(call):
    """per launch of at most 16 elements: hoist_mac_kernel<nd> when a workgroup fits in a row and nd has an instance, with
    the item group min(count, 8), or 16 (64 when the launch's key slices pass 48 MiB: the largest candidate first) when
    that still leaves 4096 workgroups; else the loop kernel"""
    n, nd, rows = shape(call)
    out = set()
    for line in launches(call):
        family, inst, _, _, group = SELECT[line[0]](*line[1:])[:5]
        if family == LOOP:
            out.add(("hoist_mac_loop", loop_reason(n, nd)))
            continue
        out.add(("hoist_mac", inst))
        out.add(("hoist_mac blocks per row", n // K_THREADS))
        if group > 8:
            out.add(("hoist_mac item group", group, "last group of", call.count % group or group))
    return out


def hoist_dot_mac(call):
    """the elements other than 1, at most 16 per launch: S = n_sums below 3, else 4; hoist_dot_mac_kernel<nd, S> under the
    conditions of hoist_mac_kernel, else the loop kernel"""
    n, nd, rows = shape(call)
    out = set()
    for line in launches(call):
        family, inst, slots = SELECT[line[0]](*line[1:])[:3]
        if family == LOOP:
            out.add(("hoist_dot_mac_loop", loop_reason(n, nd)))
        else:
            out |= {("hoist_dot_mac", inst, slots), ("hoist_dot_mac blocks per row", n // K_THREADS)}
    return out


def hoist_giant_mac(call):
    """per launch of at most 16 giants: hoist_giant_mac_kernel<nd> under the conditions of hoist_mac_kernel, four ciphertexts
    per lane; else the loop kernel. (The inner sums of the call run hoist_dot_mac, which the "dot" calls cover.)"""
    n, nd, rows = shape(call)
    out = set()
    for line in launches(call):
        family, inst = SELECT[line[0]](*line[1:])[:2]
        assert family != REFUSED, call
        if family == LOOP:
            out.add(("hoist_giant_mac_loop", loop_reason(n, nd)))
        else:
            out |= {("hoist_giant_mac", inst), ("hoist_giant_mac blocks per row", n // K_THREADS)}
    return out


RULES = {"switch": ks_mac, "many": hoist_mac, "dot": hoist_dot_mac, "bsgs": hoist_giant_mac}


def reached(calls):
    out = set()
    for call in calls:
        out |= RULES[call.op](call)
    return out


def all_calls():
    return [call for calls in G.CASES.values() for call in calls]


def test_the_calls_reach_every_instance():
    ND = range(1, INSTANCES + 1)
    table = {("ks_mac_items", nd) for nd in ND} | {("ks_mac",)}
    table |= {("hoist_mac", nd) for nd in ND}
    table |= {("hoist_mac_loop", "ring below a workgroup"), ("hoist_mac_loop", "more than 16 digits")}
    table |= {("hoist_dot_mac", nd, s) for nd in ND for s in (1, 2, 4)}
    table |= {("hoist_dot_mac_loop", "ring below a workgroup"), ("hoist_dot_mac_loop", "more than 16 digits")}
    table |= {("hoist_mac blocks per row", 1), ("hoist_mac blocks per row", 4)}
    table |= {("hoist_dot_mac blocks per row", 1), ("hoist_dot_mac blocks per row", 4)}
    table |= {("hoist_mac item group", 16, "last group of", 1)}
    table |= {("ks_mac_pair", nd, nd <= PAIR_PREFETCH) for nd in ND}
    table |= {("ks_mac_pair item group", 16, "last group of", 1)}
    table |= {("ks_mac_pair ring", logn) for logn in (14, 15, 16)}
    table |= {("hoist_giant_mac", nd) for nd in ND}
    table |= {("hoist_giant_mac_loop", "ring below a workgroup"), ("hoist_giant_mac_loop", "more than 16 digits")}
    table |= {("hoist_giant_mac blocks per row", 1), ("hoist_giant_mac blocks per row", 4)}
    got = reached(all_calls())
    assert got == table, (sorted(table - got, key=str), sorted(got - table, key=str))


def test_the_sweep_alone_reaches_every_instance_at_sixty_bit_primes():
    """the digit-count sweep does not lean on the other sections: its own calls walk ND = 1..16 of all three families and all
    three slot cuts, and the loop kernels by their digit count"""
    sweep = [call for call in all_calls() if call.ctx == "sweep"]
    got = reached(sweep)
    for nd in range(1, INSTANCES + 1):
        assert {("ks_mac_items", nd), ("hoist_mac", nd)} <= got, nd
        assert {("hoist_dot_mac", nd, s) for s in (1, 2, 4)} <= got, nd
    assert {("ks_mac",), ("hoist_mac_loop", "more than 16 digits"), ("hoist_dot_mac_loop", "more than 16 digits")} <= got
    assert {call.k for call in sweep if call.op == "switch" and call.count < 16} == set(G.SMALL_BATCH_LEVELS)


def test_lane_slots_and_item_groups_of_the_sweep():
    """S = 1 holds four ciphertexts per lane (5 = 4 + 1), S = 2 two (3 = 2 + 1), S = 4 one with n_sums = 3 (the fourth slot
    masked); the plain key switch has item groups 8 + 8 + 1 and the hoisted rotation 8 + 1"""
    sweep = [call for call in all_calls() if call.ctx == "sweep"]
    assert {(call.n_sums, call.count) for call in sweep if call.op == "dot"} == {(1, 5), (2, 3), (3, 2)}
    assert {call.count for call in sweep if call.op == "many"} == {9}
    assert {call.count for call in sweep if call.op == "switch" and call.count >= 16} == {17}
    assert G.compared_items(G.Call("sweep", "switch", 1, 17)) == (0, 7, 8, 15, 16)
    assert G.compared_items(G.Call("sweep", "many", 1, 9, G.PAIR)) == (0, 7, 8)
    assert G.compared_items(G.Call("sweep", "dot", 1, 5, G.AROUND_ONE, 1)) == (0, 1, 2, 3, 4)
    # (what the docstring says of the groups is what the rule gives: 3 groups of 8 for 17 ciphertexts, 2 for 9)
    assert {select_ks_mac(10, nd, nd + 1, 17, 0, nd, 0)[4:6] for nd in range(1, INSTANCES + 1)} == {(8, 3)}
    assert {select_hoist_mac(10, nd, nd + 1, 2, 9)[4:6] for nd in range(1, INSTANCES + 1)} == {(8, 2)}


def test_digit_mapping_contexts():
    """nsp = 3: every level of twelve primes, so last bundles of one, two and three rows; nsp = 9: a bundle of nine next to a
    bundle of one (level 10), a single bundle of nine, a single bundle of one"""
    for name, levels in (("nsp3", set(range(1, 13))), ("nsp9", {10, 9, 1})):
        calls = [call for call in all_calls() if call.ctx == name]
        for op in RULES:
            assert {call.k for call in calls if call.op == op} == levels, (name, op)
        assert {call.count for call in calls if call.op == "switch"} == {17, 2}
    c = G.CONTEXTS["nsp9"]
    assert c.nsp == 9 and len(c.bits) == 19 and G.CONTEXTS["nsp3"].nsp == 3 and len(G.CONTEXTS["nsp3"].bits) == 15


def test_the_extremes_fill_a_launch_and_cross_it():
    """61-bit primes throughout; 16 elements other than 1 in one launch, 17 for a second launch that adds, the identity as
    the 4th and 8th term"""
    assert set(G.CONTEXTS["extreme"].bits) == {61}
    lists = [call.elts for call in G.CASES["extremes_dot"]]
    assert all(call.extreme and call.k == 16 for call in G.CASES["extremes_dot"] + G.CASES["extremes_switch_many"])
    assert any(len(e) == 16 and len(set(e)) == 16 and min(e) >= 0 for e in lists)
    assert any(len(e) == 17 and len(set(e)) == 17 and min(e) >= 0 for e in lists)
    assert any([i for i, g in enumerate(e) if g < 0] == [3, 7] for e in lists)
    assert {call.n_sums for call in G.CASES["extremes_dot"]} == {1, 2, 3}


def test_the_giant_sweep_alone_reaches_every_instance():
    """five ciphertexts (a lane's four slots and a group of one) at every level: ND = 1..16 and the loop kernel at 17, each
    launch with the acc_j path, a non-identity giant and the identity giant; babies all 1 on a few levels"""
    sweep = [call for call in all_calls() if call.ctx == "sweep" and call.op == "bsgs"]
    got = reached(sweep)
    assert {("hoist_giant_mac", nd) for nd in range(1, INSTANCES + 1)} | {("hoist_giant_mac_loop", "more than 16 digits")} <= got
    assert {call.count for call in sweep} == {5}
    assert {select_hoist_giant_mac(10, nd, nd + 1, 3, 5)[5] for nd in range(1, INSTANCES + 1)} == {2}
    with_acc = [call for call in sweep if call.babies == G.BABIES]
    assert {call.k for call in with_acc} == set(range(1, 18)) and {call.elts for call in with_acc} == {G.GIANTS}
    assert G.GIANTS.count(-1) == 1 and len([i for i in G.GIANTS if i >= 0]) == 2 and G.BABIES == (0, -1)
    assert {call.k for call in sweep if call.babies == G.NO_BABIES} == set(G.SMALL_BATCH_LEVELS)
    assert all(len(launches(call)) == 1 for call in sweep)


def test_the_giant_extremes_fill_a_launch_and_cross_it():
    """61-bit primes at level 16, three ciphertexts; sixteen distinct giants other than 1 in one launch, seventeen in two (the
    second of one giant), the identity as 4th and 8th giant, and sixteen giants under babies all 1"""
    calls = G.CASES["extremes_bsgs"]
    assert all(call.ctx == "extreme" and call.extreme and call.k == 16 and call.count == 3 for call in calls)
    cut = {(call.elts, call.babies): [line[4] for line in launches(call)] for call in calls}
    sixteen, seventeen = tuple(range(16)), tuple(range(17))
    assert cut[sixteen, G.BABIES] == [16] and cut[seventeen, G.BABIES] == [16, 1] and cut[sixteen, G.NO_BABIES] == [16]
    (with_identity,) = [e for e, b in cut if -1 in e]
    assert [i for i, g in enumerate(with_identity) if g < 0] == [3, 7] and cut[with_identity, G.BABIES] == [len(with_identity)]
    assert len(G.elements(1 << G.CONTEXTS["extreme"].logn)) == 17 and 1 not in G.elements(1 << G.CONTEXTS["extreme"].logn)
    # (without acc_j an identity giant is no entry of the launch)
    assert [line[4] for line in launches(G.Call("extreme", "bsgs", 16, 3, with_identity, babies=G.NO_BABIES))] == [8]


# ---------------------------------------------------------------- the pair form
def pair_calls():
    return [call for call in all_calls() if call.op == "switch" and pair_admitted(call.ctx, call.k, call.count)]


def test_the_pair_form_is_taken_where_it_is_meant_to_be():
    """every "switch" call of the pair contexts from 16 ciphertexts on and none of the others: more than one special prime,
    STRICT, the rings below 2^14 and the 59- to 61-bit chains stay on the whole-row kernels"""
    admitted = {call.ctx for call in pair_calls()}
    assert admitted == {name for name in G.CONTEXTS if name.startswith("pair")}
    for call in all_calls():
        if call.op == "switch" and call.ctx in admitted:
            assert call.count >= 16 and pair_admitted(call.ctx, call.k, call.count), call
    # the same chains in STRICT mode, with two special primes or one prime wider are refused by the rule
    c = G.CONTEXTS["pair"]
    try:
        G.CONTEXTS["_strict"] = c._replace(mode=G.STRICT)
        G.CONTEXTS["_nsp2"] = c._replace(nsp=2)
        G.CONTEXTS["_wide"] = c._replace(bits=[55] * 15 + [59, 56])
        G.CONTEXTS["_fp"] = c._replace(bits=[45] * 3 + [46])
        assert pair_admitted("pair", 16, 16) and not pair_admitted("pair", 16, 15)
        assert not pair_admitted("_strict", 8, 17) and not pair_admitted("_nsp2", 8, 17) and not pair_admitted("_fp", 3, 17)
        assert pair_admitted("_wide", 15, 17) and not pair_admitted("_wide", 16, 17)
    finally:
        for name in ("_strict", "_nsp2", "_wide", "_fp"):
            G.CONTEXTS.pop(name, None)


def test_the_pair_sweep_alone_reaches_every_instance():
    """nd = 1..16 with the prefetch up to 8 digits; 19 ciphertexts on every level (groups 8 + 8 + 3: the two-per-trip loop ends
    on an odd group longer than one), 17 on the first and last level and both sides of the prefetch threshold (8 + 8 + 1), 16
    on level 9; relinearize on those four levels at least"""
    sweep = [call for call in all_calls() if call.ctx == "pair"]
    assert all(call.op == "switch" for call in sweep)
    assert {("ks_mac_pair", nd, nd <= PAIR_PREFETCH) for nd in range(1, INSTANCES + 1)} <= reached(sweep)
    assert {call.k for call in sweep if call.count == 19} == set(range(1, 17))
    assert {call.k for call in sweep if call.count == 17} == {1, 8, 9, 16} == {call.k for call in sweep if call.relin}
    assert {call.k for call in sweep if call.count == 16} == {9}
    for count, last in ((19, 3), (17, 1), (16, 8)):
        choices = {select_ks_mac(14, nd, nd + 1, count, 0, nd, 1)[4:6] for nd in range(1, INSTANCES + 1)}
        assert choices == {(8, -(-count // 8))} and count - 8 * (-(-count // 8) - 1) == last
    assert G.compared_items(G.Call("pair", "switch", 1, 19)) == (0, 7, 8, 15, 16, 18)
    # BFV on the same chain: relinearize on the same four levels
    assert {(call.k, call.count, call.relin) for call in all_calls() if call.ctx == "pair_bfv"} == {(k, 17, True) for k in (1, 8, 9, 16)}
    assert G.CONTEXTS["pair_bfv"].bits == G.CONTEXTS["pair"].bits and G.CONTEXTS["pair_bfv"].mode == G.PARITY


def test_the_split_transform_instances_the_pair_calls_run():
    """the six (schedule, treatment) cells of ntt_fwd_half_kernel's SPLIT form are not all reachable through the pipeline at
    every ring (tests/test_ks_split_last.py launches all six per ring by themselves); the calls run: the approximate
    schedule without a treatment at every ring and with Barrett at 2^15, and at 2^16, where a 58-bit prime is outside
    fwd_lazy_admits, the exact schedule with each of the three treatments -- the one place the conditional subtraction
    survives. (2^14 with Barrett runs in tests/test_ks_split_last.py; at 2^16 the 40 + 55 | 58 chain is on the exact schedule.)"""
    got = set()
    for call in pair_calls():
        got |= split_instances(call)
    want = {(logn, "approx", "none") for logn in (14, 15, 16)} | {(15, "approx", "barrett")}
    want |= {(16, "exact", t) for t in ("none", "barrett", "condsub")}
    assert got == want, (sorted(want - got), sorted(got - want))
    first_level = G.Call("pair16_p58", "switch", 2, 17)
    assert first_level in pair_calls() and split_instances(first_level) == {(16, "exact", "condsub")}


def test_the_pair_extremes_use_the_widest_admitted_primes(bounds_exe):
    """every prime of the context has the size fwd_split_admits stops at, read from ntt_bounds.hpp through the check program;
    one bit more is refused by the rule; sixteen digits, 17 and 16 ciphertexts, extreme inputs"""
    bits = program_bits(bounds_exe)
    c = G.CONTEXTS["pair58"]
    assert set(c.bits) == {bits["split"][c.logn]} and len(c.bits) == 17
    assert {p.bit_length() for p in key_primes("pair58")} == {bits["split"][c.logn]}
    calls = G.CASES["pair_extremes"]
    assert {(call.k, call.count, call.extreme) for call in calls} == {(16, 17, True), (16, 16, True)}
    assert all(pair_admitted(call.ctx, call.k, call.count) for call in calls)
    try:
        G.CONTEXTS["_above"] = c._replace(bits=[bits["split"][c.logn] + 1] * 17)
        assert not pair_admitted("_above", 16, 17)
    finally:
        G.CONTEXTS.pop("_above", None)


def test_the_item_group_of_sixteen_in_the_pair_form():
    (call,) = G.CASES["pair_group16"]
    n, nd, rows = shape(call)
    choice = select_ks_mac(14, nd, rows, call.count, 0, nd, 1)
    assert choice[0] == PAIR_FORM and choice[4:6] == (16, 16) and call.count % 16 == 1
    assert 16 * rows * n // K_THREADS == FULL_ROUNDS and select_ks_mac(14, nd, rows, call.count - 1, 0, nd, 1)[4] == 8
    assert G.compared_items(call) == (0, 15, 16, 239, 240)


@pytest.fixture(scope="module")
def bounds_exe(tmp_path_factory):
    return compile_cpp(tmp_path_factory.mktemp("split_bits"), "ks_split_bounds_check.cpp")


def program_bits(exe):
    """tests/ks_split_bounds_check.cpp --bits: {"split": {logn: bits}, "lazy": {logn: bits}, "fp": bits, "input": bits}"""
    out = {"split": {}, "lazy": {}}
    for line in run_exe(exe, "--bits", timeout=60).splitlines():
        w = line.split()
        if w[0] == "ring":
            out["split"][int(w[1])], out["lazy"][int(w[1])] = int(w[3]), int(w[5])
        else:
            out["fp"], out["input"] = int(w[1]), int(w[3])
    return out


def test_the_prime_sizes_here_are_the_header_s(bounds_exe):
    bits = program_bits(bounds_exe)
    assert bits == {"split": SPLIT_BITS, "lazy": LAZY_BITS, "fp": FP_BITS, "input": FP_INPUT_BITS}


# ---------------------------------------------------------------- the header's functions against the rules above
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return compile_cpp(tmp_path_factory.mktemp("mac_select"), "mac_select_check.cpp", extra=("-I", CSRC))


def grid_lines():
    """rings 2^6..2^16 x 1..17 digits x batches around 8, 16 and the 4096-workgroup cut: the plain key switch over all
    digits, digit ranges and refused ranges, with and without the pair request; the hoisted launchers at 1, 3, 16 and 17
    elements, the weighted sum at 1..5 sums"""
    counts = (1, 7, 8, 15, 16, 17, 49, 256, 1000, 4096)
    for logn in range(6, 17):
        for nd in range(1, 18):
            for nsp in (1, 3):
                rows = nd * nsp + nsp
                for count in counts:
                    for j0, j1 in ((0, nd), (1, nd), (0, nd - 1), (0, nd + 1), (-1, nd)):
                        for pair in (0, 1):
                            yield ("ks", logn, nd, rows, 0, count, 0, j0, j1, pair)
                    for n_elts in (1, 3, 16, 17):
                        yield ("hoist", logn, nd, rows, n_elts, count, 0, 0, nd, 0)
                        yield ("giant", logn, nd, rows, n_elts, count, 0, 0, nd, 0)
                    for n_sums in (1, 2, 3, 4, 5):
                        yield ("dot", logn, nd, rows, 2, count, n_sums, 0, nd, 0)


def test_the_header_and_the_rules_here_agree_call_by_call(exe, tmp_path):
    """tests/mac_select_check.cpp evaluates mac_select.hpp -- the functions the launchers call -- on every launch of CASES and
    on the grid; each choice (family, nd, S, prefetch, item group, groups, grid) equals what the rules of this file give"""
    lines = [line for call in all_calls() for line in launches(call)] + list(grid_lines())
    path = tmp_path / "calls.txt"
    path.write_text("".join(" ".join(str(v) for v in line) + "\n" for line in lines))
    got = run_exe(exe, "--calls", path, timeout=120).splitlines()
    assert len(got) == len(lines)
    families, prefetch = set(), set()
    for line, out in zip(lines, got):
        want = SELECT[line[0]](*line[1:])
        assert out == " ".join(str(v) for v in want), (line, out, want)
        families.add((line[0], want[0], want[4]))
        if want[0] == PAIR_FORM:
            prefetch.add((want[1] <= PAIR_PREFETCH, want[3]))
    # the grid is not vacuous: every family of every launcher, the pair form with and without its prefetch, every group size
    assert {(op, f) for op, f, _ in families} == {("ks", REFUSED), ("ks", LOOP), ("ks", ITEMS), ("ks", PAIR_FORM), ("hoist", REFUSED),
                                                  ("hoist", LOOP), ("hoist", ITEMS), ("dot", LOOP), ("dot", ITEMS),
                                                  ("giant", REFUSED), ("giant", LOOP), ("giant", ITEMS)}
    assert {g for op, f, g in families if op == "ks" and f in (ITEMS, PAIR_FORM)} == {8, 16, 32, 64}
    assert {g for op, f, g in families if op == "hoist" and f == ITEMS} >= {1, 7, 8, 16, 32, 64}
    assert prefetch == {(True, 1), (False, 0)}


def test_select_program_checks_its_invariants(exe):
    """the header's own invariants over rings 2^6..2^16, 1..17 digits, 1..16 elements: the group is min(count, 8), 16, 32 or
    64, a group above 8 leaves 4096 workgroups and no larger candidate would, the pair form only inside
    ks_mac_has_pair_form, instances only up to 16 digits, and the dispatchers call the instance of the value and no other"""
    assert "mac_select_check: OK" in run_exe(exe, timeout=120)


def test_select_program_under_sanitizers(tmp_path):
    """mac_select.hpp and instance_dispatch.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = compile_cpp(tmp_path, "mac_select_check.cpp", sanitize=True)
    assert "mac_select_check: OK" in run_exe(exe, timeout=300)
