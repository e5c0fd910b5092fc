"""The calls of tests/test_gpu_ks_instances.py cover the instance tables of the key switch's inner products, and the rules
that pick those instances are what the launchers run: checked without a device. The launchers (launch_ks_mac in keyswitch.hip;
launch_hoist_mac, launch_hoist_dot_mac and launch_hoist_giant_mac in hoist.hip; DESIGN.md sections 15 to 17) take their kernel,
item group and grid from the pure functions of gemini-seal_amd/csrc/mac_select.hpp. This file holds the second, independent
statement of those rules, in Python over plain numbers, and tests/mac_select_check.cpp prints what the header's functions
choose: the two must agree call by call, over the GPU file's CASES -- the very records its test walks, imported without the
device module -- and over a grid that reaches every family, group size and threshold. The set of kernels CASES reaches must
be exactly the table. A dropped case, a changed shape or a moved threshold, here or in the header, fails."""
import pytest

import test_gpu_ks_instances as G
from support import CSRC, compile_cpp, run_exe

K_THREADS = 256        # kThreads: lanes of a workgroup
INSTANCES = 16         # template instances ND = 1..16 of each family
MAX_ELTS = 16          # kHoistMaxElts: elements of one launch
FULL_ROUNDS = 4096     # workgroups a larger item group must still leave
KEY_CACHE = 48 << 20   # bytes of key slices above which groups of up to 64 are tried
PAIR_MIN_LOGN = 14     # the pair form reads rows the single-pass NTT wrote: rings of 2^14 and more
PAIR_PREFETCH = 8      # digits up to which the pair form keeps the next ciphertext's words in flight

REFUSED, LOOP, ITEMS, PAIR_FORM = "refused", "loop", "items", "pair"


def shape(call):
    c = G.CONTEXTS[call.ctx]
    n_ct = len(c.bits) - c.nsp
    assert 1 <= call.k <= n_ct, call
    return 1 << c.logn, -(-call.k // c.nsp), call.k + c.nsp


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
    at most 16 elements each, the weighted sum over its elements other than 1"""
    n, nd, rows = shape(call)
    logn = n.bit_length() - 1
    if call.op == "switch":
        return [("ks", logn, nd, rows, 0, call.count, 0, 0, nd, 0)]
    elts = [i for i in call.elts if i >= 0] if call.op == "dot" else list(call.elts)
    op = {"many": "hoist", "dot": "dot"}[call.op]
    return [(op, logn, nd, rows, min(MAX_ELTS, len(elts) - l0), call.count, call.n_sums, 0, nd, 0)
            for l0 in range(0, len(elts), MAX_ELTS)]


# ---------------------------------------------------------------- the kernels the calls of the GPU file reach
def ks_mac(call):
    """count >= 16 over all digits: ks_mac_items_kernel<nd> while there is an instance; else ks_mac_kernel"""
    out = set()
    for line in launches(call):
        family, nd = SELECT[line[0]](*line[1:])[:2]
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


RULES = {"switch": ks_mac, "many": hoist_mac, "dot": hoist_dot_mac}


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
