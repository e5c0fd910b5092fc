"""The calls of tests/test_gpu_ks_instances.py cover the instance tables of the key switch's inner products: checked without
a device. The selection rules of launch_ks_mac (keyswitch.hip), launch_hoist_mac and launch_hoist_dot_mac (hoist.hip; DESIGN.md
sections 15 and 16) are restated here over the GPU file's CASES -- the very records its test walks, imported without the
device module -- and the set of kernels they reach must be exactly the table. A dropped case, a changed shape or a moved
threshold in the rules below changes the set."""
import test_gpu_ks_instances as G

K_THREADS = 256        # kThreads: lanes of a workgroup
INSTANCES = 16         # template instances ND = 1..16 of each family
MAX_ELTS = 16          # kHoistMaxElts: elements of one launch
FULL_ROUNDS = 4096     # workgroups a larger item group must still leave


def shape(call):
    c = G.CONTEXTS[call.ctx]
    n_ct = len(c.bits) - c.nsp
    assert 1 <= call.k <= n_ct, call
    return 1 << c.logn, -(-call.k // c.nsp), call.k + c.nsp


def ks_mac(call):
    """count >= 16 over all digits: ks_mac_items_kernel<nd> while there is an instance; else ks_mac_kernel"""
    n, nd, rows = shape(call)
    if call.count >= 16 and nd <= INSTANCES:
        return {("ks_mac_items", nd)}
    return {("ks_mac",)}


def hoist_mac(call):
    """per launch of at most 16 elements: hoist_mac_kernel<nd> when a workgroup fits in a row and nd has an instance, with
    the item group min(count, 8), or 16 (64 when the launch's key slices pass 48 MiB: the largest candidate first) when
    that still leaves 4096 workgroups; else the loop kernel"""
    n, nd, rows = shape(call)
    out = set()
    for l0 in range(0, len(call.elts), MAX_ELTS):
        n_elts = min(MAX_ELTS, len(call.elts) - l0)
        if n < K_THREADS:
            out.add(("hoist_mac_loop", "ring below a workgroup"))
            continue
        if nd > INSTANCES:
            out.add(("hoist_mac_loop", "more than 16 digits"))
            continue
        key_bytes = 2 * nd * rows * n_elts * n * 8
        group, g = min(call.count, 8), 64 if key_bytes > 48 << 20 else 16
        while g > 8:
            if -(-call.count // g) * rows * n_elts * n // K_THREADS >= FULL_ROUNDS:
                group = g
                break
            g //= 2
        out.add(("hoist_mac", nd))
        out.add(("hoist_mac blocks per row", n // K_THREADS))
        if group > 8:
            out.add(("hoist_mac item group", group, "last group of", call.count % group or group))
    return out


def hoist_dot_mac(call):
    """the elements other than 1, at most 16 per launch: S = n_sums below 3, else 4; hoist_dot_mac_kernel<nd, S> under the
    conditions of hoist_mac_kernel, else the loop kernel"""
    n, nd, rows = shape(call)
    if all(i < 0 for i in call.elts):
        return set()
    slots = 4 if call.n_sums >= 3 else call.n_sums
    if n < K_THREADS:
        return {("hoist_dot_mac_loop", "ring below a workgroup")}
    if nd > INSTANCES:
        return {("hoist_dot_mac_loop", "more than 16 digits")}
    return {("hoist_dot_mac", nd, slots), ("hoist_dot_mac blocks per row", n // K_THREADS)}


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
