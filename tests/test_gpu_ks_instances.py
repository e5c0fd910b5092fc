"""The key switch's inner products at every instance of their launchers, word for word against the CPU oracle.

launch_ks_mac (keyswitch.hip), launch_hoist_mac, launch_hoist_dot_mac and launch_hoist_giant_mac (hoist.hip) pick a template
instance from the level's digit count nd = ceil(k / nsp): ks_mac_items_kernel<1..16>, ks_mac_pair_kernel<1..16, nd <= 8> (where
the digit rows were stored without their transform's last layer), hoist_mac_kernel<1..16>, hoist_dot_mac_kernel<1..16, {1, 2,
4}>, hoist_giant_mac_kernel<1..16>, and four loop kernels for everything else. Every device call of this file is a `Call` in
CASES, which names its context, level and batch; tests/test_ks_instances_host.py evaluates the launchers' rules
(csrc/mac_select.hpp, and its own statement of them) over CASES and asserts, without a device, that the calls reach the whole
table. References: ref_apply_galois_inplace / ref_relinearize for the plain key switch, hoist_ref.hoisted_rotation for
apply_galois_many, hoist_dot_ref.dot_plain for apply_galois_dot_plain, hoist_bsgs_ref.bsgs for apply_galois_bsgs_plain. Keys are
random rows (the comparison needs no valid keys); no tolerance is involved anywhere.

The sections of CASES:
  sweep     N = 2^10 (four workgroups per row), 17 ciphertext primes of 60 bits and a 61-bit special prime, one 17-digit key
            per element, every level k = 1..17: nd = k, so instances 1..16 of each family and the loop kernels at 17, with the
            key's row stride at every level below its own. Plain key switch at 17 ciphertexts (item groups 8 + 8 + 1;
            ks_mac_items from 16 ciphertexts on) and at 3 on a few levels (ks_mac_kernel); apply_galois_many with two
            elements and 9 ciphertexts (groups 8 + 1); apply_galois_dot_plain over [g, 1, g'] at (n_sums, count) = (1, 5),
            (2, 3), (3, 2): S = 1 with lanes of 4 + 1 ciphertexts, S = 2 with 2 + 1, S = 4 with the fourth sum slot masked.
            BFV at nd in {1, 5, 11, 16}: the plain key switch in both modes (STRICT reads the in-bundle rows from the
            transformed copy, not from the target), the hoisted operations in STRICT. The BFV contexts take 59-bit ciphertext
            primes: the BEHZ auxiliary base is the 60-bit primes of the ring, so a BFV level over those has no RNS tool
            (`invalid rns bases`, in the reference as here).
  digits    my_digit = r / nsp with more than one special prime: 12 + 3 primes at N = 2^8, levels 1..12 (short last bundles),
            and 10 + 9 primes at levels 10, 9 and 1 (a bundle of nine takes ks_modup_kernel's recomputation path, then a
            bundle of one).
  rings     N = 2^6 and 2^7 (both hoisted operations on their loop kernels: a workgroup spans several rows), N = 2^8 (a
            workgroup is exactly one row, blocks_per_row == 1), and N = 2^8 at 17 digits (the other road to the loop kernels).
  extremes  seventeen 61-bit primes (the widest the context admits) at level 16, every key and plaintext word p - 1,
            ciphertexts all p - 1 / alternating 0 and p - 1 / random: the upper halves of the 128-bit accumulators. The
            weighted sum with 16 distinct elements (the most one launch accumulates before it reduces), with 17 (the second
            launch adds into acc and base), and with the identity as 4th and 8th term (hoist_dot_base_kernel folds its
            accumulator right after an identity term).
  group16   launch_hoist_mac's item group of 16: N = 2^10, 16 + 1 primes, level 16, 16 elements, 49 ciphertexts (4 groups x 17
            rows x 16 elements x 4 blocks = 4352 workgroups >= 4096; 32 and 64 stay below). Groups of 32 and 64 need
            gigabytes of digits at any ring a test can afford and are not covered: the group is a run-time loop bound of the
            same instance.

The giant-step kernels (op "bsgs", apply_galois_bsgs_plain) on the contexts above: the sweep at every level with five
ciphertexts (a lane's four slots and a group of one), babies [g, 1] and giants [g', conjugation, 1] -- the acc_j path, a
non-identity giant and the identity giant in one launch -- and babies [1, 1] (no acc_j: d_j = base_j[1]) on a few levels; BFV in
STRICT; both digit-mapping contexts; the rings (the loop kernel at 2^6 and 2^7 and at 17 digits, one workgroup per row at 2^8);
the extremes with every key, plaintext and ciphertext word p - 1 on 61-bit primes: sixteen distinct giants (one full launch),
seventeen (the second launch adds into ACC and BASE), the identity as 4th and 8th giant, babies all 1. The number of
hoist_giant_mac launches of every call is the host rule's.

The pair form (ks_mac_pair_kernel; the digit transforms run ntt_fwd_half_kernel's SPLIT instances) is taken by the plain key
switch with one special prime in PARITY mode at N >= 2^14, from 16 ciphertexts on, where every live prime of every digit launch
lies in bounds::fwd_split_admits (58 bits) and not all of them are below 2^50 (the FP64 schedule has no split form). More than
one special prime and STRICT never take it. tests/test_ks_instances_host.py states that rule (pair_admitted); every "switch"
call asserts that sealhip_debug_ks_split_last says what the rule predicts and that the batch was one arena chunk.
  pair sweep    CKKS, N = 2^14, sixteen 55-bit primes and a 56-bit special prime, every level k = 1..16 (nd = k: all sixteen
                instances, PF false from nd = 9, the 16-digit key's row stride at every level below its own). 19 ciphertexts:
                item groups 8 + 8 + 3, the prefetch loop's two-per-trip form ending on an odd group longer than one; 17 on
                levels 1, 8, 9, 16 (a last group of one); 16 on level 9. apply_galois on every level, relinearize on 1, 8, 9, 16.
  pair BFV      the same chain with t = 65537 (PARITY), levels 1, 8, 9, 16, 17 ciphertexts.
  pair extremes seventeen 58-bit primes (the widest the form admits), level 16, every key word p - 1, the extremes'
                ciphertext pattern, 17 and 16 ciphertexts.
  pair rings    N = 2^15 and 2^16, 17 ciphertexts, first level and level 1: 55 + 55 + 55 | 56 bits (no load treatment),
                40 + 55 | 58 (Barrett on load; at 2^16 the 58-bit prime is outside fwd_lazy_admits: the exact schedule), and at
                2^16 58 + 58 | 58 (the conditional subtraction survives: the CondSub instance).
  pair group16  N = 2^14, three 55-bit primes and a special prime, level 3, 241 ciphertexts: ceil(241 / 16) x 4 rows x 64
                blocks = 4096 workgroups, so the item group is 16 -- fifteen full groups and one of one. A group of 16 at
                nd >= 9 needs more than 1 GB of digits and is not covered: the group is a run-time bound of the same instance,
                as are 32 and 64.

Compared: the first and last ciphertext of every item group of eight, every ciphertext where there are at most five."""
import collections
import ctypes as C

import numpy as np
import pytest

import hoist_bsgs_ref as HB
import hoist_dot_ref as HD
import hoist_ref as H
import oracle_lib as O
from support import BaseSession, rows, top

pytestmark = pytest.mark.gpu

BFV, CKKS = 1, 2
PARITY, STRICT = 0, 1

Ctx = collections.namedtuple("Ctx", "scheme logn bits nsp mode t")
CONTEXTS = {
    "sweep": Ctx(CKKS, 10, [60] * 17 + [61], 1, PARITY, 0),
    "sweep_bfv": Ctx(BFV, 10, [59] * 17 + [61], 1, PARITY, 65537),
    "sweep_bfv_strict": Ctx(BFV, 10, [59] * 17 + [61], 1, STRICT, 65537),
    "nsp3": Ctx(CKKS, 8, [50] * 12 + [51] * 3, 3, PARITY, 0),
    "nsp9": Ctx(CKKS, 8, [50] * 10 + [51] * 9, 9, PARITY, 0),
    "ring6": Ctx(CKKS, 6, [50] * 3 + [51], 1, PARITY, 0),
    "ring7": Ctx(CKKS, 7, [50] * 3 + [51], 1, PARITY, 0),
    "ring8": Ctx(CKKS, 8, [50] * 3 + [51], 1, PARITY, 0),
    "ring8_17": Ctx(CKKS, 8, [50] * 17 + [51], 1, PARITY, 0),
    "extreme": Ctx(CKKS, 10, [61] * 17, 1, PARITY, 0),
    "group16": Ctx(CKKS, 10, [60] * 16 + [61], 1, PARITY, 0),
    "pair": Ctx(CKKS, 14, [55] * 16 + [56], 1, PARITY, 0),
    "pair_bfv": Ctx(BFV, 14, [55] * 16 + [56], 1, PARITY, 65537),
    "pair58": Ctx(CKKS, 14, [58] * 17, 1, PARITY, 0),
    "pair15_p55": Ctx(CKKS, 15, [55, 55, 55, 56], 1, PARITY, 0),
    "pair16_p55": Ctx(CKKS, 16, [55, 55, 55, 56], 1, PARITY, 0),
    "pair15_mixed": Ctx(CKKS, 15, [40, 55, 58], 1, PARITY, 0),
    "pair16_mixed": Ctx(CKKS, 16, [40, 55, 58], 1, PARITY, 0),
    "pair16_p58": Ctx(CKKS, 16, [58, 58, 58], 1, PARITY, 0),
    "pair_group16": Ctx(CKKS, 14, [55] * 3 + [56], 1, PARITY, 0),
}

# op: "switch" (apply_galois_inplace and relinearize_inplace), "many" (apply_galois_many), "dot" (apply_galois_dot_plain),
# "bsgs" (apply_galois_bsgs_plain: elts are the giants).
# elts: indices into the context's element list (elements()), -1 the identity; extreme: the inputs of the extremes section;
# items: the ciphertexts compared (None: compared_items); only: the positions of elts compared by "many" (None: all);
# babies: the baby elements of "bsgs"; relin: "switch" runs relinearize_inplace too
Call = collections.namedtuple("Call", "ctx op k count elts n_sums extreme items only babies relin",
                              defaults=((), 0, False, None, None, (), True))

PAIR, AROUND_ONE = (0, 1), (0, -1, 1)  # [g, g'] and [g, 1, g']
DOT_SLOTS = ((1, 5), (2, 3), (3, 2))  # (n_sums, count): S = 1, 2, 4
SMALL_BATCH_LEVELS = (1, 6, 11, 16)
BFV_LEVELS = (1, 5, 11, 16)
BABIES, GIANTS, NO_BABIES = (0, -1), (2, 1, -1), (-1, -1)  # [g, 1]; [g', conjugation, 1]; [1, 1]
PAIR_EDGE_LEVELS = (1, 8, 9, 16)  # the first and last instance, and both sides of the prefetch threshold


def switch_calls(ctx, levels, counts=(17,), small=()):
    return [Call(ctx, "switch", k, c) for k in levels for c in counts + ((3,) if k in small else ())]


def many_calls(ctx, levels, count):
    return [Call(ctx, "many", k, count, PAIR) for k in levels]


def dot_calls(ctx, levels, slots=DOT_SLOTS):
    return [Call(ctx, "dot", k, count, AROUND_ONE, n_sums) for k in levels for n_sums, count in slots]


def all_ops(ctx, levels, switch_counts, count):
    return switch_calls(ctx, levels, switch_counts) + many_calls(ctx, levels, count) + dot_calls(ctx, levels, ((2, count),))


def bsgs_calls(ctx, levels, count, no_babies=()):
    return [Call(ctx, "bsgs", k, count, GIANTS, babies=b) for k in levels for b in (BABIES,) + ((NO_BABIES,) if k in no_babies else ())]


def pair_sweep_calls(levels):
    """19 ciphertexts on every level (relinearize on the edge levels only); 17 on the edge levels; 16 on level 9"""
    out = []
    for k in levels:
        out.append(Call("pair", "switch", k, 19, relin=k in PAIR_EDGE_LEVELS))
        if k in PAIR_EDGE_LEVELS:
            out.append(Call("pair", "switch", k, 17))
        if k == 9:
            out.append(Call("pair", "switch", k, 16))
    return out


CASES = {}
for _name, _levels in (("1_6", range(1, 7)), ("7_12", range(7, 13)), ("13_17", range(13, 18))):
    CASES["sweep_switch_" + _name] = switch_calls("sweep", _levels, small=SMALL_BATCH_LEVELS)
    CASES["sweep_many_" + _name] = many_calls("sweep", _levels, 9)
    CASES["sweep_dot_" + _name] = dot_calls("sweep", _levels)
CASES["sweep_bfv_switch"] = switch_calls("sweep_bfv", BFV_LEVELS, small=SMALL_BATCH_LEVELS) + switch_calls(
    "sweep_bfv_strict", BFV_LEVELS, small=SMALL_BATCH_LEVELS)
CASES["sweep_bfv_strict_many"] = many_calls("sweep_bfv_strict", BFV_LEVELS, 9)
CASES["sweep_bfv_strict_dot"] = dot_calls("sweep_bfv_strict", BFV_LEVELS)
CASES["digits_nsp3"] = all_ops("nsp3", range(1, 13), (17, 2), 2)
CASES["digits_nsp9"] = all_ops("nsp9", (10, 9, 1), (17, 2), 2)
CASES["rings"] = (all_ops("ring6", (3, 1), (17, 2), 3) + all_ops("ring7", (3, 1), (17, 2), 3)
                  + all_ops("ring8", (3, 1), (17, 2), 3) + all_ops("ring8_17", (17,), (17, 2), 3)
                  # 17 distinct elements: the second launch of hoist_dot_mac_loop_kernel adds into acc
                  + [Call("ring7", "dot", 3, 2, tuple(range(17)), 2)])
CASES["extremes_switch_many"] = [Call("extreme", "switch", 16, 17, extreme=True),
                                 Call("extreme", "switch", 16, 3, extreme=True),
                                 Call("extreme", "many", 16, 9, PAIR, extreme=True)]
_SIXTEEN = tuple(range(16))
CASES["extremes_dot"] = [Call("extreme", "dot", 16, 3, _SIXTEEN, 1, extreme=True),
                         Call("extreme", "dot", 16, 3, _SIXTEEN, 2, extreme=True),
                         Call("extreme", "dot", 16, 3, _SIXTEEN + (16,), 3, extreme=True),
                         Call("extreme", "dot", 16, 3, (0, 1, 2, -1, 3, 4, 5, -1, 6, 7), 2, extreme=True)]
CASES["group16"] = [Call("group16", "many", 16, 49, _SIXTEEN, items=(0, 15, 16, 47, 48), only=(0, 7, 15))]
# ---- the giant-step kernels
for _name, _levels in (("1_6", range(1, 7)), ("7_12", range(7, 13)), ("13_17", range(13, 18))):
    CASES["sweep_bsgs_" + _name] = bsgs_calls("sweep", _levels, 5, SMALL_BATCH_LEVELS)
CASES["sweep_bfv_strict_bsgs"] = bsgs_calls("sweep_bfv_strict", BFV_LEVELS, 5)
CASES["digits_bsgs"] = bsgs_calls("nsp3", range(1, 13), 2) + bsgs_calls("nsp9", (10, 9, 1), 2)
CASES["rings_bsgs"] = (bsgs_calls("ring6", (3, 1), 3) + bsgs_calls("ring7", (3, 1), 3) + bsgs_calls("ring8", (3, 1), 3)
                       + bsgs_calls("ring8_17", (17,), 3))
CASES["extremes_bsgs"] = [Call("extreme", "bsgs", 16, 3, _SIXTEEN, extreme=True, babies=BABIES),
                          Call("extreme", "bsgs", 16, 3, _SIXTEEN + (16,), extreme=True, babies=BABIES),
                          Call("extreme", "bsgs", 16, 3, (0, 1, 2, -1, 3, 4, 5, -1, 6, 7), extreme=True, babies=BABIES),
                          Call("extreme", "bsgs", 16, 3, _SIXTEEN, extreme=True, babies=NO_BABIES)]
# ---- the pair form
for _name, _levels in (("1_6", range(1, 7)), ("7_9", range(7, 10)), ("10_13", range(10, 14)), ("14_16", range(14, 17))):
    CASES["pair_sweep_" + _name] = pair_sweep_calls(_levels)
CASES["pair_bfv"] = switch_calls("pair_bfv", PAIR_EDGE_LEVELS)
CASES["pair_extremes"] = [Call("pair58", "switch", 16, 17, extreme=True), Call("pair58", "switch", 16, 16, extreme=True)]
CASES["pair_rings_15"] = switch_calls("pair15_p55", (3, 1)) + switch_calls("pair15_mixed", (2, 1))
CASES["pair_rings_16"] = (switch_calls("pair16_p55", (3, 1)) + switch_calls("pair16_mixed", (2, 1))
                          + switch_calls("pair16_p58", (2, 1)))
CASES["pair_group16"] = [Call("pair_group16", "switch", 3, 241, items=(0, 15, 16, 239, 240))]


def elements(n):
    """the context's element list: a rotation by one step, conjugation, then distinct odd elements (17 in all)"""
    out = [H.elt_from_step(n, 1), 2 * n - 1]
    g = 3
    while len(out) < 17:
        if g not in out:
            out.append(g)
        g += 2
    return out


def compared_items(call):
    if call.items is not None:
        return tuple(call.items)
    if call.count <= 5:
        return tuple(range(call.count))
    edges = {i for i in range(call.count) if i % 8 in (0, 7)} | {call.count - 1}
    return tuple(sorted(edges))


class Session(BaseSession):
    """the contexts of both sides, one key per element and one for relinearize, built once per module"""

    def __init__(self, S, name):
        c = CONTEXTS[name]
        super().__init__(S, c.scheme, c.logn, c.bits, c.nsp, c.mode, c.t, sum(name.encode()))
        self.name = name
        self.elts = elements(self.n)
        self.keys, self.top_key = {}, None

    def key(self, which, extreme=False):
        """(host words, device handle) of element `which` (None: the relinearization key); the extremes share one key"""
        if extreme:
            if self.top_key is None:
                host = top(self.mods, self.n, (self.nd, 2))
                self.top_key = (host, self.S.KSwitchKeys(self.ctx, host))
            return self.top_key
        if which not in self.keys:
            host = rows(self.rng, self.mods, self.n, (self.nd, 2))
            self.keys[which] = (host, self.S.KSwitchKeys(self.ctx, host))
        return self.keys[which]

    def ciphertexts(self, k, count, size, extreme):
        ct = rows(self.rng, self.mods[:k], self.n, (count, size))
        if extreme:  # all p - 1, alternating 0 / p - 1, random, and so on through the batch
            hi = top(self.mods[:k], self.n, (size,))
            ct[0::3] = hi
            ct[1::3] = hi
            ct[1::3, :, :, 0::2] = 0
        return ct

    # ---- the three operations: device words against the oracle's on the compared items
    def switch(self, call):
        from test_ks_instances_host import pair_admitted  # (that file imports this one: resolved at the call)

        L, k, count, n = O.lib(), call.k, call.count, self.n
        # the pair form is taken exactly where the host file's rule says (its table counts on it), on the whole batch
        assert self.ctx.debug_ks_split_last(k, count) == pair_admitted(call.ctx, k, count), (call, "split_last")
        elt = self.elts[0]
        gkey, gdev = self.key(elt, call.extreme)
        ct = self.ciphertexts(k, count, 2, call.extreme)
        d = self.ctx.upload(ct)
        self.ctx.chunk_log()
        self.ev.apply_galois_inplace(d, k, count, elt, gdev)
        assert self.ctx.chunk_log() == [(count, count)], call
        got = d.download(ct.shape)
        for c in compared_items(call):
            want = ct[c].copy()
            assert L.ref_apply_galois_inplace(C.byref(self.ref.c), k, O.ptr(want), elt, O.ptr(gkey)) == 0
            assert np.array_equal(got[c], want), (call, "apply_galois", "item", c)
        d.free()
        if not call.relin:
            return
        rkey, rdev = self.key(None, call.extreme)
        ct = self.ciphertexts(k, count, 3, call.extreme)
        d = self.ctx.upload(ct)
        self.ctx.chunk_log()
        self.ev.relinearize_inplace(d, 3, k, count, [rdev])
        assert self.ctx.chunk_log() == [(count, count)], call
        got = d.download(ct.shape)
        keys = (C.c_void_p * 1)(rkey.ctypes.data)
        for c in compared_items(call):
            want = ct[c].copy()
            assert L.ref_relinearize(C.byref(self.ref.c), k, O.ptr(want), 3, keys) == 0
            assert np.array_equal(got[c, :2], want[:2]), (call, "relinearize", "item", c)
        d.free()

    def many(self, call):
        k, count, n = call.k, call.count, self.n
        elts = [self.elts[i] for i in call.elts]
        keys = [self.key(g, call.extreme) for g in elts]
        ct = self.ciphertexts(k, count, 2, call.extreme)
        d = self.ctx.upload(ct)
        out = self.ctx.alloc(len(elts) * count * 2 * k * n)
        self.ctx.chunk_log()
        self.ev.apply_galois_many(d, k, count, elts, [key[1] for key in keys], out)
        assert self.ctx.chunk_log() == [(count, count)], call  # (the launcher saw the whole batch: what the host test assumes)
        got = out.download((len(elts), count, 2, k, n))
        assert np.array_equal(d.download(ct.shape), ct), (call, "the input was modified")
        for i in (range(len(elts)) if call.only is None else call.only):
            kinv = H.hoisted_key(self.ref, keys[i][0], elts[i])
            for c in compared_items(call):
                want = H.hoisted_rotation(self.ref, k, ct[c], elts[i], keys[i][0], kinv)
                assert np.array_equal(got[i, c], want), (call, "element", elts[i], "item", c)
        d.free()
        out.free()

    def dot(self, call):
        k, count, n, n_sums = call.k, call.count, self.n, call.n_sums
        elts = [1 if i < 0 else self.elts[i] for i in call.elts]
        keys = [(None, None) if g == 1 else self.key(g, call.extreme) for g in elts]
        ct = self.ciphertexts(k, count, 2, call.extreme)
        lead = (n_sums, len(elts))
        plains = top(self.mods, n, lead) if call.extreme else rows(self.rng, self.mods, n, lead)
        d, dp = self.ctx.upload(ct), self.ctx.upload(plains)
        out = self.ctx.alloc(n_sums * count * 2 * k * n)
        self.ctx.chunk_log()
        self.ev.apply_galois_dot_plain(d, k, count, elts, [key[1] for key in keys], dp, n_sums, out)
        assert self.ctx.chunk_log() == [(count, count)], call
        got = out.download((n_sums, count, 2, k, n))
        assert np.array_equal(d.download(ct.shape), ct), (call, "the input was modified")
        items = compared_items(call)
        want = HD.dot_plain(self.ref, k, ct, elts, [key[0] for key in keys], plains, items)
        for s in range(n_sums):
            for c in items:
                assert np.array_equal(got[s, c], want[s, c]), (call, "sum", s, "item", c)
        for b in (d, dp, out):
            b.free()

    def bsgs(self, call):
        from test_ks_instances_host import launches

        k, count, n = call.k, call.count, self.n
        baby, giant = ([1 if i < 0 else self.elts[i] for i in axis] for axis in (call.babies, call.elts))
        bk, gk = ([(None, None) if g == 1 else self.key(g, call.extreme) for g in axis] for axis in (baby, giant))
        ct = self.ciphertexts(k, count, 2, call.extreme)
        lead = (len(giant), len(baby))
        plains = top(self.mods, n, lead) if call.extreme else rows(self.rng, self.mods, n, lead)
        d, dp = self.ctx.upload(ct), self.ctx.upload(plains)
        out = self.ctx.alloc(count * 2 * k * n)
        self.ctx.chunk_log()
        self.ctx.profile_enable(True)
        try:
            self.ev.apply_galois_bsgs_plain(d, k, count, baby, [key[1] for key in bk], giant, [key[1] for key in gk], dp, out)
            prof = self.ctx.profile_fetch()
        finally:
            self.ctx.profile_enable(False)
        # the whole batch and the whole giant list in one pass, cut into the launches the host test counts on
        assert self.ctx.chunk_log() == [(count, count)], call
        assert prof.get("hoist_giant_mac", {"launches": 0})["launches"] == len(launches(call)), (call, prof)
        got = out.download((count, 2, k, n))
        assert np.array_equal(d.download(ct.shape), ct), (call, "the input was modified")
        assert np.array_equal(dp.download(plains.shape), plains), (call, "the plaintexts were modified")
        items = compared_items(call)
        want = HB.bsgs(self.ref, k, ct, baby, [key[0] for key in bk], giant, [key[0] for key in gk], plains, items)
        for c in items:
            assert np.array_equal(got[c], want[c]), (call, "item", c)
        for b in (d, dp, out):
            b.free()


@pytest.fixture(scope="module")
def sessions():
    import sealhip

    assert sealhip.num_devices() >= 1
    made = {}

    def get(name):
        if name not in made:
            made[name] = Session(sealhip, name)
        return made[name]

    return get


@pytest.mark.parametrize("case", list(CASES))
def test_words_equal_the_oracle(sessions, case):
    for call in CASES[case]:
        se = sessions(call.ctx)
        if call.op == "switch":
            se.switch(call)
        elif call.op == "many":
            se.many(call)
        elif call.op == "dot":
            se.dot(call)
        else:
            assert call.op == "bsgs", call
            se.bsgs(call)
