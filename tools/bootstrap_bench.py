#!/usr/bin/env python3
"""CKKS bootstrapping on one MI355X: prints one JSON line per measurement.
    python tools/bootstrap_bench.py [--counts 1,16] [--min-seconds 0.5] [--encapsulated]
Its own context: N = 2^16, q_0 of 54 bits, fifteen primes next to 12 q_0 (57.6 bits), two 59-bit special primes. ModRaise to
level 16, CoeffToSlot [5,5,5], EvalMod (K 12, r 3, degree 31, eight baby steps), SlotToCoeff [5,5,5]: out level 1. Keys are
random words (timing does not depend on them).
  bootstrap     sealhip_evaluator_bootstrap per ciphertext at each batch size, and each of its four parts alone through its own
                entry on operands of the same shape, with every part's share of their sum; device events around at least
                --min-seconds of back-to-back calls after two warm-up calls.
  double_angle  sealhip_evaluator_double_angle against the three entries it merges (dot_product without keys,
                linear_combination_levels, relinearize_rescale), alternating in the same process: the ratio of the medians
                with the spread of both.
  encapsulated  (--encapsulated) sealhip_evaluator_bootstrap_encapsulated against
                sealhip_evaluator_bootstrap, alternating in the same process, next to the two switch_secret calls it adds (level
                1 and level k_top) alone: the difference of the medians should be those two key switches.
There is no bar: nothing like this existed to compare against."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,16")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--encapsulated", action="store_true")
    a = ap.parse_args()
    import torch

    import oracle_lib as O
    import sealhip as S

    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    logn, n, K, r, d, nb, k_top, stages = 16, 1 << 16, 12, 3, 31, 8, 16, [5, 5, 5]
    q0 = O.get_primes(n, 54, 1)[0]
    below, above = O.ntt_primes_around(12 * q0, logn)
    while len(below) + len(above) < 17:
        below += O.ntt_primes_around(below[-1] - 1, logn)[0]
        above += O.ntt_primes_around(above[-1], logn)[1]
    near = [p for pair in zip(above, below) for p in pair][:15]
    mods = [q0] + near + O.get_primes(n, 59, 2)
    n_key, nd = len(mods), 8
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 2, 0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ev = S.Evaluator(ctx)
    rng = np.random.default_rng(15)
    plan = ev.bootstrap_plan(k_top, stages, stages, K, r, d, n_baby=nb)
    em = plan["evalmod"]
    one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])

    def random_key():
        nonlocal one
        one = np.roll(one, 1, axis=1)  # (one random slice, rolled: timing does not depend on the key words)
        return S.KSwitchKeys(ctx, np.broadcast_to(one, (nd, 2, n_key, n)).copy())

    gk = {g: random_key() for g in [ctx.galois_elt_from_step(s) for s in plan["key_steps"]] + [2 * n - 1]}
    rk = [random_key()]
    tables = S.BootstrapTables(ctx, k_top, stages, stages, K, r, d, n_baby=nb)
    t1 = S.DftTables(ctx, S.DFT_COEFFS_TO_SLOTS, k_top, stages)
    t2 = S.DftTables(ctx, S.DFT_SLOTS_TO_COEFFS, em["out_level"], stages, gain=plan["s2c_gain"])

    def rows(level, items):
        return ctx.upload(np.stack([rng.integers(0, q, size=(items * 2, n), dtype=np.uint64) for q in mods[:level]], axis=1))

    def timed(call):
        call()
        call()
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        reps = max(1, int(a.min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
        e0.record(stream)
        for _ in range(reps):
            call()
        e1.record(stream)
        ctx.synchronize()
        return e0.elapsed_time(e1) / reps, reps

    l1, l2, lo = plan["c2s_out_level"], em["out_level"], plan["out_level"]
    for count in [int(v) for v in a.counts.split(",")]:
        low, top, slots, sine = rows(1, count), rows(k_top, count), rows(l1, 2 * count), rows(l2, 2 * count)
        raised, re_im, sin_out, out = (ctx.alloc(count * 2 * k_top * n), ctx.alloc(2 * count * 2 * l1 * n),
                                       ctx.alloc(2 * count * 2 * l2 * n), ctx.alloc(count * 2 * lo * n))
        half1, half2 = count * 2 * l1 * n * 8, count * 2 * l2 * n * 8
        parts = {
            "mod_raise": lambda: ev.mod_raise(low, 1, count, k_top, raised),
            "coeffs_to_slots": lambda: ev.coeffs_to_slots(t1, top, count, gk, re_im.ptr, re_im.ptr + half1),
            "eval_mod": lambda: ev.eval_mod(slots, l1, 2 * count, plan["raise_scale"], K, r, d, rk, sin_out, n_baby=nb),
            "slots_to_coeffs": lambda: ev.slots_to_coeffs(t2, sine.ptr, sine.ptr + half2, count, gk, out),
        }
        ms, reps = timed(lambda: ev.bootstrap(tables, low, 1, count, gk, rk, out))
        part_ms = {name: timed(call)[0] for name, call in parts.items()}
        total = sum(part_ms.values())
        print(json.dumps({"what": "bootstrap", "count": count, "k_top": k_top, "out_level": lo, "reps": reps,
                          "ms_per_call": round(ms, 3), "ms_per_ciphertext": round(ms / count, 3),
                          "parts_ms": {name: round(v, 3) for name, v in part_ms.items()},
                          "parts_share": {name: round(v / total, 3) for name, v in part_ms.items()}}), flush=True)
        for b in (low, top, slots, sine, raised, re_im, sin_out, out):
            b.free()

    # ---- the encapsulated bootstrap against the plain one, alternating
    for count in [int(v) for v in a.counts.split(",")] if a.encapsulated else []:
        to_sparse, to_dense = random_key(), random_key()
        low, top, out = rows(1, count), rows(k_top, count), ctx.alloc(count * 2 * lo * n)
        low_out, top_out = ctx.alloc(count * 2 * n), ctx.alloc(count * 2 * k_top * n)
        plain, enc = [], []
        for _ in range(5):
            plain.append(timed(lambda: ev.bootstrap(tables, low, 1, count, gk, rk, out))[0])
            enc.append(timed(lambda: ev.bootstrap_encapsulated(tables, low, 1, count, gk, rk, to_sparse, to_dense, out))[0])
        s1 = timed(lambda: ev.switch_secret(low, 1, count, to_sparse, low_out))[0]
        s2 = timed(lambda: ev.switch_secret(top, k_top, count, to_dense, top_out))[0]
        print(json.dumps({"what": "encapsulated", "count": count, "plain_ms": [round(v, 3) for v in plain],
                          "encapsulated_ms": [round(v, 3) for v in enc],
                          "difference_ms": round(float(np.median(enc) - np.median(plain)), 3),
                          "switch_secret_level_1_ms": round(s1, 3), "switch_secret_level_k_top_ms": round(s2, 3),
                          "ratio": round(float(np.median(enc) / np.median(plain)), 4),
                          "spread_plain": round((max(plain) - min(plain)) / float(np.median(plain)), 4),
                          "spread_encapsulated": round((max(enc) - min(enc)) / float(np.median(enc)), 4)}), flush=True)
        for b in (low, top, out, low_out, top_out):
            b.free()

    # ---- double_angle against the three entries it merges, alternating
    k, scale = em["poly_level"], em["scales"][0]
    import poly_eval_ckks_ref as PC

    w = ctx.upload(np.array([2 % p for p in mods[:k]], dtype=np.uint64))
    kc = ctx.upload(np.array(PC.residues(-float(PC.rint(scale * scale)), mods[:k]), dtype=np.uint64))
    for count in [int(v) for v in a.counts.split(",")]:
        ct, wide, comb, out = rows(k, count), ctx.alloc(count * 3 * k * n), ctx.alloc(count * 3 * k * n), ctx.alloc(count * 2 * (k - 1) * n)

        def fused():
            ev.double_angle(ct, k, count, scale, rk, out)

        def chain():
            ev.dot_product([ct], [ct], k, count, wide)
            ev.linear_combination_levels([wide], [k], [3], w, k, count, comb, size=3, n_sums=1, constant=kc)
            ev.relinearize_rescale(comb, k, count, rk, out)

        f, c = [], []
        for _ in range(5):
            f.append(timed(fused)[0])
            c.append(timed(chain)[0])
        print(json.dumps({"what": "double_angle", "count": count, "k": k, "fused_ms": [round(v, 4) for v in f],
                          "chain_ms": [round(v, 4) for v in c], "ratio_fused_over_chain": round(float(np.median(f) / np.median(c)), 4),
                          "spread_fused": round((max(f) - min(f)) / float(np.median(f)), 4),
                          "spread_chain": round((max(c) - min(c)) / float(np.median(c)), 4)}), flush=True)
        for b in (ct, wide, comb, out):
            b.free()
    for t in (tables, t1, t2):
        t.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
