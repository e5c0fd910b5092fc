#!/usr/bin/env python3
"""Blind rotation on one MI355X: one JSON line per measurement.
    python tools/blind_rotate_bench.py [--schemes ckks,bfv] [--counts 1,64] [--steps 64] [--out FILE]
Shape: section 28's (N = 2^13, two 50-bit primes and one 60-bit special prime, k = 2, two digits). STRICT, a random RGSW block
used at every step, a random shared test vector and random exponents (timing does not depend on the words). The fused
entry is measured against the composition from entries of the same build, step by step as the header defines the words:
  blind_rotate     one call: X^(e_0) tv into out, then per step one prepare launch and one external product in place
  composition      multiply_monomial(tv) and per step multiply_monomial(acc, minus_one) + external_product(target, base = acc)
                   into a second accumulator (the entry refuses out = base), the two swapped
Both are warmed up, then timed in alternation (fused, composition, fused, ...) over `--rounds` rounds of synchronised calls on
the host clock; the figure is each side's median. The shares come from sealhip_profile_fetch of one further call each."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np


def timed_ms(ctx, call):
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def shares(ctx, call):
    ctx.profile_enable(True)
    call()
    ctx.synchronize()
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    total = sum(v["ms"] for v in prof.values())
    return {tag: round(v["ms"] / total, 4) for tag, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])} if total else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="ckks,bfv")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import oracle_lib as O
    import sealhip as S

    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    sink = open(a.out, "a") if a.out else None
    logn = 13
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [50, 50, 60])
    k, nd, n_steps = len(mods) - 1, len(mods) - 1, a.steps
    rng = np.random.default_rng(30)
    for name in a.schemes.split(","):
        scheme = S.SCHEME_CKKS if name == "ckks" else S.SCHEME_BFV
        ctx = S.Context(scheme, logn, mods, 1, 65537 if scheme == S.SCHEME_BFV else 0, mode=S.MODE_STRICT)
        ev = S.Evaluator(ctx)
        key = np.stack([rng.integers(0, q, size=(nd, 2, n), dtype=np.uint64) for q in mods], axis=2)  # [nd][2][n_key][N]
        g = ctx.rgsw_create(S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, np.roll(key, 1, axis=3)))
        gs = [g] * n_steps
        tv = ctx.upload(np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in mods[:k]], axis=1))
        ct_words = 2 * k * n
        for count in (int(c) for c in a.counts.split(",")):
            row = 1 + n_steps
            exps = ctx.upload_u32(rng.integers(0, 2 * n, size=(count, row)).astype(np.uint32))
            out, acc, nxt, target = (ctx.alloc(count * ct_words) for _ in range(4))

            def fused():
                ev.blind_rotate(tv, k, count, exps, gs, out)

            def composed():
                a0, a1 = acc, nxt
                ev.multiply_monomial(tv, k, count, exps, a0, n_ct=1, exps_stride=row)
                for t in range(1, row):
                    ev.multiply_monomial(a0, k, count, exps.ptr + 4 * t, target, exps_stride=row, minus_one=True)
                    ev.external_product(target, k, count, g, a1, base=a0)
                    a0, a1 = a1, a0

            for call in (fused, composed):
                call()
                ctx.synchronize()
            same = np.array_equal(out.download(), (acc if n_steps % 2 == 0 else nxt).download())
            f_ms, c_ms = [], []
            for _ in range(a.rounds):
                f_ms.append(timed_ms(ctx, fused))
                c_ms.append(timed_ms(ctx, composed))
            f, c = statistics.median(f_ms), statistics.median(c_ms)
            # what a step must move around its key switch: acc read, target written; acc read and written by the mod-down
            step_bytes = 4 * count * ct_words * 8 // 2
            rec = {"what": "blind_rotate", "scheme": name, "logn": logn, "k": k, "nd": nd, "count": count, "steps": n_steps,
                   "same_words": bool(same), "plan": ctx.debug_ext_mac_plan(k, count), "fused_ms": round(f, 3),
                   "composition_ms": round(c, 3), "fused_over_composition": round(f / c, 4),
                   "fused_ms_min_max": [round(min(f_ms), 3), round(max(f_ms), 3)],
                   "composition_ms_min_max": [round(min(c_ms), 3), round(max(c_ms), 3)],
                   "fused_us_per_step_per_item": round(f * 1e3 / (n_steps * count), 3),
                   "polynomial_bytes_per_step": step_bytes, "fused_shares": shares(ctx, fused),
                   "composition_shares": shares(ctx, composed)}
            line = json.dumps(rec)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
            for b in (out, acc, nxt, target, exps):
                b.free()
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
