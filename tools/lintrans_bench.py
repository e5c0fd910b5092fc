#!/usr/bin/env python3
"""Matrix-vector products from a caller's matrix on one MI355X: prints one JSON line per measurement.
    python tools/lintrans_bench.py [--shapes dense64,tridiag,stride32] [--counts 1,64] [--min-seconds 0.3]
Ring: config 4 (CKKS, N = 2^15, 12 primes, one special), n = 2^14 slots. Shapes: d = 64 dense; d = n tridiagonal (the
diagonals 0, 1 and d - 1 of a 4 GiB matrix); d = 1024 with every 32nd diagonal. Per shape:
  tables   sealhip_linear_transform_create: wall-clock time of the call, which synchronises, the bytes of the tables, and the
           launch profile (sealhip_profile_fetch) split into occupancy (the scan), gather (the values) and encode (the
           encoder's FFTs and the transforms to NTT form).
  call     sealhip_evaluator_linear_transform with the merged rescale, per ciphertext at each batch size, at the default
           baby stride and at its two neighbours (half and double, where they are strides at all): device events around at
           least --min-seconds of back-to-back calls after two warm-up calls. What the rule's weight 2 costs or saves shows
           as the neighbours' ratio to the default. Keys are random words (timing does not depend on them).
There is no bar: nothing like this existed to compare against."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dense64,tridiag,stride32")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    a = ap.parse_args()
    import torch

    import sealhip as S
    from bench import CFG4_PRIMES

    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    logn, mods = 15, CFG4_PRIMES
    n, n_key = 1 << logn, len(mods)
    slots, k = n // 2, n_key - 1
    nd = k
    counts = [int(v) for v in a.counts.split(",")]
    rng = np.random.default_rng(26)
    stream = torch.cuda.Stream()
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ctx.set_stream(stream.cuda_stream)
    ev = S.Evaluator(ctx)
    scale = float(mods[k - 1])
    one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
    keys = {}

    def keys_for(steps):
        nonlocal one
        elts = [ctx.galois_elt_from_step(s) for s in steps]
        for g in elts:
            if g not in keys:  # (one random slice, rolled: timing does not depend on the key words)
                one = np.roll(one, 1, axis=1)
                keys[g] = S.KSwitchKeys(ctx, np.broadcast_to(one, (nd, 2, n_key, n)).copy())
        return {g: keys[g] for g in elts}

    def matrix(shape):
        """(d, the matrix as a device tensor): made on the device, the 4 GiB one never exists on the host"""
        gen = torch.Generator(device="cuda").manual_seed(26)
        if shape == "dense64":
            d = 64
            return d, torch.view_as_complex(torch.randn((d, d, 2), dtype=torch.float64, device="cuda", generator=gen))
        d, diags = (slots, (0, 1, slots - 1)) if shape == "tridiag" else (1024, tuple(range(0, 1024, 32)))
        m = torch.zeros((d, d), dtype=torch.complex128, device="cuda")
        i = torch.arange(d, device="cuda")
        for c in diags:
            m[i, (i + c) % d] = torch.view_as_complex(torch.randn((d, 2), dtype=torch.float64, device="cuda", generator=gen))
        return d, m

    for shape in a.shapes.split(","):
        d, m = matrix(shape)
        torch.cuda.synchronize()
        tables = S.LinearTransform(ctx, m, d, scale)  # (warm-up: the encoder's tables, the pool)
        tables.free()
        ctx.synchronize()
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        tables = S.LinearTransform(ctx, m, d, scale)
        t_create = time.perf_counter() - t0
        prof = ctx.profile_fetch()
        ctx.profile_enable(False)
        split = {"occupancy": 0.0, "gather": 0.0, "encode": 0.0}
        for tag, v in prof.items():
            split["occupancy" if tag == "lintrans_occupancy" else "gather" if tag == "lintrans_values" else "encode"] += v["ms"]
        plan = tables.plan
        print(json.dumps({"shape": shape, "what": "tables", "d": d, "n_diagonals": plan["n_diagonals"], "n1": plan["n1"],
                          "n_baby": plan["n_baby"], "n_giant": plan["n_giant"], "keys": len(plan["key_steps"]),
                          "table_bytes": plan["table_words"] * 8, "create_seconds": round(t_create, 4),
                          "kernels_ms": {key: round(v, 4) for key, v in split.items()}}), flush=True)
        default = plan["n1"]
        for n1 in [s for s in (default // 2, default, default * 2) if 1 <= s <= d]:
            tables.free()
            tables = S.LinearTransform(ctx, m, d, scale, n1=n1)
            plan = tables.plan
            gk = keys_for(plan["key_steps"])
            nb = sum(1 for s in plan["baby_steps"] if s)
            ng = sum(1 for s in plan["giant_steps"] if s)
            for count in counts:
                src_h = np.stack([rng.integers(0, q, size=(count * 2, n), dtype=np.uint64) for q in mods[:k]], axis=1)
                src, out = ctx.upload(src_h), ctx.alloc(count * 2 * (k - 1) * n)

                def call():
                    ev.linear_transform(tables, src, k, count, gk, out, rescale=True)

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
                ms = e0.elapsed_time(e1) / reps
                print(json.dumps({"shape": shape, "what": "linear_transform", "d": d, "n1": n1, "default_n1": default,
                                  "nonzero_baby": nb, "nonzero_giant": ng, "rule_cost": nb + 2 * ng, "count": count, "k": k,
                                  "reps": reps, "ms_per_call": round(ms, 4), "ms_per_ciphertext": round(ms / count, 4)}),
                      flush=True)
                src.free()
                out.free()
        tables.free()
        del m
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
