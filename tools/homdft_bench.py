#!/usr/bin/env python3
"""Homomorphic DFT on one MI355X: prints one JSON line per measurement.
    python tools/homdft_bench.py [--only cfg4,cfg5] [--counts 1,64] [--splits 5-5-4,4-4-3-3,7-7] [--min-seconds 0.5]
Rings: config 4 (CKKS, N = 2^15, 12 primes, one special) and config 5's ring (N = 2^16, 16 primes, run as CKKS). A split
lists layer counts for log2(N/2) = 14 layers; on config 5's ring (15 layers) the last stage takes one layer more.
Per ring and split, both directions:
  tables   sealhip_dft_tables_create (values generated on the device, encoded at the key level): wall-clock time of the call,
           which synchronises, and the bytes of the tables; next to it the host route over the entries the library had
           before: the same values made on the host (sealhip_dft_stage_values_host, the C++ closed form -- a numpy product of
           layer matrices is out of reach at these sizes, so this flatters the host route), uploaded, then sealhip_ckks_encode.
  call     sealhip_evaluator_coeffs_to_slots / _slots_to_coeffs per ciphertext at each batch size, device events around at
           least --min-seconds of back-to-back calls after two warm-up calls; every record carries the launch profile of one
           call. Keys are random words (timing does not depend on them).
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
    ap.add_argument("--only", default="cfg4,cfg5")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--splits", default="5-5-4,4-4-3-3,7-7")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    import torch

    import sealhip as S
    from bench import CFG4_PRIMES, CFG5_PRIMES

    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    cfgs = {"cfg4": (15, CFG4_PRIMES), "cfg5": (16, CFG5_PRIMES)}
    counts = [int(v) for v in a.counts.split(",")]
    rng = np.random.default_rng(14)
    stream = torch.cuda.Stream()
    for name in a.only.split(","):
        logn, mods = cfgs[name]
        n, n_key = 1 << logn, len(mods)
        k = nd = n_key - 1
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
        ctx.set_stream(stream.cuda_stream)
        ev = S.Evaluator(ctx)
        one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
        keys = {}

        def keys_for(steps, conj):
            nonlocal one
            elts = [ctx.galois_elt_from_step(s) for s in steps] + ([2 * n - 1] if conj else [])
            for g in elts:
                if g not in keys:  # (one random slice, rolled: timing does not depend on the key words)
                    one = np.roll(one, 1, axis=1)
                    keys[g] = S.KSwitchKeys(ctx, np.broadcast_to(one, (nd, 2, n_key, n)).copy())
            return {g: keys[g] for g in elts}

        for split in a.splits.split(","):
            stages = [int(v) for v in split.split("-")]
            stages[-1] += (logn - 1) - sum(stages)
            for direction, label in ((S.DFT_COEFFS_TO_SLOTS, "coeffs_to_slots"), (S.DFT_SLOTS_TO_COEFFS, "slots_to_coeffs")):
                plan = ev.dft_plan(direction, k, stages)
                tables = S.DftTables(ctx, direction, k, stages)  # (warm-up: the encoder's tables, the pool)
                tables.free()
                ctx.synchronize()
                t0 = time.perf_counter()
                tables = S.DftTables(ctx, direction, k, stages)
                t_dev = time.perf_counter() - t0
                # the host route: values on the host, uploaded, encoded by the entry that was there before
                t0 = time.perf_counter()
                bufs = []
                for t, st in enumerate(plan["stages"]):
                    vals = ev.dft_stage_values(direction, k, stages, t, host=True)
                    cells = st["n_giant"] * st["n_baby"]
                    dv = ctx.upload(vals.view(np.uint64))
                    plain = ctx.alloc(cells * n_key * n)
                    S._check(S.lib().sealhip_ckks_encode(ctx.handle, n_key, dv.ptr, n // 2, cells, st["scale"], plain.ptr))
                    bufs.append(plain)
                    dv.free()
                ctx.synchronize()
                t_host = time.perf_counter() - t0
                for b in bufs:
                    b.free()
                print(json.dumps({"config": name, "what": "tables", "direction": label, "stages": stages,
                                  "table_bytes": plan["table_words"] * 8, "plaintexts": plan["table_words"] // (n_key * n),
                                  "keys": len(plan["key_steps"]) + plan["needs_conjugation"],
                                  "create_seconds": round(t_dev, 4), "host_route_seconds": round(t_host, 4)}), flush=True)
                gk = keys_for(plan["key_steps"], direction == S.DFT_COEFFS_TO_SLOTS)
                ko = plan["out_level"]
                for count in counts:
                    src_h = np.stack([rng.integers(0, q, size=(count * 2, n), dtype=np.uint64) for q in mods[:k]], axis=1)
                    src, src2 = ctx.upload(src_h), ctx.upload(src_h[::-1].copy())
                    o1, o2 = ctx.alloc(count * 2 * ko * n), ctx.alloc(count * 2 * ko * n)
                    if direction == S.DFT_COEFFS_TO_SLOTS:

                        def call():
                            ev.coeffs_to_slots(tables, src, count, gk, o1, o2)
                    else:

                        def call():
                            ev.slots_to_coeffs(tables, src, src2, count, gk, o1)

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
                    rec = {"config": name, "what": label, "stages": stages, "count": count, "k": k, "out_level": ko,
                           "reps": reps, "ms_per_call": round(ms, 4), "ms_per_ciphertext": round(ms / count, 4)}
                    ctx.profile_enable(True)
                    call()
                    prof = ctx.profile_fetch()
                    ctx.profile_enable(False)
                    rec["kernels_ms"] = {tag: round(v["ms"], 4) for tag, v in prof.items()}
                    print(json.dumps(rec), flush=True)
                    for b in (src, src2, o1, o2):
                        b.free()
                tables.free()
        del keys, ctx
    return 0


if __name__ == "__main__":
    sys.exit(main())
