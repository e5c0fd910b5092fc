#!/usr/bin/env python3
"""Hoisted rotation on one MI355X: prints one JSON line per measurement.
    python tools/hoist_bench.py --baseline-lib PATH [--only cfg4,cfg5] [--counts 1,64] [--elts 1,2,4,8,16]
                                [--rounds 3] [--min-seconds 0.5]
candidate: one sealhip_evaluator_apply_galois_many call for n_elts elements (this tree's library);
baseline:  n_elts calls of sealhip_evaluator_apply_galois on copies of the input (the copies are made outside the timed
           window), with the library of the PARENT commit: --baseline-lib is its libsealhip.so, built from a checkout of the
           parent next to this tree.
Each side runs in a process of its own per round (--rounds of them, candidate and baseline alternated); a process warms
every shape up, then times it with device events around at least --min-seconds of back-to-back calls. The driver reports the
median and the spread (max - min) over the rounds, the ratio hoisted / loop per rotation, and for the new inner-product
kernel the bytes its shapes imply (keys 2 nd rows N 8 per element and item group, digits nd rows N 8 per element and item,
stores 2 rows N 8 per element and item) over its time from the library's launch profiler.
Shapes: config 4 (CKKS, N = 2^15, 12 primes) and config 5's ring (N = 2^16, 16 primes, run as CKKS)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

NEW = ("sealhip_evaluator_apply_galois_many", "sealhip_evaluator_rotate_vector_many")


def mac_group(count, n_elts, nd, rows, logn):
    """ciphertexts per key load, as launch_hoist_mac (hoist.hip) picks it"""
    key_bytes = (2 * nd * rows * n_elts) << (logn + 3)
    g = 64 if key_bytes > (48 << 20) else 16
    while g > 8:
        if ((((count + g - 1) // g) * rows * n_elts) << logn) // 256 >= 4096:
            return g
        g >>= 1
    return min(count, 8)


def worker(a):
    import torch

    import sealhip as S
    from bench import CFG4_PRIMES, CFG5_PRIMES

    baseline = a.role == "loop"
    if baseline:
        S.LIB_PATH = os.path.abspath(a.baseline_lib)
        for name in NEW:  # (the parent's library does not have them)
            S.SYMBOLS.pop(name, None)
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    cfgs = {"cfg4": (15, CFG4_PRIMES), "cfg5": (16, CFG5_PRIMES)}
    counts = [int(v) for v in a.counts.split(",")]
    n_elts_list = [int(v) for v in a.elts.split(",")]
    rng = np.random.default_rng(4)
    stream = torch.cuda.Stream()
    for name in a.only.split(","):
        logn, mods = cfgs[name]
        n, n_key = 1 << logn, len(mods)
        k = n_key - 1
        nd, rows = k, n_key
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
        ctx.set_stream(stream.cuda_stream)
        ev = S.Evaluator(ctx)
        max_e = max(n_elts_list)
        elts = [ctx.galois_elt_from_step(s + 1) for s in range(max_e)]
        one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
        keys = []
        for _ in range(max_e):  # (timing does not depend on the key words: one random slice, rolled)
            one = np.roll(one, 1, axis=1)
            keys.append(S.KSwitchKeys(ctx, np.broadcast_to(one, (nd, 2, n_key, n)).copy()))
        for count in counts:
            item = 2 * k * n
            src_h = np.stack([rng.integers(0, q, size=(count * 2, n), dtype=np.uint64) for q in mods[:k]], axis=1)
            src = ctx.upload(src_h)
            for n_elts in n_elts_list:
                out = ctx.alloc(n_elts * count * item)
                if baseline:
                    for i in range(n_elts):
                        ctx.memcpy_d2d(out.ptr + i * count * item * 8, src, count * item)

                    def call():
                        for i in range(n_elts):
                            S._check(S.lib().sealhip_evaluator_apply_galois(ctx.handle, k, out.ptr + i * count * item * 8, count,
                                                                            elts[i], keys[i].handle))
                else:
                    def call():
                        ev.apply_galois_many(src, k, count, elts[:n_elts], keys[:n_elts], out)

                call()
                call()
                ctx.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                call()
                t1.record(stream)
                ctx.synchronize()
                reps = max(1, int(a.min_seconds * 1e3 / max(t0.elapsed_time(t1), 1e-3)) + 1)
                t0.record(stream)
                for _ in range(reps):
                    call()
                t1.record(stream)
                ctx.synchronize()
                ms = t0.elapsed_time(t1) / reps
                rec = {"config": name, "role": a.role, "count": count, "n_elts": n_elts, "k": k, "reps": reps,
                       "ms_per_call": ms}
                if not baseline:
                    ctx.profile_enable(True)
                    call()
                    prof = ctx.profile_fetch()
                    ctx.profile_enable(False)
                    mac = prof.get("hoist_mac")
                    if mac:
                        group = mac_group(count, n_elts, nd, rows, logn)
                        byts = 8 * n * rows * n_elts * (2 * nd * ((count + group - 1) // group) + nd * count + 2 * count)
                        rec.update({"hoist_mac_ms": mac["ms"], "hoist_mac_model_bytes": byts,
                                    "hoist_mac_gbytes_per_s": byts / (mac["ms"] * 1e-3) / 1e9})
                    rec["kernels_ms"] = {tag: round(v["ms"], 4) for tag, v in prof.items()}
                print(json.dumps(rec), flush=True)
                out.free()
            src.free()
        del keys, ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--only", default="cfg4,cfg5")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--elts", default="1,2,4,8,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--role", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.role:
        return worker(a)
    assert os.path.exists(a.baseline_lib), "the parent commit's libsealhip.so is needed for the baseline"
    base = [sys.executable, os.path.abspath(__file__), "--baseline-lib", a.baseline_lib, "--only", a.only, "--counts", a.counts,
            "--elts", a.elts, "--min-seconds", str(a.min_seconds)]
    got = {}
    for rnd in range(a.rounds):
        for role in ("hoisted", "loop"):  # alternated: every round runs each side once, a process each
            out = subprocess.run(base + ["--role", role], capture_output=True, text=True, timeout=1500)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                return 1
            for line in out.stdout.splitlines():
                rec = json.loads(line)
                rec["round"] = rnd
                print(json.dumps(rec), flush=True)
                got.setdefault((rec["config"], rec["count"], rec["n_elts"], role), []).append(rec)
    for (cfg, count, n_elts, role), recs in sorted(got.items()):
        if role != "hoisted":
            continue
        loop = got[(cfg, count, n_elts, "loop")]
        h = [r["ms_per_call"] for r in recs]
        lo = [r["ms_per_call"] for r in loop]
        summary = {"summary": cfg, "count": count, "n_elts": n_elts,
                   "hoisted_ms_median": float(np.median(h)), "hoisted_ms_spread": max(h) - min(h),
                   "loop_ms_median": float(np.median(lo)), "loop_ms_spread": max(lo) - min(lo),
                   "hoisted_over_loop": float(np.median(h) / np.median(lo)),
                   "beats_loop_by_more_than_spread": bool(np.median(lo) - np.median(h) > (max(h) - min(h)) + (max(lo) - min(lo)))}
        bw = [r["hoist_mac_gbytes_per_s"] for r in recs if "hoist_mac_gbytes_per_s" in r]
        if bw:
            summary["hoist_mac_gbytes_per_s_median"] = float(np.median(bw))
        print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
