#!/usr/bin/env python3
"""Polynomial evaluation on ciphertexts on one MI355X: prints one JSON line per measurement.
    python tools/poly_eval_bench.py --baseline-lib PATH [--degrees 7,15,31] [--counts 1,64] [--rounds 3] [--min-seconds 0.5]
candidate:  ONE sealhip_evaluator_evaluate_polynomial call (this tree's library);
baseline:   the composition it replaces, with the library of the PARENT commit (--baseline-lib is its libsealhip.so, built
            from a checkout of the parent next to this tree): the same power basis (multiply + relinearize per power,
            through sealhip_evaluator_multiply_many on two operands), multiply_plain with one-coefficient plaintexts + add
            for the inner sums, the scaling-variant add for their constants, multiply + relinearize + add per giant step.
            The ABI's multiply_plain works in place and a baby power is used by several inner sums, so the baseline copies
            each term before it scales it (one device-to-device copy per scalar product): the composition cannot be had
            without those copies on the parent's ABI, and every figure of this tool includes them.
Also `lincomb`: sealhip_evaluator_linear_combination alone (8 terms, 4 sums, no constant) against n_terms x (copy +
multiply_plain + add) per sum on the parent's library.
Each side runs in a process of its own per round (--rounds of them, the sides alternated); a process warms every shape up,
then times it with device events around at least --min-seconds of back-to-back calls. The driver reports the median and the
spread (max - min) over the rounds and the ratio call / composed; every record carries the library's launch profile of one
call. The bar: at degree 15 and 64 items the single call's median is no slower than the composition's.
Shape: config 3's ring in STRICT mode (BFV, N = 2^15, 8 x 55-bit, k = 7)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

NEW = ("sealhip_evaluator_linear_combination", "sealhip_evaluator_evaluate_polynomial")
ROLES = ("call", "composed")


def shape(d):
    m = 1
    while m * m < d + 1:
        m += 1
    return m, (d + m) // m


def worker(a):
    import torch

    import sealhip as S
    from bench import CFG3_PRIMES, PLAIN_T

    baseline = a.role == "composed"
    if baseline:
        S.LIB_PATH = os.path.abspath(a.baseline_lib)
        for name in NEW:  # (the parent's library does not have them)
            S.SYMBOLS.pop(name, None)
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    logn, mods, t = 15, CFG3_PRIMES, PLAIN_T
    n, n_key = 1 << logn, len(mods)
    k = n_key - 1
    rng = np.random.default_rng(20)
    stream = torch.cuda.Stream()
    dev = torch.device("cuda:0")
    L = S.lib()
    ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, t, mode=S.MODE_STRICT)
    ctx.set_stream(stream.cuda_stream)
    ev = S.Evaluator(ctx)
    one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
    key = S.KSwitchKeys(ctx, np.broadcast_to(one, (k, 2, n_key, n)).copy())  # (timing does not depend on the key words)
    keys = (C.c_void_p * 1)(key.handle)
    low = int(min(mods[:k]))
    item = 2 * k * n

    def timed(call, rec):
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
        rec.update({"role": a.role, "k": k, "reps": reps, "ms_per_call": t0.elapsed_time(t1) / reps})
        ctx.profile_enable(True)
        call()
        prof = ctx.profile_fetch()
        ctx.profile_enable(False)
        rec["kernels_ms"] = {tag: round(v["ms"], 4) for tag, v in prof.items()}
        rec["launches"] = int(sum(v["launches"] for v in prof.values()))
        print(json.dumps(rec), flush=True)

    def plain_of(c):
        p = np.zeros(n, dtype=np.uint64)
        p[0] = c
        return ctx.upload(p)

    def product(x, y, out, count):
        ptrs = (C.c_void_p * 2)(S._ptr(x), S._ptr(y))
        S._check(L.sealhip_evaluator_multiply_many(ctx.handle, k, ptrs, 2, count, keys, 1, S._ptr(out)))

    def scaled_sum(terms, plains, acc, tmp, count):
        """acc = sum_i plains[i] * terms[i]: multiply_plain works in place, so every term is copied first"""
        for i, (x, p) in enumerate(zip(terms, plains)):
            dst = acc if i == 0 else tmp
            ctx.memcpy_d2d(dst, x, count * item)
            ev.multiply_plain_inplace(dst, 2, k, count, p, 0, ntt_form=False)
            if i:
                ev.add(acc, 2, tmp, 2, k, count, acc)

    for count in [int(v) for v in a.counts.split(",")]:
        x = torch.randint(0, low, (count * item,), dtype=torch.int64, device=dev)  # canonical residues of every prime
        for d in [int(v) for v in a.degrees.split(",")]:
            m, g = shape(d)
            coeffs = [int(v) for v in rng.integers(1, t, size=d + 1)]
            out = ctx.alloc(count * item)
            if not baseline:

                def call():
                    ev.evaluate_polynomial(x, coeffs, k, count, out, [key])
            else:
                padded = coeffs + [0] * (g * m - len(coeffs))
                plains = [plain_of(c) for c in padded]
                B = [None, x] + [ctx.alloc(count * item) for _ in range(2, m + 1)]
                G = [None, B[m]] + [ctx.alloc(count * item) for _ in range(2, g)]
                I = [ctx.alloc(count * item) for _ in range(g)]
                tmp = ctx.alloc(count * item)

                def call():
                    for e in range(2, m + 1):
                        product(B[(e + 1) // 2], B[e // 2], B[e], count)
                    for j in range(2, g):
                        product(G[(j + 1) // 2], G[j // 2], G[j], count)
                    for j in range(g):
                        idx = [i for i in range(1, m) if padded[j * m + i]]
                        scaled_sum([B[i] for i in idx], [plains[j * m + i] for i in idx], I[j], tmp, count)
                        ev.add_plain_inplace(I[j], 2, k, count, plains[j * m], 0)
                    for j in range(1, g):
                        product(G[j], I[j], tmp, count)
                        ev.add(I[0] if j == 1 else out, 2, tmp, 2, k, count, out)

            timed(call, {"what": "poly", "count": count, "degree": d, "n_baby": m, "n_giant": g})
            del call
            torch.cuda.empty_cache()
        # the linear combination alone: 8 terms, 4 sums
        n_terms, n_sums = 8, 4
        terms = [torch.randint(0, low, (count * item,), dtype=torch.int64, device=dev) for _ in range(n_terms)]
        outs = ctx.alloc(n_sums * count * item)
        scalars = [[int(v) for v in rng.integers(1, t, size=n_terms)] for _ in range(n_sums)]
        if not baseline:
            half = (t + 1) // 2
            w = np.array([[[(c - (t if c >= half else 0)) % q for q in mods[:k]] for c in row] for row in scalars], dtype=np.uint64)
            dw = ctx.upload(w)

            def call():
                ev.linear_combination(terms, dw, k, count, outs, n_sums=n_sums)
        else:
            plains = [[plain_of(c) for c in row] for row in scalars]
            accs = [ctx.alloc(count * item) for _ in range(n_sums)]
            tmp = ctx.alloc(count * item)

            def call():
                for s in range(n_sums):
                    scaled_sum(terms, plains[s], accs[s], tmp, count)

        timed(call, {"what": "lincomb", "count": count, "n_terms": n_terms, "n_sums": n_sums})
        del call, terms
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--degrees", default="7,15,31")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--role", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.role:
        return worker(a)
    assert os.path.exists(a.baseline_lib), "the parent commit's libsealhip.so is needed for the baseline"
    base = [sys.executable, os.path.abspath(__file__), "--baseline-lib", a.baseline_lib, "--degrees", a.degrees, "--counts", a.counts,
            "--min-seconds", str(a.min_seconds)]
    got = {}
    for rnd in range(a.rounds):
        for role in ROLES:  # alternated: every round runs each side once, a process each
            out = subprocess.run(base + ["--role", role], capture_output=True, text=True, timeout=1500)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                return 1
            for line in out.stdout.splitlines():
                rec = json.loads(line)
                rec["round"] = rnd
                print(json.dumps(rec), flush=True)
                got.setdefault((rec["what"], rec["count"], rec.get("degree", 0), role), []).append(rec)
    for (what, count, degree, role), recs in sorted(got.items()):
        if role != "call":
            continue
        c = [r["ms_per_call"] for r in recs]
        b = [r["ms_per_call"] for r in got[(what, count, degree, "composed")]]
        print(json.dumps({"summary": what, "count": count, "degree": degree,
                          "call_ms_median": float(np.median(c)), "call_ms_spread": max(c) - min(c),
                          "composed_ms_median": float(np.median(b)), "composed_ms_spread": max(b) - min(b),
                          "call_over_composed": float(np.median(c) / np.median(b)),
                          "no_slower_than_composed": bool(np.median(c) <= np.median(b))}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
