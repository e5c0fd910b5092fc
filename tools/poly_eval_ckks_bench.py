#!/usr/bin/env python3
"""Polynomial evaluation on CKKS ciphertexts on one MI355X: prints one JSON line per measurement.
    python tools/poly_eval_ckks_bench.py --baseline-lib PATH [--degrees 7,15,31] [--counts 1,64] [--rounds 3] [--min-seconds 0.5]
candidate:  ONE sealhip_evaluator_evaluate_polynomial_ckks call (this tree's library), monomial basis;
baseline:   the hand composition it replaces, with the library of the PARENT commit (--baseline-lib is its libsealhip.so,
            built from a checkout of the parent next to this tree), following the same plan: every power by multiply +
            relinearize_rescale, an operand above the product's level dropped by mod_switch_to_next copies; every baby power
            dropped to the inner sums' level by mod_switch_to_next copies (once, shared by the sums); per inner sum and term a
            copy, multiply_plain with a constant plaintext and add, then add_plain for the constant and rescale_to_next per
            sum; per giant step the operands dropped by mod_switch_to_next copies, multiply + relinearize_rescale, and add.
            The ABI's multiply_plain works in place and a baby power feeds several inner sums, so each term is copied before
            it is scaled (as tools/poly_eval_bench.py does); every figure of this tool includes those copies on the
            baseline's side.
The protocol is that of tools/poly_eval_bench.py: each side runs in a process of its own per round (--rounds of them, the
sides alternated); a process warms every shape up, then times it with device events around at least --min-seconds of
back-to-back calls. The driver reports the median and the spread (max - min) over the rounds and the ratio call / composed;
every record carries the library's launch profile of one call. The bar: at degree 15 and 64 items the single call's median is
no slower than the composition's.
Shape: config 4's ring (CKKS, N = 2^15, 12 x 50-bit, k = 11), scale 2^50."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

NEW = ("sealhip_evaluator_linear_combination_levels", "sealhip_evaluator_polynomial_plan_ckks",
       "sealhip_evaluator_evaluate_polynomial_ckks")
ROLES = ("call", "composed")


def delta(e):
    b = 0
    while (1 << b) < e:
        b += 1
    return b


def shape(d, k):
    """the plan's shape for a dense polynomial in the monomial basis: m, g and the levels"""
    m = 1
    while m * m < d + 1:
        m += 1
    g = (d + m) // m
    lev = {e: k - delta(e) for e in range(1, min(m, d) + 1)}
    glev = {j: k - delta(m) - delta(j) for j in range(1, g)}
    l_in = k - delta(m - 1)
    l_out = min([l_in - 1] + list(glev.values()))
    return m, g, lev, glev, l_in, l_out


def worker(a):
    import torch

    import sealhip as S
    from bench import CFG4_PRIMES

    baseline = a.role == "composed"
    if baseline:
        S.LIB_PATH = os.path.abspath(a.baseline_lib)
        for name in NEW:  # (the parent's library does not have them)
            S.SYMBOLS.pop(name, None)
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    logn, mods = 15, CFG4_PRIMES
    n, n_key = 1 << logn, len(mods)
    k = n_key - 1
    scale = 2.0 ** 50
    rng = np.random.default_rng(21)
    stream = torch.cuda.Stream()
    dev = torch.device("cuda:0")
    ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
    ctx.set_stream(stream.cuda_stream)
    ev = S.Evaluator(ctx)
    one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
    key = S.KSwitchKeys(ctx, np.broadcast_to(one, (k, 2, n_key, n)).copy())  # (timing does not depend on the key words)
    low = int(min(mods[:k]))

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

    for count in [int(v) for v in a.counts.split(",")]:
        x = torch.randint(0, low, (count * 2 * k * n,), dtype=torch.int64, device=dev)  # canonical residues of every prime
        for d in [int(v) for v in a.degrees.split(",")]:
            m, g, lev, glev, l_in, l_out = shape(d, k)
            coeffs = [float(v) for v in rng.uniform(-1, 1, d + 1)]
            words = lambda level, size=2: count * size * level * n
            out = ctx.alloc(words(l_out - 1))
            if not baseline:

                def call():
                    ev.evaluate_polynomial_ckks(x, coeffs, k, count, scale, out, [key])
            else:
                plain = ctx.upload(np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods[:k]]))  # any k x N rows
                plains = torch.randint(0, low, (count * k * n,), dtype=torch.int64, device=dev)
                wide = ctx.alloc(words(k, 3))
                pair_a, pair_b = (ctx.alloc(words(k)), ctx.alloc(words(k))), (ctx.alloc(words(k)), ctx.alloc(words(k)))
                E = {1: x}
                E.update({e: ctx.alloc(words(lev[e])) for e in range(2, m + 1)})
                Y = {1: E[m]}
                Y.update({j: ctx.alloc(words(glev[j])) for j in range(2, g)})
                at_in = {i: ctx.alloc(words(l_in)) for i in range(1, m) if lev[i] != l_in}
                sums = [ctx.alloc(words(l_in)) for _ in range(g)]
                I = [ctx.alloc(words(l_in - 1)) for _ in range(g)]
                tmp = ctx.alloc(words(k))

                def dropped(src, level, target, pair):
                    """mod_switch_to_next copies down to `target`, alternating between the pair's buffers"""
                    cur, hop = src, 0
                    while level > target:
                        ev.mod_switch_to_next(cur, 2, level, count, pair[hop & 1])
                        cur, level, hop = pair[hop & 1], level - 1, hop + 1
                    return cur

                def product(a_, la, b_, lb, dst):
                    level = min(la, lb)
                    pa, pb = dropped(a_, la, level, pair_a), dropped(b_, lb, level, pair_b)
                    ev.multiply(pa, 2, pb, 2, level, count, wide)
                    ev.relinearize_rescale(wide, level, count, [key], dst)

                def call():
                    for e in range(2, m + 1):
                        hi, lo = (e + 1) // 2, e // 2
                        product(E[hi], lev[hi], E[lo], lev[lo], E[e])
                    for j in range(2, g):
                        hi, lo = (j + 1) // 2, j // 2
                        product(Y[hi], glev[hi], Y[lo], glev[lo], Y[j])
                    terms = {}
                    for i in range(1, m):
                        if lev[i] == l_in:
                            terms[i] = E[i]
                        else:  # (the last hop writes the copy at the inner level that every sum shares)
                            cur = dropped(E[i], lev[i], l_in + 1, pair_a)
                            ev.mod_switch_to_next(cur, 2, l_in + 1, count, at_in[i])
                            terms[i] = at_in[i]
                    for j in range(g):
                        for i in range(1, m):
                            dst = sums[j] if i == 1 else tmp
                            ctx.memcpy_d2d(dst, terms[i], words(l_in))
                            ev.multiply_plain_inplace(dst, 2, l_in, count, plain, 0)
                            if i > 1:
                                ev.add(sums[j], 2, tmp, 2, l_in, count, sums[j])
                        ev.add_plain_inplace(sums[j], 2, l_in, count, plains)
                        ev.rescale_to_next(sums[j], 2, l_in, count, I[j])
                    ctx.memcpy_d2d(out, dropped(I[0], l_in - 1, l_out - 1, pair_a), words(l_out - 1))
                    for j in range(1, g):
                        product(Y[j], glev[j], I[j], l_in - 1, tmp)
                        ev.add(out, 2, tmp, 2, l_out - 1, count, out)

            timed(call, {"what": "poly_ckks", "count": count, "degree": d, "n_baby": m, "n_giant": g, "out_level": l_out - 1})
            del call
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
