#!/usr/bin/env python3
"""The external product, CMux and the CMux tree on one MI355X: one JSON line per measurement.
    python tools/rgsw_bench.py [--shapes s28,cfg4] [--schemes ckks,bfv] [--counts 1,64] [--out FILE]
Shapes: s28 is section 28's (N = 2^13, two 50-bit primes and one 60-bit special prime), cfg4 is config 4's (N = 2^15, twelve
50-bit primes, k = 11). STRICT, a random RGSW block and random operands (timing does not depend on the words). Every figure
is the median of three synchronised calls after a warm-up call, on the host clock; the shares come from
sealhip_profile_fetch of one further call.
Each fused entry is measured against the composition from entries that exist without it, run from the same build:
  external_product   two switch_key_partial (c_0 with K_b, c_1 with K_a, the halves from rgsw_export), add_poly_coeffmod of
                     the partials, a copy of the base, switch_key_finish with two partials
  cmux               sub_poly_coeffmod of the two components, then the above with base = ct0
  select (l = 4)     the four levels' cmux compositions at count * 8, 4, 2, 1 pairs
The composition is handed its targets as separate component arrays (the partial entry reads packed polynomials): the
gathers a caller would need are NOT charged to it, and its select levels run on buffers of the right sizes rather than on
each other's results (the launches are the same). Both favour the composition."""
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


def median_ms(ctx, call):
    call()
    ctx.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


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
    ap.add_argument("--shapes", default="s28,cfg4")
    ap.add_argument("--schemes", default="ckks,bfv")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import oracle_lib as O
    import sealhip as S
    from bench_configs import P15_12

    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    sink = open(a.out, "a") if a.out else None
    shapes = {"s28": (13, O.coeff_modulus_create(1 << 13, [50, 50, 60])), "cfg4": (15, list(P15_12))}
    L_SEL = 4
    for shape in a.shapes.split(","):
        logn, mods = shapes[shape]
        n, k, nd = 1 << logn, len(mods) - 1, len(mods) - 1
        rng = np.random.default_rng(29)
        for name in a.schemes.split(","):
            scheme = S.SCHEME_CKKS if name == "ckks" else S.SCHEME_BFV
            ctx = S.Context(scheme, logn, mods, 1, 65537 if scheme == S.SCHEME_BFV else 0, mode=S.MODE_STRICT)
            ev = S.Evaluator(ctx)
            key = np.stack([rng.integers(0, q, size=(nd, 2, n), dtype=np.uint64) for q in mods], axis=2)  # [nd][2][n_key][N]
            halves = (S.KSwitchKeys(ctx, key), S.KSwitchKeys(ctx, np.roll(key, 1, axis=3)))
            g = ctx.rgsw_create(*halves)
            kb, ka = ctx.rgsw_export(g)
            bits = [g] * L_SEL
            unit = np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in mods[:k]], axis=1)  # one ciphertext
            ct_words = 2 * k * n

            def filled(cts):
                """cts ciphertexts of canonical words: one uploaded, the rest doubling copies on the device"""
                buf = ctx.alloc(cts * ct_words)
                ctx.memcpy_d2d(buf, ctx.upload(unit), ct_words)
                have = 1
                while have < cts:
                    m = min(have, cts - have)
                    ctx.memcpy_d2d(buf.ptr + have * ct_words * 8, buf, m * ct_words)
                    have += m
                return buf

            for count in (int(c) for c in a.counts.split(",")):
                leaves = count << L_SEL
                tree = filled(leaves)  # the tree's input; its front serves as ct / ct0, the next `count` as ct1 and base
                ct0, ct1 = tree, tree.ptr + count * ct_words * 8
                out, acc = ctx.alloc(count * ct_words), ctx.alloc((leaves // 2) * ct_words)
                pairs_max = leaves // 2
                ext_words = 2 * (k + 1) * n
                comp = [filled((pairs_max + 1) // 2) for _ in range(2)]  # component arrays: pairs_max polynomials of k rows each
                diff = [ctx.alloc(pairs_max * k * n) for _ in range(2)]
                part = [ctx.alloc(pairs_max * ext_words) for _ in range(2)]

                def composition(pairs, targets, base):
                    ctx.switch_key_partial(k, targets[0], pairs, kb, 0, nd, part[0])
                    ctx.switch_key_partial(k, targets[1], pairs, ka, 0, nd, part[1])
                    # (count polynomials of the level's KEY rows, k + nsp each: every word of the partials)
                    ctx.add_poly_coeffmod(part[0], part[1], pairs * 2, k, part[0], base=S.BASE_KEY)
                    ctx.memcpy_d2d(acc, base, pairs * ct_words)
                    ctx.switch_key_finish(k, acc, part[0], pairs, 2)

                def cmux_composition(pairs):
                    for c in range(2):
                        ctx.sub_poly_coeffmod(comp[c], comp[1 - c], pairs, k, diff[c])
                    composition(pairs, diff, tree)

                def select_composition():
                    for t in range(L_SEL):
                        cmux_composition(count << (L_SEL - t - 1))

                runs = (("external_product", lambda: ev.external_product(ct0, k, count, g, out, base=ct1),
                         lambda: composition(count, comp, ct1)),
                        ("cmux", lambda: ev.cmux(ct0, ct1, k, count, g, out), lambda: cmux_composition(count)),
                        ("select_l4", lambda: ev.select(tree, k, count, bits, out), select_composition))
                for what, fused, composed in runs:
                    f_ms, c_ms = median_ms(ctx, fused), median_ms(ctx, composed)
                    rec = {"what": what, "shape": shape, "scheme": name, "logn": logn, "k": k, "nd": nd, "count": count,
                           "plan": ctx.debug_ext_mac_plan(k, count), "fused_ms": round(f_ms, 3), "composition_ms": round(c_ms, 3),
                           "fused_over_composition": round(f_ms / c_ms, 4), "fused_shares": shares(ctx, fused),
                           "composition_shares": shares(ctx, composed)}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if sink:
                        sink.write(line + "\n")
                        sink.flush()
                for b in [tree, out, acc] + comp + diff + part:
                    b.free()
            ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
