#!/usr/bin/env python3
"""profiles/r04/summary.md from the files tools/collect_profiles.sh r04 produced (+ the round's A/B records):
tools/make_profile_summary_r04.py"""
import csv, json, os, re

tag = "r04"
root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", tag)
rd = lambda f: open(os.path.join(root, f)).read()
last = lambda f: json.loads(rd(f).strip().splitlines()[-1])


def short(name):
    m = re.search(r"(\w+_kernel(<[^(]*>)?)\(", name)
    return m.group(1) if m else re.sub(r"^void |\(.*$", "", name)[:100]


out = ["# Round 4 profile summary (1x MI355X, `tools/collect_profiles.sh r04`)", "",
       "`rocprofv3 --kernel-trace --stats -- python3 bench.py --no-cpu-baseline` (default: config 3, batch 4096, 1 warm-up + 3 timed "
       "steps + the NTT-only section):", "", "| kernel | calls | total ms | avg us | % |", "|---|---|---|---|---|"]
rows = list(csv.DictReader(open(os.path.join(root, "bench_default_kernel_stats.csv"))))
for r in rows[:14]:
    out.append("| %s | %s | %.2f | %.1f | %.2f |" % (short(r["Name"]), r["Calls"], int(r["TotalDurationNs"]) / 1e6,
                                                   float(r["AverageNs"]) / 1e3, float(r["Percentage"])))
b, d = last("bench_with_traffic.jsonl"), last("bench_default.jsonl")
rf, cb, pr = b["roofline"], d["cpu_baseline"], b["pipeline_roofline"]
tr = json.loads(rd("traffic.json"))
fw = tr["ntt_fwd_half"]
out += ["", "Bench line of the same build (`bench_with_traffic.jsonl`, traffic measured by this run's own `--measure-traffic` PMC passes):",
        "- value **%.0f ct-mul+relin/s**, %.1f ms per step of %d pairs; %d items verified word for word against the CPU oracle (0, B/2, B-1, the "
        "edges of the arena chunks %s, seeded random picks): %s; PCIe-inclusive (host-pointer entries, %d separately allocated pageable pairs): "
        "%.0f ct/s at %.1f GB/s host -> device; on pool blocks pinned in place (`sealhip_host_register`, no staging copies): %.0f ct/s at %.1f GB/s" % (
            b["value"], b["ms_per_step"], b["config"]["global_batch"], b["verified_count"], b["verified_chunk_sizes"], b["verified_vs_oracle"],
            b["pcie_inclusive"]["units"], b["pcie_inclusive"]["value"], b["pcie_inclusive"]["h2d_GBps"],
            b["pcie_inclusive"]["registered"]["value"], b["pcie_inclusive"]["registered"]["h2d_GBps"]),
        "- roofline (dominant kernel `ntt_fwd_half`): achieved %.0f GB/s of %.0f = **%.3f**; %d launches, avg %.3f ms, %.0f rows per launch; "
        "PMC traffic / algorithmic bytes = %.3f. **bound: %s** -- measured arithmetic ceiling of the butterfly sequence on this box %.2f T "
        "butterflies/s (reference's exact sequence: %.2f T) = %.3f of HBM for butterflies alone; the kernel executes %.0f wave-level VALU "
        "instructions per row (SQ_INSTS_VALU, own --pmc pass) against %.2f per butterfly in the rate kernel -> issue ceiling %.3f of HBM; "
        "the kernel runs at **%.2f of that ceiling** (`roofline.alu_ceiling_frac`); in cycles its vector ALUs are occupied %.0f %% of the time "
        "(`roofline.valu_busy_frac`: 4 x SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES, own --pmc passes) -- the difference is the clock, which the power "
        "limit holds lower in the transform than in the rate kernel (`fwd_clock_trace.txt`)" % (
            rf["achieved"], rf["peak"], rf["frac"], rf["launches"], rf["avg_launch_ms"], rf["rows_per_launch"],
            (rf["traffic"] or 0) / rf["algorithmic_bytes_per_launch"], rf["bound"], rf["valu_ceiling"]["butterflies_per_s"] / 1e12,
            rf["valu_ceiling"]["butterflies_per_s_reference_sequence"] / 1e12, rf["valu_ceiling"]["as_frac_of_hbm"],
            rf["valu_ceiling"].get("kernel_valu_wave_insts_per_row", 0), rf["valu_ceiling"].get("valu_insts_per_butterfly", 0),
            rf["valu_ceiling"].get("issue_ceiling_as_frac_of_hbm", 0), rf["alu_ceiling_frac"], 100 * rf.get("valu_busy_frac", 0)),
        "- forward NTT per row from the counters: read %.1f KB (x%.3f of 262.1), written %.1f KB (x%.4f of 262.1): no wasted traffic (reads below "
        "the algorithmic 262 KB on average: the key-switch digit launches run four readers of a source row on one XCD)" % (
            fw["read_bytes_per_row"] / 1e3, fw["read_bytes_per_row"] / 262144, fw["write_bytes_per_row"] / 1e3, fw["write_bytes_per_row"] / 262144),
        "- NTT-only section (the BASELINE `forward-NTT/s` metric, canonical `ntt_negacyclic_harvey`, %d rows per launch): %.2f M forward NTT/s = **%.3f** "
        "of the HBM roofline" % (b["ntt"]["rows"], b["ntt"]["forward_ntt_per_s"] / 1e6, b["ntt"]["hbm_roofline_frac"]),
        "- pipeline roofline (SURVEY 8d): compulsory %.1f MB per pair -> %.3f of HBM; NTT-equivalent %.1f MB (%d rows) -> %.3f; measured "
        "(PMC, all kernels of the step) %.1f MB per pair = %.1fx compulsory -> %.3f of HBM" % (
            pr["compulsory_bytes_per_unit"] / 1e6, pr["compulsory_frac_of_hbm"], pr["ntt_equivalent_bytes_per_unit"] / 1e6, pr["ntt_rows_per_unit"],
            pr["ntt_equivalent_frac_of_hbm"], (pr["measured_hbm_bytes_per_unit"] or 0) / 1e6, pr.get("measured_over_compulsory", 0),
            pr.get("measured_frac_of_hbm", 0)),
        "- top kernels against their own algorithmic bytes (HIP events): " + "; ".join(
            "%s %.2f ms/step = %.3f" % (k["kernel"], k["ms_per_step"], k["frac_of_hbm"] or 0) for k in b["kernels"]),
        "- default run (`bench_default.jsonl`, what the driver runs): %.0f ct/s, roofline %.3f, NTT section %.3f, traffic source: %s" % (
            d["value"], d["roofline"]["frac"], d["ntt"]["hbm_roofline_frac"], d["roofline"].get("traffic_source")),
        "- CPU baseline (oracle built -O3 -march=native on the box): %s; %.1f ct/s on %d threads, %.2f on one; host has %d physical cores -> "
        "linear all-core PROJECTION %.0f ct/s, GPU/CPU = %.1fx projected (an upper bound on the host: it assumes perfect scaling of a "
        "memory-heavy workload; the container may use %d CPUs), %.0fx against the measured %d threads" % (
            cb["cpu_model"], cb["value"], cb["cores"], cb["value_1thread"], cb["physical_cores"], cb["projected_all_physical_cores_linear"],
            cb["gpu_over_cpu_all_physical_cores_projected"], cb["cores"], cb["gpu_over_cpu_%dthreads_measured" % cb["cores"]], cb["cores"]),
        "- kernel time shares in the timed steps: %s" % json.dumps(d["kernel_time_shares"]), ""]
st = last("bench_strict.jsonl")
out += ["`--mode strict` (SURVEY F4 \"report both modes\"; `bench_strict.jsonl`): **%.0f ct-mul+relin/s**, %.1f ms per step, forward NTT %.3f in-step (launches whose consumer takes "
        "any representative drop Harvey's conditional subtraction where nothing can wrap; the 60-bit Bsk rows run the dense lazy forward schedule, the in-bundle rows are gathered and run the approximate quotient), NTT section %.3f, %d items verified against the oracle's STRICT restatement: %s, "
        "PCIe-inclusive %.0f ct/s" % (st["value"], st["ms_per_step"], st["roofline"]["frac"], st["ntt"]["hbm_roofline_frac"], st["verified_count"],
                                      st["verified_vs_oracle"], st["pcie_inclusive"]["value"]), ""]
out += ["Other BASELINE lines through the same `bench.py` (`--config 4`, `--config 5`; 256 items each verified against the oracle):"]
for c in (4, 5):
    j = last("bench_cfg%d.jsonl" % c)
    out.append("- config %d: **%.0f %s**, %.1f ms per step of %d, dominant `%s` at %.3f of HBM (bound: %s, %.2f of the butterfly ceiling), NTT-only section %.3f, "
               "%d items verified: %s; PCIe-inclusive %.0f /s; CPU oracle %.1f/s on %d threads (%.2f on one)" % (
                   c, j["value"], j["unit"], j["ms_per_step"], j["config"]["global_batch"], j["roofline"]["kernel"], j["roofline"]["frac"],
                   j["roofline"]["bound"], j["roofline"]["alu_ceiling_frac"], j["ntt"]["hbm_roofline_frac"], j["verified_count"],
                   j["verified_vs_oracle"], j["pcie_inclusive"]["value"], j["cpu_baseline"]["value"], j["cpu_baseline"]["cores"],
                   j["cpu_baseline"]["value_1thread"]))
f = last("bench_force_dist.jsonl")
out += ["", "Multi-rank path on the real backend with one rank (`bench_force_dist.jsonl`: `python -m torch.distributed.run --nproc-per-node 1 bench.py "
        "--gpus 1 --force-dist`): dist_initialized %s, gather backend %s, ranks_seen %d, %.1f GB moved at %.0f GB/s (device-local copy: one rank "
        "gathers to itself), %.0f ct/s, verified %s. No multi-GPU curve exists until the driver's SCALE record." % (
            f["dist_initialized"], f["gather"]["backend"], f["gather"]["ranks_seen"], f["gather"]["bytes_per_rank"] / 1e9,
            f["gather"]["GBps_into_root"], f["value"], f["verified_vs_oracle"]), ""]
out += ["PMC (`traffic.json`; separate `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` / `--pmc SQ_INSTS_VALU` passes over `bench.py --batch 256 --steps 2 --warmup 0 --ntt-polys 0 --pcie-pairs 0`; "
        "FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md), per kernel and for the whole step:", "```", rd("traffic.json").strip(), "```", ""]
out += ["Per-kernel times of one step (HIP events; `step_profile_b1024.txt`: config 3 multiply+relinearize and square+relinearize over 1024 pairs; "
        "`step_profile_side_configs.txt`: config 4 rotate and multiply+relinearize over 1024 ciphertexts, config 5 over 256, config 1 over 4096):",
        "```", "\n".join(l for l in rd("step_profile_b1024.txt").splitlines() if l.startswith("cfg")), rd("step_profile_side_configs.txt").strip(), "```",
        "Round 3, config 3, same kind of box: fwd 16.9-17.05, inv + tensor 11.8-12.05, floor 5.3-5.4, lift 3.6, mac 3.5-3.7, moddown 2.24 = 43.4-44.2 ms "
        "(round 2: 47.4-48.5). Same-box A/B of this round's transform kernels against round 3's: `step_ab_vs_r03_kernels.txt`.", ""]
out += ["Side configs (`configs_1gpu.jsonl`):", "```"]
for l in rd("configs_1gpu.jsonl").splitlines():
    if l.startswith('{"config": "cfg'):
        j = json.loads(l)
        out.append(j["config"] + ": " + ", ".join("%s %.4g" % (k, v) for k, v in j.items() if k != "config" and isinstance(v, (int, float))))
out += ["```", "", "FP64 against integer NTT instances on 50-bit primes, same box back to back (`ntt_fp64_ab.txt`; inverse at 2^16 = half + top kernels):",
        "```", rd("ntt_fp64_ab.txt").strip(), "```",
        "Standalone transforms (`ntt_only.txt`: N = 2^15 on config 3's 55-bit primes = integer instances; 2^14 / 2^16 on 50-bit primes = FP64):", "```"]
out += [l[:100] for l in rd("ntt_only.txt").splitlines() if l.startswith("logn")]
out += ["```", "", "Round-4 experiment records in this directory:",
        "- `fwd_quotient_ab.txt` (`tools/ab_r04_fwd.sh`, since removed; one box, three interleaved rounds, 57 344 rows per launch): the standalone canonical forward "
        "transform -- round 3's kernel (level-1 quotient, Barrett step in the store) 0.378-0.381, level-2 quotient on zero-high pairs 0.389-0.391, "
        "+ single-precision quotient estimate in the store **0.395** (+4.0 %).",
        "- `step_ab_vs_r03_kernels.txt` (`tools/ab_step.sh 1024 libsealhip.so libsealhip_apx1.so`): config 3 step over 1024 pairs, this round's transforms "
        "against round 3's in the same library otherwise: forward 17.41 -> 17.10 ms, inverse + tensor 12.22 -> 12.04 ms, step 44.68 -> 44.17 ms (-1.1 %).",
        "- `step_ab_dense_inverse.txt`: the dense lazy schedule (LZ = 3) on the 60-bit Bsk rows of the inverse against the build before it: inverse + tensor "
        "11.94 -> 11.61 ms per 1024 pairs (-2.8 %).",
        "- `fuzz_parity.txt`: `tools/fuzz_parity.py`, 4550 random cases (schemes, rings 2^3 .. 2^16, 25-59-bit primes, 1-3 special primes, batches up to 33, a quarter of the last 1350 in STRICT mode, the last 1150 on the wave-owned build, the last 1400 with the dense STRICT forward schedule; "
        "round 4: the four NTT entries on their documented operand ranges), all bit-exact against the oracle.",
        "- `inv_standalone_ab.txt`: standalone inverse at N = 2^15 (whole-row form): 0.319 -> 0.325 with the level-2 quotient in the lazy layers.",
        "- `bconv_mfma_ab.txt` (`tools/ubench_bconv_mfma.hip`, VERDICT r03 item 5): config 3's q -> Bsk base conversion as int8-MFMA byte-limb products, "
        "bit-exact against the shipped carry-free vector-ALU form on 134 M words: alone (memory-bound) it takes 158 % of the shipped form's time; repeated 4 x "
        "on the loaded words (arithmetic-bound, like the fused kernels) 92 %: -8 %, below the 15 % the verdict set as the bar. Closed.",
        "- `n65536_quarter_row_projection.txt` (`tools/n65536_projection.sh`, since removed; VERDICT r03 item 2): the quarter-row inverse at N = 2^16 IS the N = 2^15 "
        "half-row kernel; on the same bytes it runs at 0.51 (FP64) / 0.40 (integer) against 0.38 / 0.30 for the 1024-lane half-row kernel at 2^16: "
        "projected standalone 2^16 inverse 0.27 / 0.24 against 0.237 / 0.205. **Then built** (quarter-row kernels + one streaming radix-4 pass, "
        "the default for standalone inverses at 2^16): the file shows both forms on one box -- measured **0.27 / 0.24**, the projection to the digit. "
        "The forward transform has no such option (a quarter-row forward pays three products per kept output on load).",
        "- `kernel_regs_ntt.txt`: 110 kernels of `ntt.hip`, 0 with spills (the zero-high pairs cost two registers per phase).",
        "- `gpu_tests_final.txt`: the `-m gpu` suite on the final build (176 passed)."]
open(os.path.join(root, "summary.md"), "w").write("\n".join(out) + "\n")
print("wrote", os.path.join(root, "summary.md"))
