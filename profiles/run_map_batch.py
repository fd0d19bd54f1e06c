"""Recipe of profiles/run_map_batch.txt: the trio step with the run map's run ends closed every four phases against the
parent commit, which closed them every phase.

    python profiles/run_map_batch.py --parent PARENT_TREE [--only kernel,headline,same,sq,pmc] [--out FILE]

PARENT_TREE: a checkout of the parent commit, built.  One process = one row, each under its own time limit; the first
failure ends the run.

  kernel    `bench.py --full --no-check --no-cpu-baseline` on both builds: ms per W sample of every span of the count
            chain from the library's HIP-event brackets (k_msp_map = the hashing launch, k_msp_part1 = the reads without
            a map)
  headline  plain `python bench.py`, parent and this build alternating, --runs of each; the verdict as in strike_wave.py
  same      `bench.py --genome 300000000 --dump-outputs DIR` on both builds, the four .npy compared byte by byte
  sq        rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS (counters only, nothing traced beside them) of one step with maps on
            the 1 Gb slice, both builds: per 64 bases of the launches of k_msp_part1<.., 4, ..>
  pmc       rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE of `bench.py --steps 1 --warmup 0 --inner`, each in a run of
            its own -> profiles/<round>_pmc_wgs.json + _pmc_summary_wgs.txt (profiles/summarize_pmc.py)
"""
import argparse
import csv
import filecmp
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = None


def say(s):
    print(s, flush=True)
    if OUT:
        OUT.write(s + "\n")
        OUT.flush()


def run(args, cwd, limit, env=None):
    p = subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, env=dict(os.environ, **(env or {})))
    if p.returncode != 0:
        say(f"FAILED rc {p.returncode}: {' '.join(args)} (in {cwd})\n" + p.stderr.decode()[-2000:])
        raise SystemExit(1)
    return p.stdout.decode()


def bench_line(tree, extra=(), limit=420):
    return json.loads(run([sys.executable, "bench.py"] + list(extra), tree, limit).strip().splitlines()[-1])


def sq_row(tree, label, work, genome):
    d = os.path.join(work, "sq_" + label)
    run(["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_INSTS_LDS", "--output-format", "csv", "-d", d, "-o", "s", "--", sys.executable,
         "bench.py", "--genome", str(genome), "--passes", "2", "--steps", "1", "--warmup", "1", "--inner"], tree, 600)
    src = glob.glob(os.path.join(d, "**", "s_counter_collection.csv"), recursive=True)[0]
    tot, launches = {"SQ_INSTS_VALU": 0.0, "SQ_INSTS_LDS": 0.0}, 0
    for r in csv.DictReader(open(src)):
        if re.search(r"k_msp_part1<(true|false), 4,|k_msp_part1ILb[01]ELi4E", r["Kernel_Name"]) and r["Counter_Name"] in tot:
            tot[r["Counter_Name"]] += float(r["Counter_Value"])
            launches += r["Counter_Name"] == "SQ_INSTS_VALU"
    rows = 3 * (genome * 30 // 300) * 2 * 150 / 64        # one map launch per block: every read of the trio once
    say(f"sq        {label:6s} k_msp_part1<.., 4, ..>: {launches} launches  INSTS_VALU {tot['SQ_INSTS_VALU']:.4g}  INSTS_LDS "
        f"{tot['SQ_INSTS_LDS']:.4g}  rows of 64 bases {rows:.4g}   VALU per row {tot['SQ_INSTS_VALU'] / rows:.2f}   LDS per row "
        f"{tot['SQ_INSTS_LDS'] / rows:.3f}")
    shutil.rmtree(d, ignore_errors=True)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="kernel,headline,same,sq,pmc")
    ap.add_argument("--pmc-round", default="r17")
    ap.add_argument("--commit", default="Run map: run ends closed every four phases, on top of b08099e")
    ap.add_argument("--genome", type=int, default=1_000_000_000)
    ap.add_argument("--out", default=None, help="also append every row to this file")
    args = ap.parse_args()
    OUT = open(args.out, "a") if args.out else None
    only = set(args.only.split(","))
    parent = os.path.abspath(args.parent) if args.parent else None
    both = ([("parent", parent)] if parent else []) + [("new", ROOT)]
    work = tempfile.mkdtemp(prefix="run_map_batch_")
    try:
        if "kernel" in only:
            for label, tree in both:
                ln = bench_line(tree, ["--full", "--no-check", "--no-cpu-baseline"])
                parts = ln["roofline"]["avg_launch_ms_by_kernel"]
                say(f"kernel    {label:6s} ms per W sample: " + "  ".join(f"{n} {v:.3f}" for n, v in parts.items())
                    + f"   chain {ln['roofline']['avg_launch_ms']:.1f}   ms_per_step (brackets on) {ln['ms_per_step']:.1f}")
        if "headline" in only:
            ms, facts = {"parent": [], "new": []}, {}
            for i in range(args.runs):
                for label, tree in both:
                    ln = bench_line(tree)
                    ms[label].append(ln["ms_per_step"])
                    c = ln["config"]
                    facts[label] = (c["mutant_kmers"], c["pulled_pairs"], c["records_per_sample"], c["hbm_peak_bytes"])
                    say(f"headline  {label:6s} run {i}: ms_per_step {ln['ms_per_step']:9.3f}   value {ln['value']:.4e} reads/s   mutant_kmers "
                        f"{c['mutant_kmers']}  pulled_pairs {c['pulled_pairs']}  hbm_peak_bytes {c['hbm_peak_bytes']}")
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            gap = mean["parent"] - mean["new"]
            below = max(ms["new"]) < min(ms["parent"])
            enough = gap >= 5 * max(spread.values())
            say(f"headline  means: parent {mean['parent']:.3f}  new {mean['new']:.3f}  gap {gap:.3f} ms ({100 * gap / mean['parent']:.2f} %)   "
                f"spreads: parent {spread['parent']:.3f}  new {spread['new']:.3f}   every new run below every parent run: {below}   "
                f"gap >= 5 x larger spread ({5 * max(spread.values()):.3f}): {enough}   -> {'MET' if below and enough else 'NOT MET'}")
            say(f"headline  results: mutant_kmers / pulled_pairs / records_per_sample equal: {facts['parent'][:3] == facts['new'][:3]}   "
                f"hbm_peak_bytes new {facts['new'][3]} vs parent {facts['parent'][3]}: "
                f"{'not above' if facts['new'][3] <= facts['parent'][3] else 'ABOVE'}")
        if "same" in only:
            dirs = {}
            for label, tree in both:
                dirs[label] = os.path.join(work, "dump_" + label)
                ln = bench_line(tree, ["--genome", "300000000", "--dump-outputs", dirs[label]])
                say(f"same      {label:6s} --genome 300000000: mutant_kmers {ln['config']['mutant_kmers']}  pulled_pairs {ln['config']['pulled_pairs']}")
            for name in ("mutant_keys", "histograms", "records_per_sample", "hit_reads"):
                a, b = (os.path.join(dirs[x], name + ".npy") for x in ("parent", "new"))
                same = filecmp.cmp(a, b, shallow=False)
                say(f"same      {name}.npy: {'byte-identical' if same else 'DIFFERENT'} ({os.path.getsize(b)} bytes)")
                if not same:
                    raise SystemExit(1)
        if "sq" in only:
            for label, tree in both:
                sq_row(tree, label, work, args.genome)
        if "pmc" in only:
            for ctr, tag in (("FETCH_SIZE", "f"), ("WRITE_SIZE", "w")):
                run(["rocprofv3", "--pmc", ctr, "--output-format", "csv", "-d", os.path.join(work, "pmc_" + tag), "-o", tag, "--",
                     sys.executable, "bench.py", "--steps", "1", "--warmup", "0", "--inner"], ROOT, 900)
                say(f"pmc       {ctr}: collected")
            f = glob.glob(os.path.join(work, "pmc_f", "**", "f_counter_collection.csv"), recursive=True)[0]
            w = glob.glob(os.path.join(work, "pmc_w", "**", "w_counter_collection.csv"), recursive=True)[0]
            js = os.path.join(ROOT, "profiles", f"{args.pmc_round}_pmc_wgs.json")
            summary = run([sys.executable, os.path.join(ROOT, "profiles", "summarize_pmc.py"), f, w, js, "3", "3100000000"], ROOT, 300,
                          env={"RFX_COMMIT": args.commit})
            open(os.path.join(ROOT, "profiles", f"{args.pmc_round}_pmc_summary_wgs.txt"), "w").write(summary)
            say("pmc       " + summary.splitlines()[0])
    finally:
        shutil.rmtree(work, ignore_errors=True)


main()
