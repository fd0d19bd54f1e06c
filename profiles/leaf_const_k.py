"""Recipe of profiles/leaf_const_k.txt: k_msp_leaf compiled for k = 25 / 31 and one segment against the parent commit, whose
one leaf kernel takes k, the segment tables and the recount knob as arguments.

    python profiles/leaf_const_k.py --parent PARENT_TREE [--only static,kernel,headline,same,sq,pmc] [--out FILE]

PARENT_TREE: a checkout of the parent commit, built.  One process = one row, each under its own time limit; the first
failure ends the run.

  static    no GPU: rfx_msp.hip of both trees compiled to assembly with the Makefile's flags; per instantiation of
            k_msp_leaf the registers, SGPR spills, occupancy, scratch and LDS (-Rpass-analysis=kernel-resource-usage) and the
            VALU / SALU / lane-move lines, in all and per section between the kernel's barriers
  kernel    `bench.py --full --no-check --no-cpu-baseline` on parent, this build, parent again: ms per W sample of every
            span of the count chain from the library's HIP-event brackets; the two parent runs give the job's spread
  headline  plain `python bench.py`, parent and this build alternating, --runs of each; the verdict as in run_map_batch.py
  same      `bench.py --genome 300000000 --dump-outputs DIR` on both builds, the four .npy compared byte by byte
  sq        rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU (counters only, nothing traced beside them) of one step on the 1 Gb
            slice with --passes 2, both builds: per 64 bases of the k_msp_leaf launches
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
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-atomic-optimizer-strategy=DPP", "--cuda-device-only",
         "-S", "-Rpass-analysis=kernel-resource-usage"]


def say(s):
    print(s, flush=True)
    if OUT:
        OUT.write(s + "\n")
        OUT.flush()


def run(args, cwd, limit, env=None, stderr_to=None):
    p = subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, env=dict(os.environ, **(env or {})))
    if p.returncode != 0:
        say(f"FAILED rc {p.returncode}: {' '.join(args)} (in {cwd})\n" + p.stderr.decode()[-2000:])
        raise SystemExit(1)
    if stderr_to:
        open(stderr_to, "wb").write(p.stderr)
    return p.stdout.decode()


def bench_line(tree, extra=(), limit=420):
    return json.loads(run([sys.executable, "bench.py"] + list(extra), tree, limit).strip().splitlines()[-1])


def static_rows(tree, label, work):
    asm, rem = os.path.join(work, label + ".s"), os.path.join(work, label + ".remarks")
    run(["hipcc"] + FLAGS + [os.path.join(tree, "rufus_amd", "csrc", "rfx_msp.hip"), "-o", asm], tree, 900, stderr_to=rem)
    usage, name = {}, None
    for ln in open(rem):
        m = re.search(r"remark: +(Function Name: (\S+)|([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", ln)
        if m and m.group(2):
            name = m.group(2)
        elif m and name:
            usage.setdefault(name, {})[m.group(3).strip()] = int(m.group(4))
    for name, body in re.findall(r"^(_Z\w*10k_msp_leafI\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", open(asm).read(), re.S | re.M):
        secs, cur = [], [0, 0, 0]
        for ln in body.splitlines():
            t = ln.split()
            if not t or not re.match(r"[vs]_", t[0]):
                continue
            if t[0] == "s_barrier":
                secs.append(cur)
                cur = [0, 0, 0]
            elif t[0].startswith("v_"):
                cur[0] += 1
                cur[2] += t[0].startswith(("v_readlane", "v_writelane"))
            else:
                cur[1] += 1
        secs.append(cur)
        u = usage.get(name, {})
        targs = re.search(r"k_msp_leafI(\w+?)EEv", name).group(1).replace("Lb1E", "true, ").replace("Lb0E", "false, ")
        targs = re.sub(r"Li(\d+)E", r"\1, ", targs).rstrip(", ")
        say(f"static    {label:6s} k_msp_leaf<{targs}>: VALU {sum(s[0] for s in secs)}  SALU {sum(s[1] for s in secs)}  lane moves "
            f"{sum(s[2] for s in secs)}  VGPRs {u.get('VGPRs')}  SGPRs {u.get('TotalSGPRs')}  SGPRs spilled {u.get('SGPRs Spill')}  scratch "
            f"{u.get('ScratchSize')}  waves/SIMD {u.get('Occupancy')}  LDS {u.get('LDS Size')}   sections v/s: "
            + "  ".join(f"{s[0]}/{s[1]}" for s in secs))


def sq_row(tree, label, work, genome):
    d = os.path.join(work, "sq_" + label)
    run(["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "--output-format", "csv", "-d", d, "-o", "s", "--", sys.executable,
         "bench.py", "--genome", str(genome), "--passes", "2", "--steps", "1", "--warmup", "0", "--inner"], tree, 600)
    src = glob.glob(os.path.join(d, "**", "s_counter_collection.csv"), recursive=True)[0]
    tot, launches = {"SQ_INSTS_VALU": 0.0, "SQ_INSTS_SALU": 0.0}, 0
    for r in csv.DictReader(open(src)):
        if re.search(r"k_msp_leaf<|10k_msp_leafI", r["Kernel_Name"]) and r["Counter_Name"] in tot:
            tot[r["Counter_Name"]] += float(r["Counter_Value"])
            launches += r["Counter_Name"] == "SQ_INSTS_VALU"
    rows = 3 * (genome * 30 // 300) * 2 * 150 / 64        # every read of the trio once: one step, no warm-up
    say(f"sq        {label:6s} k_msp_leaf: {launches} launches  INSTS_VALU {tot['SQ_INSTS_VALU']:.4g}  INSTS_SALU {tot['SQ_INSTS_SALU']:.4g}  "
        f"rows of 64 bases {rows:.4g}   VALU per row {tot['SQ_INSTS_VALU'] / rows:.2f}   SALU per row {tot['SQ_INSTS_SALU'] / rows:.2f}   "
        f"both {(tot['SQ_INSTS_VALU'] + tot['SQ_INSTS_SALU']) / rows:.2f}")
    shutil.rmtree(d, ignore_errors=True)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="static,kernel,headline,same,sq,pmc")
    ap.add_argument("--pmc-round", default="r18")
    ap.add_argument("--commit", default="k_msp_leaf compiled for k = 25 / 31 and one segment, on top of 2fd08d9")
    ap.add_argument("--genome", type=int, default=1_000_000_000)
    ap.add_argument("--out", default=None, help="also append every row to this file")
    args = ap.parse_args()
    OUT = open(args.out, "a") if args.out else None
    only = set(args.only.split(","))
    parent = os.path.abspath(args.parent) if args.parent else None
    both = ([("parent", parent)] if parent else []) + [("new", ROOT)]
    work = tempfile.mkdtemp(prefix="leaf_const_k_")
    try:
        if "static" in only:
            for label, tree in both:
                static_rows(tree, label, work)
        if "kernel" in only:
            for label, tree in both + both[:-1]:
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
