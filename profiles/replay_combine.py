"""Recipe of profiles/replay_combine.txt: k_msp_replay writing a wave's records in bin order (the default form) against the
parent commit, whose queued kernel stores every record on its own.

    python profiles/replay_combine.py --parent PARENT_TREE [--probe-lib LIB] [--only probe,static,kernel,sq,late,same,headline,pmc]
                                      [--out FILE]

PARENT_TREE: a checkout of the parent commit, built.  One process = one row, each under its own time limit; the first
failure ends the run.

  probe     (step 0 of the issue; --probe-lib: a scratch build of the PARENT's library whose msp_replay, under
            RFX_REPLAY_PROBE=1 / 2 / 3, brackets a probe launch of k_msp_replay<.., true> as the span, puts the bin cursors
            and the flag back and lets the real kernel do the work unbracketed -- 1: the record store behind a condition never
            true at run time, 2: every record stored to dummy + 64 * trip + lane of a per-wave area, 3: the kernel as it is,
            counting its records and those of a lane's third and later batch)  `bench.py --full --no-check --no-cpu-baseline`
            at 1 Gb (--passes 2) and at W, parent and probes alternating
  static    no GPU: rfx_msp.hip of both trees compiled to assembly with the Makefile's flags; per instantiation of
            k_msp_replay the registers, spills, occupancy, scratch and LDS (-Rpass-analysis=kernel-resource-usage) and the
            VALU / SALU / LDS / global lines; whether the old forms are line for line the parent's
  kernel    `bench.py --full --no-check --no-cpu-baseline` on parent, this build, parent again: ms per W sample of every
            span of the count chain from the library's HIP-event brackets; the two parent runs give the job's spread
  sq        rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS (counters only, nothing traced beside them) of one step
            with maps on the 1 Gb slice, both builds: per 64 bases and pass of the k_msp_replay launches
  late      (needs --probe-lib) the share of records cut in a lane's third or later batch, RFX_REPLAY_PROBE=3 at 1 Gb
  same      `bench.py --genome 300000000 --dump-outputs DIR` on both builds, the four .npy compared byte by byte
  headline  `python bench.py --no-cpu-baseline` (the timed part only: the CPU legs do not touch ms_per_step), parent and this
            build alternating, --runs of each; the verdict as in leaf_const_k.py
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
    """-> {template arguments: the kernel's instruction lines}"""
    asm, rem = os.path.join(work, label + ".s"), os.path.join(work, label + ".remarks")
    run(["hipcc"] + FLAGS + [os.path.join(tree, "rufus_amd", "csrc", "rfx_msp.hip"), "-o", asm], tree, 900, stderr_to=rem)
    usage, name, out = {}, None, {}
    for ln in open(rem):
        m = re.search(r"remark: +(Function Name: (\S+)|([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", ln)
        if m and m.group(2):
            name = m.group(2)
        elif m and name:
            usage.setdefault(name, {})[m.group(3).strip()] = int(m.group(4))
    for name, body in re.findall(r"^(_Z\w*12k_msp_replayI\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", open(asm).read(), re.S | re.M):
        lines = [re.sub(r"\.L\w+", "L", re.sub(r";.*", "", ln)).strip() for ln in body.splitlines()]
        lines = [re.sub(r"_Z\w*12k_msp_replayI\w+", "K", ln) for ln in lines if re.match(r"[a-z]+_", ln)]
        n = {p: sum(ln.startswith(p) for ln in lines) for p in ("v_", "s_", "ds_", "global_", "scratch_")}
        u = usage.get(name, {})
        targs = re.search(r"k_msp_replayI((?:Lb[01]E)+)EEv", name).group(1).replace("Lb1E", "true, ").replace("Lb0E", "false, ").rstrip(", ")
        out[targs] = lines
        say(f"static    {label:6s} k_msp_replay<{targs}>: VALU {n['v_']}  SALU {n['s_']}  LDS {n['ds_']}  global {n['global_']}  scratch ops "
            f"{n['scratch_']}  VGPRs {u.get('VGPRs')}  SGPRs {u.get('TotalSGPRs')}  VGPRs spilled {u.get('VGPRs Spill')}  scratch "
            f"{u.get('ScratchSize')}  waves/SIMD {u.get('Occupancy')}  LDS {u.get('LDS Size')}")
    return out


def sq_row(tree, label, work, genome):
    d = os.path.join(work, "sq_" + label)
    ctrs = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS")
    run(["rocprofv3", "--pmc", *ctrs, "--output-format", "csv", "-d", d, "-o", "s", "--", sys.executable,
         "bench.py", "--genome", str(genome), "--passes", "2", "--steps", "1", "--warmup", "1", "--inner"], tree, 600)
    src = glob.glob(os.path.join(d, "**", "s_counter_collection.csv"), recursive=True)[0]
    tot, launches = dict.fromkeys(ctrs, 0.0), 0
    for r in csv.DictReader(open(src)):
        if re.search(r"k_msp_replay<|12k_msp_replayI", r["Kernel_Name"]) and r["Counter_Name"] in tot:
            tot[r["Counter_Name"]] += float(r["Counter_Value"])
            launches += r["Counter_Name"] == "SQ_INSTS_VALU"
    rows = 2 * 3 * (genome * 30 // 300) * 2 * 150 / 64        # the timed step replays every read of the trio once per pass
    say(f"sq        {label:6s} k_msp_replay: {launches} launches  rows of 64 bases x passes {rows:.4g}   per row: "
        + "  ".join(f"{c[9:]} {tot[c] / rows:.2f}" for c in ctrs) + f"   VALU + SALU {(tot[ctrs[0]] + tot[ctrs[1]]) / rows:.2f}")
    shutil.rmtree(d, ignore_errors=True)


SPANS = ("k_msp_part1", "k_msp_map", "k_msp_replay", "k_part2", "k_part3", "k_msp_leaf")


def probe_row(tree, label, lib, probe, extra):
    env = {"RFX_LIB": lib, "RFX_REPLAY_PROBE": str(probe)} if probe else {}
    p = subprocess.run([sys.executable, "bench.py", "--full", "--no-check", "--no-cpu-baseline"] + extra, cwd=tree, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=420, env=dict(os.environ, **env))
    if p.returncode != 0:
        say(f"FAILED rc {p.returncode}: probe {label}\n" + p.stderr.decode()[-2000:])
        raise SystemExit(1)
    ln = json.loads(p.stdout.decode().strip().splitlines()[-1])
    parts = ln["roofline"]["avg_launch_ms_by_kernel"]
    late = [x for x in p.stderr.decode().splitlines() if x.startswith("replay_probe")]
    say(f"probe     {label:8s} " + "  ".join(f"{n} {parts.get(n, 0):.3f}" for n in SPANS) + (f"   {late[-1]}" if late else ""))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="static,kernel,sq,same,headline,pmc")
    ap.add_argument("--probe-lib", default=None, help="the scratch build of the parent's library with the probes (see above)")
    ap.add_argument("--pmc-round", default="r19")
    ap.add_argument("--commit", default="k_msp_replay: a wave's records written in bin order, on top of ef0c7d8")
    ap.add_argument("--genome", type=int, default=1_000_000_000)
    ap.add_argument("--out", default=None, help="also append every row to this file")
    args = ap.parse_args()
    OUT = open(args.out, "a") if args.out else None
    only = set(args.only.split(","))
    parent = os.path.abspath(args.parent) if args.parent else None
    both = ([("parent", parent)] if parent else []) + [("new", ROOT)]
    work = tempfile.mkdtemp(prefix="replay_combine_")
    try:
        if "probe" in only and args.probe_lib and parent:
            lib = os.path.abspath(args.probe_lib)
            for title, extra, seq in (("1 Gb, --passes 2: ms per sample", ["--genome", str(args.genome), "--passes", "2"], (0, 1, 2, 0, 1, 2, 0)),
                                      ("W: ms per W sample", [], (0, 1, 2, 0))):
                say("probe     " + title)
                for pr in seq:
                    probe_row(parent, ("parent", "probe_a", "probe_b")[pr], lib, pr, extra)
        if "late" in only and args.probe_lib and parent:
            probe_row(parent, "count", os.path.abspath(args.probe_lib), 3, ["--genome", str(args.genome), "--passes", "2"])
        if "static" in only:
            got = {label: static_rows(tree, label, work) for label, tree in both}
            if parent:
                for targs, lines in got["parent"].items():
                    say(f"static    k_msp_replay<{targs}> of the parent and <{targs}, false> of this build: "
                        + ("line for line the same" if got["new"].get(targs + ", false") == lines else "DIFFERENT"))
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
                    ln = bench_line(tree, ["--no-cpu-baseline"])
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
