"""Recipe of profiles/strike_wave.txt: the trio step with k_strike_wave (a wave per plain unit, k_strike_bins for the rest)
against the parent commit's k_strike_bins alone.

    python profiles/strike_wave.py --parent PARENT_TREE [--variant LABEL=TREE ...] [--only headline,kernel,pmc,stats,same]

PARENT_TREE: a checkout of the parent commit, built; a variant TREE: this tree built with other -DRFX_SW_SET_LOG2 / -DRFX_SW_PER.
One process = one row, each under its own time limit; the first failure ends the run.

  headline  plain `python bench.py` (--steps 3 --warmup 2), parent and this build alternating, --runs of each; then the
            verdict: every run of this build below every run of the parent, and the gap of the means at least five times the
            larger of the two run-to-run spreads
  kernel    rocprofv3 --kernel-trace of `bench.py --steps 1 --warmup 2 --inner`, the strike kernels of the last step
            (profiles/summarize_trace.py), parent, this build and every variant
  pmc       rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE of `bench.py --steps 1 --warmup 0 --inner`, each in a run of its
            own with nothing traced beside it -> profiles/r13_pmc_wgs.json + r13_pmc_summary_wgs.txt (profiles/summarize_pmc.py)
  stats     units and deferred units of every strike of one --genome 1000000000 --passes 2 step (rfx_binned_strike_stats)
  same      `bench.py --genome 300000000 --dump-outputs DIR` on both builds, the four .npy compared byte by byte
"""
import argparse
import csv
import filecmp
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, JF_SIZE, LOWER, MIN_COV, MAX_DEPTH, MIN_Q, THRESH, READ_LEN, SEED, COVERAGE = 25, 8 << 30, 2, 5, 1200, 15, 1, 150, 12345, 30


def stats_row(genome, passes):
    """(child) one trio step; every rfx_binned_strike's route."""
    sys.path.insert(0, ROOT)
    from rufus_amd import capi, wgs
    seen = []
    inner = capi.binned_strike

    def strike(ctx, *a, **kw):
        r = inner(ctx, *a, **kw)
        seen.append(capi.binned_strike_stats(ctx))
        return r
    capi.binned_strike = strike
    n_pairs = genome * COVERAGE // (2 * READ_LEN)
    sys_ = [capi.Synth.sample(genome, w, n_snv=max(20, min(1000, genome // 3_000_000)), seed=SEED, read_len=READ_LEN) for w in range(3)]
    with capi.Context(0) as ctx:
        samples = [wgs.make_sample(ctx, sy, n_pairs, 1 << 24, MIN_Q, want_good=(i == 0), compact=True) for i, sy in enumerate(sys_)]
        trio = wgs.WgsTrio(ctx, K, JF_SIZE, LOWER, MIN_COV, MAX_DEPTH, THRESH, passes=passes)
        trio.masks_are_views = True
        res = trio.run(samples)
        units, deferred = sum(s["units"] for s in seen), sum(s["deferred"] for s in seen)
        print(f"stats     genome {genome} passes {passes}: " + "  ".join(f"strike {i}: {s['units']} units, {s['deferred']} deferred"
                                                                          for i, s in enumerate(seen))
              + f"   deferred share {100.0 * deferred / max(units, 1):.4f} %   mutant_kmers {res['n_mutant']}", flush=True)
        trio.close()
        for s in samples:
            for b in s:
                b.free()


def run(args, cwd, limit, env=None, stdout=subprocess.PIPE):
    p = subprocess.run(args, cwd=cwd, stdout=stdout, stderr=subprocess.PIPE, timeout=limit, env=dict(os.environ, **(env or {})))
    if p.returncode != 0:
        sys.stdout.write(f"FAILED rc {p.returncode}: {' '.join(args)} (in {cwd})\n" + p.stderr.decode()[-2000:] + "\n")
        raise SystemExit(1)
    return p.stdout.decode() if stdout == subprocess.PIPE else ""


def bench_line(tree, extra=(), limit=420):
    return json.loads(run([sys.executable, "bench.py"] + list(extra), tree, limit).strip().splitlines()[-1])


def strike_ms(tree, label, work):
    d = os.path.join(work, "trace_" + label)
    run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, "bench.py", "--steps", "1",
         "--warmup", "2", "--inner"], tree, 420)
    src = glob.glob(os.path.join(d, "**", "t_kernel_trace.csv"), recursive=True)[0]
    dst = os.path.join(work, label + "_stats.csv")
    meta = json.loads(run([sys.executable, os.path.join(ROOT, "profiles", "summarize_trace.py"), src, dst], ROOT, 120).strip().splitlines()[-1])
    out = {}
    for r in csv.DictReader(open(dst)):
        for name in ("k_strike_wave", "k_strike_bins", "k_strike_cands"):
            if name + "<" in r["Name"] or name + "(" in r["Name"]:
                c, t = out.get(name, (0, 0.0))
                out[name] = (c + int(r["Calls"]), t + float(r["TotalDurationNs"]) / 1e6)
    shutil.rmtree(d, ignore_errors=True)
    total = sum(t for n, (c, t) in out.items() if n != "k_strike_cands")
    print(f"kernel    {label:10s} " + "  ".join(f"{n} {t:.3f} ms in {c} launches" for n, (c, t) in sorted(out.items()))
          + f"   strike per step {total:.3f} ms   all kernels of the step {meta['kernel_ms']:.1f} ms", flush=True)
    return total, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--variant", action="append", default=[], help="LABEL=TREE")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="headline,kernel,pmc,stats,same")
    ap.add_argument("--pmc-round", default="r13")
    ap.add_argument("--commit", default="Trio strike: k_strike_wave takes the plain units, on top of 4e421fc")
    ap.add_argument("--stats-row", action="store_true", help="(internal) the child of the `stats` row")
    ap.add_argument("--genome", type=int, default=1_000_000_000)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    if args.stats_row:
        return stats_row(args.genome, args.passes)
    only = set(args.only.split(","))
    parent = os.path.abspath(args.parent) if args.parent else None
    variants = [(v.split("=", 1)[0], os.path.abspath(v.split("=", 1)[1])) for v in args.variant]
    work = tempfile.mkdtemp(prefix="strike_wave_")
    try:
        if "headline" in only:
            ms = {"parent": [], "new": []}
            facts = {}
            for i in range(args.runs):
                for label, tree in (("parent", parent), ("new", ROOT)):
                    ln = bench_line(tree)
                    ms[label].append(ln["ms_per_step"])
                    c = ln["config"]
                    facts[label] = (c["mutant_kmers"], c["pulled_pairs"], c["hbm_peak_bytes"])
                    print(f"headline  {label:6s} run {i}: ms_per_step {ln['ms_per_step']:9.3f}   value {ln['value']:.4e} reads/s   mutant_kmers "
                          f"{c['mutant_kmers']}  pulled_pairs {c['pulled_pairs']}  hbm_peak_bytes {c['hbm_peak_bytes']}", flush=True)
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            gap = mean["parent"] - mean["new"]
            below = max(ms["new"]) < min(ms["parent"])
            enough = gap >= 5 * max(spread.values())
            print(f"headline  means: parent {mean['parent']:.3f}  new {mean['new']:.3f}  gap {gap:.3f} ms ({100 * gap / mean['parent']:.2f} %)   "
                  f"spreads: parent {spread['parent']:.3f}  new {spread['new']:.3f}   every new run below every parent run: {below}   "
                  f"gap >= 5 x larger spread ({5 * max(spread.values()):.3f}): {enough}   -> {'MET' if below and enough else 'NOT MET'}")
            print(f"headline  results: mutant_kmers / pulled_pairs equal: {facts['parent'][:2] == facts['new'][:2]}   hbm_peak_bytes new "
                  f"{facts['new'][2]} vs parent {facts['parent'][2]}: {'not above' if facts['new'][2] <= facts['parent'][2] else 'ABOVE'}", flush=True)
        totals = {}
        if "kernel" in only:
            for label, tree in ([("parent", parent)] if parent else []) + [("new", ROOT)] + variants:
                totals[label] = strike_ms(tree, label, work)
        if "stats" in only:
            sys.stdout.write(run([sys.executable, os.path.abspath(__file__), "--stats-row", "--genome", str(args.genome), "--passes",
                                  str(args.passes)], ROOT, 300))
            for label, tree in variants:
                out = run([sys.executable, os.path.join(tree, "profiles", "strike_wave.py"), "--stats-row", "--genome", str(args.genome),
                           "--passes", str(args.passes)], tree, 300)
                sys.stdout.write(out.replace("stats    ", f"stats {label}", 1))
            sys.stdout.flush()
        if "pmc" in only:
            for ctr, tag in (("FETCH_SIZE", "f"), ("WRITE_SIZE", "w")):
                run(["rocprofv3", "--pmc", ctr, "--output-format", "csv", "-d", os.path.join(work, "pmc_" + tag), "-o", tag, "--",
                     sys.executable, "bench.py", "--steps", "1", "--warmup", "0", "--inner"], ROOT, 900)
            f = glob.glob(os.path.join(work, "pmc_f", "**", "f_counter_collection.csv"), recursive=True)[0]
            w = glob.glob(os.path.join(work, "pmc_w", "**", "w_counter_collection.csv"), recursive=True)[0]
            js = os.path.join(ROOT, "profiles", f"{args.pmc_round}_pmc_wgs.json")
            summary = run([sys.executable, os.path.join(ROOT, "profiles", "summarize_pmc.py"), f, w, js, "3", "3100000000"], ROOT, 300,
                          env={"RFX_COMMIT": args.commit})
            open(os.path.join(ROOT, "profiles", f"{args.pmc_round}_pmc_summary_wgs.txt"), "w").write(summary)
            pmc = json.load(open(js))
            old = json.load(open(os.path.join(ROOT, "profiles", "r12_pmc_wgs.json")))
            for name in ("k_strike_wave", "k_strike_bins"):
                if name in pmc:
                    print(f"pmc       new    {name}: {pmc[name]['hbm_bytes_per_launch'] / 1e9:.2f} GB per launch, {pmc[name]['launches']} launches", flush=True)
            print(f"pmc       parent k_strike_bins: {old['k_strike_bins']['hbm_bytes_per_launch'] / 1e9:.2f} GB per launch (r12_pmc_wgs.json)")
            if "new" in totals and "parent" in totals:
                nb = sum(pmc[n]["hbm_bytes_per_launch"] * pmc[n]["launches"] for n in ("k_strike_wave", "k_strike_bins") if n in pmc)
                ob = old["k_strike_bins"]["hbm_bytes_per_launch"] * old["k_strike_bins"]["launches"]
                print(f"pmc       effective: parent {ob / totals['parent'][0] / 1e9:.2f} TB/s   new {nb / totals['new'][0] / 1e9:.2f} TB/s", flush=True)
        if "same" in only:
            dirs = {}
            for label, tree in (("parent", parent), ("new", ROOT)):
                dirs[label] = os.path.join(work, "dump_" + label)
                ln = bench_line(tree, ["--genome", "300000000", "--dump-outputs", dirs[label]])
                print(f"same      {label:6s} --genome 300000000: mutant_kmers {ln['config']['mutant_kmers']}  pulled_pairs {ln['config']['pulled_pairs']}", flush=True)
            for name in ("mutant_keys", "histograms", "records_per_sample", "hit_reads"):
                a, b = (os.path.join(dirs[x], name + ".npy") for x in ("parent", "new"))
                same = filecmp.cmp(a, b, shallow=False)
                print(f"same      {name}.npy: {'byte-identical' if same else 'DIFFERENT'} ({os.path.getsize(b)} bytes)", flush=True)
                if not same:
                    raise SystemExit(1)
    finally:
        shutil.rmtree(work, ignore_errors=True)


main()
