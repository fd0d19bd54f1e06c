"""Recipe of profiles/pull_reads.txt: the trio driver's step with and without the pull of the subject's read pairs.

One process = one row: the synthetic trio of bench.py's --workload wgs at --genome bases (compact blocks, generated on the
device), `--warmup` untimed steps, then `--steps` timed plain run() steps; with --pull the same number of run(pull=True)
steps after them (the pulled block is freed outside the timed region) and one profiled step of each kind for the kernel times
from rfx_prof_*.  --tree DIR imports rufus_amd from DIR (a checkout of the parent commit, built) instead of this tree.

    python profiles/pull_reads.py --label N1 --pull
    python profiles/pull_reads.py --label P1 --tree PARENT_TREE
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="run")
ap.add_argument("--genome", type=int, default=1_000_000_000)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--pull", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

from rufus_amd import capi, wgs  # noqa: E402

K, JF_SIZE, LOWER, MIN_COV, MAX_DEPTH, MIN_Q, THRESH, READ_LEN, SEED, COVERAGE = 25, 8 << 30, 2, 5, 1200, 15, 1, 150, 12345, 30


def timed(ctx, fn, n):
    out = []
    for _ in range(n):
        ctx.sync()
        t0 = time.perf_counter()
        res = fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
        if "pulled" in res:
            res["pulled"]["block"].free()
    return out, res


def main():
    G = args.genome
    n_pairs = G * COVERAGE // (2 * READ_LEN)
    sys_ = [capi.Synth.sample(G, w, n_snv=max(20, min(1000, G // 3_000_000)), seed=SEED, read_len=READ_LEN) for w in range(3)]
    with capi.Context(0) as ctx:
        samples = [wgs.make_sample(ctx, sy, n_pairs, 1 << 24, MIN_Q, want_good=(i == 0), compact=True) for i, sy in enumerate(sys_)]
        trio = wgs.WgsTrio(ctx, K, JF_SIZE, LOWER, MIN_COV, MAX_DEPTH, THRESH, passes=args.passes)
        trio.masks_are_views = True
        timed(ctx, lambda: trio.run(samples), args.warmup)
        ms, res = timed(ctx, lambda: trio.run(samples), args.steps)
        facts = f"mutant_kmers {res['n_mutant']}  pulled_pairs {res['n_pulled']}  subject blocks {len(samples[0])}"
        print(f"{args.label:10s} plain  ms/step " + " ".join(f"{x:8.2f}" for x in ms) + f"   median {sorted(ms)[len(ms) // 2]:8.2f}   {facts}", flush=True)
        if args.pull:
            timed(ctx, lambda: trio.run(samples, pull=True), 1)
            ms2, res2 = timed(ctx, lambda: trio.run(samples, pull=True), args.steps)
            assert res2["n_pulled"] == res["n_pulled"]
            print(f"{args.label:10s} pull   ms/step " + " ".join(f"{x:8.2f}" for x in ms2) + f"   median {sorted(ms2)[len(ms2) // 2]:8.2f}", flush=True)
            ctx.prof(True)
            for name, fn in (("plain", lambda: trio.run(samples)), ("pull", lambda: trio.run(samples, pull=True))):
                ctx.prof_reset()
                timed(ctx, fn, 1)
                d = ctx.prof_dict()
                keep = {n_: v for n_, v in d.items() if n_.startswith("k_select") or n_.startswith("k_filter")}
                print(f"{args.label:10s} {name:5s}  kernel ms (launches): " + "  ".join(f"{n_} {v[0]:.3f} ({v[1]})" for n_, v in sorted(keep.items()))
                      + f"   all kernels {sum(v[0] for v in d.values()):.2f}", flush=True)
            ctx.prof(False)
            r = trio.run(samples, pull=True)
            b = r["pulled"]["block"]
            print(f"{args.label:10s} pulled block: {b.n} reads, {b.bases} bases, {b.device_bytes} device bytes; "
                  f"mask words per step {sum((x.n + 63) // 64 for x in samples[0])}", flush=True)
            b.free()
        trio.close()
        for s in samples:
            for b in s:
                b.free()


main()
