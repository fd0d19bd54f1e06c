"""Recipe of profiles/filter_bam_cache.txt: the subject's BAM inflated once (jellyfish count --bam --keep-packed, RUFUS.Filter
--packed; rfx_bam_cache.hpp, rfx_ingest.hpp BamCachePull).  profiles/filter_bam.py's recipe, extended.

One process = one row (a JSON line on stdout), each under a time limit of its own:

    python profiles/filter_bam.py sample DIR --pairs N               # the input of section 4.15: s.bam, s.sam, hl (tmpfs)
    python profiles/filter_bam_cache.py count DIR --keep 0 [--bin B] # jellyfish count --bam CHR s.bam
    python profiles/filter_bam_cache.py count DIR --keep 1           # ... --keep-packed DIR/kp: the cost of the option, B per record
    python profiles/filter_bam_cache.py filter DIR --route bam       # RUFUS.Filter --bam CHR hl s.bam ...
    python profiles/filter_bam_cache.py filter DIR --route packed    # RUFUS.Filter --packed DIR/kp CHR hl s.bam ...
    python profiles/filter_bam_cache.py kernels DIR                  # rfx_prof_* times of the new kernels on the sample's first arena

`count`: wall seconds of the whole process, the sha256 of the payload and of the chromosome log, the cache's bytes.
`filter`: wall seconds, the sha256 of the three outputs, the route's trace line.  `--bin`: another build's executables (the
parent's, for the count without the option).  Alternate the routes that are compared.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, MIN_Q, THRESH = 25, 15, 1
COUNT = "count --disk -m 25 -L 2 -s 8G -t 16 -C"


def count(args):
    jf, stub = f"{os.path.abspath(args.bin)}/jellyfish", f"keep{args.keep}"
    cmd = f"{jf} {COUNT} -o {stub}.Jhash --bam {stub}.chr" + (f" --keep-packed kp --keep-minq {MIN_Q}" if args.keep else "") + " s.bam"
    if args.keep and os.path.exists(f"{args.dir}/kp"):
        os.unlink(f"{args.dir}/kp")
    t0 = time.time()
    p = subprocess.run(["bash", "-c", cmd], cwd=args.dir, stderr=subprocess.PIPE, timeout=args.limit, env=dict(os.environ, RFX_CLI_TRACE="1"))
    s = time.time() - t0
    h = hashlib.sha256()
    row = {"row": "count", "keep": args.keep, "bin": args.bin, "s": round(s, 3), "rc": p.returncode}
    if p.returncode == 0:
        with open(f"{args.dir}/{stub}.Jhash", "rb") as f:
            f.read(int(f.read(9)))
            for b in iter(lambda: f.read(1 << 24), b""):
                h.update(b)
        row.update({"payload_sha256": h.hexdigest()[:16], "chr_sha256": hashlib.sha256(open(f"{args.dir}/{stub}.chr", "rb").read()).hexdigest()[:16]})
        if args.keep:
            row["cache_bytes"] = os.path.getsize(f"{args.dir}/kp")
    row["trace"] = [ln for ln in p.stderr.decode().splitlines() if "bam route" in ln or "bam cache" in ln]
    row["stderr"] = "" if p.returncode == 0 else p.stderr.decode()[-300:]
    print(json.dumps(row))
    sys.exit(p.returncode)


def run_filter(args):
    exe, stub = f"{os.path.abspath(args.bin)}/RUFUS.Filter", args.route
    tail = f"{stub} {K} {MIN_Q} {THRESH} 16"
    cmd = {"bam": f"{exe} --bam {stub}.chr hl s.bam {tail}", "packed": f"{exe} --packed kp {stub}.chr hl s.bam {tail}"}[args.route]
    t0 = time.time()
    p = subprocess.run(["bash", "-c", cmd], cwd=args.dir, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=args.limit,
                       env=dict(os.environ, RFX_CLI_TRACE="1"))
    s = time.time() - t0
    sha = {}
    if p.returncode == 0:
        for f in (f"{stub}.Mutations.Mate1.fastq", f"{stub}.Mutations.Mate2.fastq", f"{stub}.chr"):
            sha[f.split(".", 1)[1]] = hashlib.sha256(open(f"{args.dir}/{f}", "rb").read()).hexdigest()[:16]
        sha["pairs"] = open(f"{args.dir}/{stub}.Mutations.Mate1.fastq", "rb").read().count(b"\n") // 4
    trace = [ln for ln in p.stderr.decode().splitlines() if "--bam" in ln or "--packed" in ln or "route:" in ln or "usable" in ln]
    print(json.dumps({"row": "filter", "route": args.route, "s": round(s, 3), "rc": p.returncode, **sha, "trace": trace[-6:],
                      "stderr": "" if p.returncode == 0 else p.stderr.decode()[-300:]}))
    sys.exit(p.returncode)


def kernels(args):
    """The new kernels on the first 1 GiB arena of s.bam: locate of all its kept records, a fetch of every --stride'th of
    them, and the mark of all their name hashes against the hashes of every 10 000th."""
    import numpy as np
    from rufus_amd import capi, tools
    data = open(f"{args.dir}/s.bam", "rb").read()
    with capi.Context(0) as ctx:
        ctx.prof(True)
        arenas = tools._bam_arenas(ctx, data, 1 << 30)
        a, n_rec, _ = next(arenas)
        empty = capi.NameSet(ctx, np.zeros(0, np.uint64))
        _, n_kept, _ = a.bam_mark_names(empty)
        empty.free()
        hashes = a.bam_name_hashes(n_kept)
        ctx.prof_reset()
        start, nbytes = a.bam_locate(n_kept)
        sel = np.arange(0, n_kept, args.stride)
        out = a.bam_fetch(start[sel], nbytes[sel])
        ns = capi.NameSet(ctx, hashes[::10000])
        mask, marked = ns.mark(hashes)
        d = ctx.prof_dict()
        row = {k + "_ms": round(v[0], 4) for k, v in d.items()
               if k in ("k_bam_locate", "k_fetch_check", "k_fetch_table", "k_gather_copy", "k_nameset_mark", "k_bam_keep", "k_bam_kept_at")}
        row.update({"row": "kernels", "arena_bytes": a.bytes, "records": n_rec, "kept": n_kept, "fetched": len(sel), "fetched_bytes": len(out),
                    "hashes": len(hashes), "set": len(ns), "marked": marked})
        print(json.dumps(row))
        ns.free()
        arenas.close()  # (closes the arenas while the context is open)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    c = sub.add_parser("count")
    c.add_argument("dir")
    c.add_argument("--keep", type=int, choices=(0, 1), required=True)
    f = sub.add_parser("filter")
    f.add_argument("dir")
    f.add_argument("--route", choices=("bam", "packed"), required=True)
    k = sub.add_parser("kernels")
    k.add_argument("dir")
    k.add_argument("--stride", type=int, default=5000)
    for p in (c, f):
        p.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
        p.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    {"count": count, "filter": run_filter, "kernels": kernels}[args.what](args)
