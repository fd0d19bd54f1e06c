"""Recipe of profiles/filter_single_bam.txt: a single-end subject's hit reads pulled straight from its BAM in one pass
(RUFUS.Filter.single --bam; rfx_ingest.hpp BamSingleFilter, rfx_bam_gather_hits in rufus_amd/csrc/rfx_bam.hip, DESIGN section
4.18).

One process = one row (a JSON line on stdout), each under a time limit of its own.  The file is profiles/filter_bam.py's
sample (`python profiles/filter_bam.py sample DIR --pairs 4000000`: 8 M records of 276 bytes, s.bam, s.sam, hl) -- here
every record is a read by itself:

    python profiles/filter_single_bam.py prepare DIR              # s.xs.sam: s.sam with an aux field behind every line
    python profiles/filter_single_bam.py filter DIR --route bam   # RUFUS.Filter.single --bam CHR hl s.bam ...
    python profiles/filter_single_bam.py filter DIR --route sam   # RUFUS.Filter.single --sam CHR hl s.xs.sam ...  (a mapped file)
    python profiles/filter_single_bam.py filter DIR --route text  # cat s.xs.sam | PassThroughSamCheck.stranded.se CHR |
                                                                  #   RUFUS.Filter.single hl stdin ...       (runRufus.sh:1031-1032)
    python profiles/filter_single_bam.py filter DIR --route pair  # the PAIRED RUFUS.Filter --bam on the same file: two inflates
    python profiles/filter_single_bam.py kernel                   # k_bamh_pick + k_bamh_table beside k_bgzf_inflate, one 1 GiB arena

`prepare`: the feeders walk off a line that ends with QUAL, and `samtools view` never prints one: "\tXS:i:0" goes behind
every line.  `filter`: wall seconds of the whole process, the sha256 of STUB.Mutations.fastq and of the chromosome log (the
paired row: of its own three files), the route's trace line.  Alternate the routes that are compared.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_count as BC  # noqa: E402
import filter_bam as FBP  # noqa: E402
from tests import bam_ref as R  # noqa: E402

K, MIN_Q, THRESH = 25, 15, 1


def prepare(args):
    t0 = time.time()
    with open(f"{args.dir}/s.sam", "rb") as f, open(f"{args.dir}/s.xs.sam", "wb") as o:
        carry = b""
        while True:
            buf = f.read(256 << 20)
            if not buf:
                break
            buf = carry + buf
            cut = buf.rfind(b"\n") + 1
            o.write(buf[:cut].replace(b"\n", b"\tXS:i:0\n"))
            carry = buf[cut:]
        assert not carry
    print(json.dumps({"row": "prepare", "bytes": os.path.getsize(f"{args.dir}/s.xs.sam"), "s": round(time.time() - t0, 1)}))


def run_filter(args):
    b, stub = os.path.abspath(args.bin), args.route
    tail = f"{stub} {K} {MIN_Q} {THRESH} 16"
    cmd = {"bam": f"{b}/RUFUS.Filter.single --bam {stub}.chr hl s.bam {tail}",
           "sam": f"{b}/RUFUS.Filter.single --sam {stub}.chr hl s.xs.sam {tail}",
           "text": f"cat s.xs.sam | {b}/PassThroughSamCheck.stranded.se {stub}.chr | {b}/RUFUS.Filter.single hl stdin {tail}",
           "pair": f"{b}/RUFUS.Filter --bam {stub}.chr hl s.bam {tail}"}[args.route]
    t0 = time.time()
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=args.dir, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       timeout=args.limit, env=dict(os.environ, RFX_CLI_TRACE="1"))
    s = time.time() - t0
    sha = {}
    if p.returncode == 0:
        files = [f"{stub}.Mutations.fastq", f"{stub}.chr"] if stub != "pair" else \
                [f"{stub}.Mutations.Mate1.fastq", f"{stub}.Mutations.Mate2.fastq", f"{stub}.chr"]
        for f in files:
            sha[f.split(".", 1)[1]] = hashlib.sha256(open(f"{args.dir}/{f}", "rb").read()).hexdigest()[:16]
        sha["records_written"] = open(f"{args.dir}/{files[0]}", "rb").read().count(b"\n") // 4
    trace = [ln for ln in p.stderr.decode().splitlines() if "route:" in ln or "pass 1 done" in ln or "pass 2 done" in ln]
    print(json.dumps({"row": "filter", "route": args.route, "s": round(s, 3), "rc": p.returncode, **sha, "trace": trace[-4:],
                      "stderr": "" if p.returncode == 0 else p.stderr.decode()[-300:]}))
    sys.exit(p.returncode)


def kernel(args):
    from rufus_amd import capi
    hdr = R.header(BC.REFS)
    n_pairs = (args.bytes - len(hdr)) // BC.REC // 2
    sy = capi.Synth.sample(n_pairs * 10, 0)
    chunks = [FBP.records(f, min(200_000, n_pairs - f), 2 * n_pairs, sy, 100_000) for f in range(0, n_pairs, 200_000)]
    data = b"".join([hdr] + [c[0] for c in chunks])
    hl = b"".join(c[2] for c in chunks)
    with ProcessPoolExecutor(16) as ex:
        groups = list(ex.map(BC._compress, [(data[i:i + BC.GROUP], args.level) for i in range(0, len(data), BC.GROUP)]))
    L = capi.lib()
    pieces = [b""]
    for g in groups:
        if len(pieces[-1]) + len(g) > 8 << 20:
            pieces.append(b"")
        pieces[-1] += g
    reps = []
    with capi.Context(0) as ctx:
        mset = capi.MutantSet(ctx, capi.hashlist_keys(hl, K, single_end=True), K)
        ctx.prof(True)
        arena = capi.TextArena(ctx, len(data) + 65536)
        pin = L.rfx_host_alloc(max(map(len, pieces)))
        for _ in range(args.reps):
            ctx.prof_reset()
            for g in pieces:
                C.memmove(pin, g, len(g))
                t = L.rfx_text_append_bgzf(arena._h, C.cast(pin, C.c_char_p), len(g))
                assert t >= 0 and L.rfx_text_wait(arena._h, t) == 0, t
            n_rec, _ = arena.bam_settle(None, len(hdr), len(BC.REFS))
            blk, _ = arena.bam_parse_filter(MIN_Q)
            blob, hits, index = arena.bam_gather_hits(mset, blk, THRESH)
            d = ctx.prof_dict()
            row = {k + "_ms": round(d[k][0], 4) for k in ("k_bamh_pick", "k_bamh_table", "k_bgzf_inflate", "k_bamf_pack", "k_gather_copy")
                   if k in d}
            row.update({k + "_ms": round(v[0], 4) for k, v in d.items() if k.startswith("k_filter")})
            row.update(records=n_rec, reads=blk.n, selected=len(hits), bytes=len(blob), windows=int(hits.sum()))
            reps.append(row)
            blk.free()
            arena.reset()
        L.rfx_host_free(pin)
        arena.close()
        mset.free()
    print(json.dumps({"row": "kernel", "inflated_bytes": len(data), "hash_list_lines": hl.count(b"\n"), "reps": reps}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    p = sub.add_parser("prepare")
    p.add_argument("dir")
    f = sub.add_parser("filter")
    f.add_argument("dir")
    f.add_argument("--route", choices=("bam", "sam", "text", "pair"), required=True)
    f.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
    f.add_argument("--limit", type=int, default=300)
    k = sub.add_parser("kernel")
    k.add_argument("--bytes", type=int, default=1 << 30)
    k.add_argument("--level", type=int, default=1)
    k.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    {"prepare": prepare, "filter": run_filter, "kernel": kernel}[args.what](args)
