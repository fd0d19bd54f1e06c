"""Recipe of profiles/bam_count.txt: BAM records found and packed on the device (rufus_amd/csrc/rfx_bam.hip, DESIGN
section 4.14).

One process = one row (a JSON line on stdout), each under a time limit of its own:

    python profiles/bam_count.py kernel                    # 1. one arena of BAM: guess / walk / repair / starts / pack
    python profiles/bam_count.py sample DIR --pairs N      #    N pairs as s.bam and, the same kept records, s.sam in DIR (tmpfs)
    python profiles/bam_count.py count DIR --route bam     # 2. jellyfish count --bam CHR s.bam
    python profiles/bam_count.py count DIR --route sam     #    jellyfish count --sam CHR s.sam
    python profiles/bam_count.py count DIR --route pipe    #    cat s.sam | jellyfish count --sam CHR /dev/stdin

`kernel`: reads from rfx_synth_text (150 bases) as BAM records of 276 bytes (a name of 10 characters, one cigar operation,
no aux; every 16th record carries flag 1024), compressed by the tests' BGZF writer (tests/bgzf_ref.py, --level, 16
processes), appended in pieces of <= 8 MiB from one page-locked buffer (a k_bgzf_inflate launch each), settled and parsed, three repetitions; the times are
the rfx_prof_* spans of the kernels, k_bgzf_inflate of the same arena beside them; rfx_bam_stats of the last repetition.
`count`: wall seconds of the whole process and the sha256 of the output's payload.  Alternate the routes that are compared.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bam_ref as R  # noqa: E402
from tests import bgzf_ref as B  # noqa: E402

GROUP = 64 * B.BLOCK_PAYLOAD
COUNT = "count --disk -m 25 -L 2 -s 8G -t 16 -C"
REFS = [(b"c%02d" % i, 250_000_000) for i in range(25)]
REC = 276  # bytes of one record


def _compress(job):
    chunk, level = job
    return b"".join(B.block(chunk[i:i + B.BLOCK_PAYLOAD], level) for i in range(0, len(chunk), B.BLOCK_PAYLOAD))


def records(first_pair, n_pairs, total_reads, sy, want_sam):
    """(BAM records, SAM lines of the kept ones) of reads 2 * first_pair .. 2 * (first_pair + n_pairs) - 1."""
    import numpy as np
    seq, qual = sy.text(first_pair, n_pairs)
    m = 2 * n_pairs
    idx = np.arange(2 * first_pair, 2 * first_pair + m)
    ref = (idx * len(REFS) // total_reads).astype(np.int32)
    flag = np.where(idx % 16 == 5, 1024, 0).astype(np.uint16)
    digits = ((idx[:, None] // 10 ** np.arange(8, -1, -1)) % 10 + 48).astype(np.uint8)
    a = np.zeros((m, REC), np.uint8)
    head = np.zeros(m, np.dtype([("bs", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                                 ("n_cigar", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")]))
    head["bs"], head["ref"], head["pos"], head["l_name"], head["mapq"], head["bin"] = REC - 4, ref, idx % 200_000_000, 11, 60, 4680
    head["n_cigar"], head["flag"], head["l_seq"], head["nref"], head["npos"] = 1, flag, 150, ref, idx % 200_000_000
    a[:, :36] = head.view(np.uint8).reshape(m, 36)
    a[:, 36], a[:, 37:46] = ord("r"), digits
    a[:, 47:51] = np.frombuffer(struct.pack("<I", 150 << 4), np.uint8)
    lut = np.full(256, 15, np.uint8)
    lut[[65, 67, 71, 84]] = [1, 2, 4, 8]
    nib = lut[seq]
    a[:, 51:126] = nib[:, 0::2] << 4 | nib[:, 1::2]
    a[:, 126:276] = qual - 33
    sam = b""
    if want_sam:
        keep = flag == 0
        s = np.full((m, 343), 9, np.uint8)  # name 10, flag 1, chr 3, pos 9, mapq 2, cigar 4, =, pnext 1, tlen 1, seq, qual
        s[:, 0], s[:, 1:10] = ord("r"), digits
        s[:, 11] = 48
        s[:, 13], s[:, 14], s[:, 15] = ord("c"), 48 + ref // 10, 48 + ref % 10
        s[:, 17:26] = ((idx[:, None] % 200_000_000 + 1) // 10 ** np.arange(8, -1, -1)) % 10 + 48
        s[:, 27:29] = np.frombuffer(b"60", np.uint8)
        s[:, 30:34] = np.frombuffer(b"150M", np.uint8)
        s[:, 35], s[:, 37], s[:, 39] = ord("="), 49, 48
        s[:, 41:191], s[:, 192:342], s[:, 342] = seq, qual, 10
        sam = s[keep].tobytes()
    return a.tobytes(), sam


def kernel(args):
    from rufus_amd import capi
    sy = capi.Synth.sample(100_000_000, 0)
    hdr = R.header(REFS)
    n_pairs = (args.bytes - len(hdr)) // REC // 2
    parts = [hdr] + [records(f, min(200_000, n_pairs - f), 2 * n_pairs, sy, False)[0] for f in range(0, n_pairs, 200_000)]
    data = b"".join(parts)
    with ProcessPoolExecutor(16) as ex:
        groups = list(ex.map(_compress, [(data[i:i + GROUP], args.level) for i in range(0, len(data), GROUP)]))
    L = capi.lib()
    reps, pieces = [], [b""]
    for g in groups:  # pieces of <= 8 MiB of whole blocks, as BamIngest appends them (a launch of k_bgzf_inflate each)
        if len(pieces[-1]) + len(g) > 8 << 20:
            pieces.append(b"")
        pieces[-1] += g
    with capi.Context(0) as ctx:
        ctx.prof(True)
        arena = capi.TextArena(ctx, len(data) + 65536)
        pin = L.rfx_host_alloc(max(map(len, pieces)))
        for rep in range(args.reps):
            ctx.prof_reset()
            w0 = time.time()
            for g in pieces:
                C.memmove(pin, g, len(g))
                t = L.rfx_text_append_bgzf(arena._h, C.cast(pin, C.c_char_p), len(g))
                assert t >= 0 and L.rfx_text_wait(arena._h, t) == 0, t
            n, carried = arena.bam_settle(None, len(hdr), len(REFS))
            blk, runs = arena.bam_parse(3328)
            d = ctx.prof_dict()
            row = {k + "_ms": round(v[0], 3) for k, v in d.items() if k.startswith("k_bam") or k in ("k_bgzf_inflate", "scan_tail", "k_scan")}
            row.update({"inflate_launches": d["k_bgzf_inflate"][1], "repair_launches": d["k_bam_repair"][1], "wall_s": round(time.time() - w0, 3), "records": n, "reads": blk.n,
                        "carried": carried, "runs": len(runs), "stats": ctx.bam_stats()})
            assert n == 2 * n_pairs and blk.n == n - (n + 10) // 16 and len(runs) == len(REFS), row
            reps.append(row)
            blk.free()
            arena.reset()
        L.rfx_host_free(pin)
        arena.close()
    bam_ms = sum(v for k, v in reps[-1].items() if k.startswith("k_bam"))
    print(json.dumps({"row": "kernel", "inflated_bytes": len(data), "compressed_bytes": sum(map(len, groups)), "level": args.level,
                      "k_bam_total_ms": round(bam_ms, 3), "of_inflate": round(bam_ms / reps[-1]["k_bgzf_inflate_ms"], 4), "reps": reps}))


def sample(args):
    from rufus_amd import capi
    sy = capi.Synth.sample(args.pairs * 10, 0)
    t0 = time.time()
    with ProcessPoolExecutor(16) as ex, open(f"{args.dir}/s.bam", "wb") as fb, open(f"{args.dir}/s.sam", "wb") as fs:
        pend, first = R.header(REFS), 0
        while first < args.pairs:
            step = min(args.step, args.pairs - first)
            chunks = [records(f, min(200_000, first + step - f), 2 * args.pairs, sy, True) for f in range(first, first + step, 200_000)]
            fs.write(b"".join(c[1] for c in chunks))
            pend += b"".join(c[0] for c in chunks)
            first += step
            whole = len(pend) if first >= args.pairs else len(pend) // B.BLOCK_PAYLOAD * B.BLOCK_PAYLOAD
            for blob in ex.map(_compress, [(pend[i:min(i + GROUP, whole)], args.level) for i in range(0, whole, GROUP)]):
                fb.write(blob)
            pend = pend[whole:]
        fb.write(B.EOF)
    print(json.dumps({"row": "sample", "pairs": args.pairs, "level": args.level, "bam_bytes": os.path.getsize(f"{args.dir}/s.bam"),
                      "sam_bytes": os.path.getsize(f"{args.dir}/s.sam"), "made_in_s": round(time.time() - t0, 1)}))


def count(args):
    jf, out = f"{os.path.abspath(args.bin)}/jellyfish", f"{args.route}.Jhash"
    cmd = {"bam": f"{jf} {COUNT} -o {out} --bam {args.route}.chr s.bam",
           "sam": f"{jf} {COUNT} -o {out} --sam {args.route}.chr s.sam",
           "pipe": f"cat s.sam | {jf} {COUNT} -o {out} --sam {args.route}.chr /dev/stdin"}[args.route]
    t0 = time.time()
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=args.dir, stderr=subprocess.PIPE, timeout=args.limit)
    s = time.time() - t0
    h = hashlib.sha256()
    if p.returncode == 0:
        with open(f"{args.dir}/{out}", "rb") as f:
            f.read(int(f.read(9)))
            for b in iter(lambda: f.read(1 << 24), b""):
                h.update(b)
    print(json.dumps({"row": "count", "route": args.route, "s": round(s, 3), "rc": p.returncode,
                      "payload_sha256": h.hexdigest() if p.returncode == 0 else None,
                      "chr_sha256": hashlib.sha256(open(f"{args.dir}/{args.route}.chr", "rb").read()).hexdigest() if p.returncode == 0 else None,
                      "stderr": p.stderr.decode()[-300:]}))
    sys.exit(p.returncode)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--bytes", type=int, default=1 << 30)
    k.add_argument("--level", type=int, default=6)
    k.add_argument("--reps", type=int, default=3)
    s = sub.add_parser("sample")
    s.add_argument("dir")
    s.add_argument("--pairs", type=int, default=32_000_000)
    s.add_argument("--level", type=int, default=6)
    s.add_argument("--step", type=int, default=1_000_000, help="pairs made and compressed at a time")
    c = sub.add_parser("count")
    c.add_argument("dir")
    c.add_argument("--route", choices=("bam", "sam", "pipe"), required=True)
    c.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
    c.add_argument("--limit", type=int, default=600)
    args = ap.parse_args()
    {"kernel": kernel, "sample": sample, "count": count}[args.what](args)
