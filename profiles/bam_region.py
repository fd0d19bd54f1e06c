"""Recipe of profiles/bam_region.txt: `jellyfish count --bam CHR --region REG` through the BAM's .bai.

One process = one row (a JSON line on stdout), each under a time limit of its own.  The file is profiles/bam_count.py's
sample (`python profiles/bam_count.py sample DIR --pairs 4000000`: 8 M records of 276 bytes, sorted, 25 references):

    python profiles/bam_region.py index DIR                  # s.bam.bai for DIR/s.bam (numpy: the records are equally long)
    python profiles/bam_region.py count DIR --route index    # jellyfish count --bam CHR --region REG s.bam, index beside it
    python profiles/bam_region.py count DIR --route walk     # ... the index moved away: the whole file walked, the device decides
    python profiles/bam_region.py count DIR --route whole [--bin PARENT/rufus_amd/bin]    # no --region (also the parent's build)
    python profiles/bam_region.py kernel                     # k_bam_region beside k_bgzf_inflate, one 1 GiB arena

REG = c12:3900001-3980000: 80 000 of the 8 M records, 1 %.  `count`: wall seconds of the whole process, the trace's block
count, the payload's sha256.  Alternate the routes that are compared.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bam_count as BC  # noqa: E402
from tests import bai_ref as X  # noqa: E402
from tests import bam_ref as R  # noqa: E402
from tests import bgzf_ref as B  # noqa: E402

REGION = "c12:3900001-3980000"


def index(args):
    """The fine index of bai_ref.build, written from arithmetic: record i lies at inflated byte len(header) + 276 i, reference
    i * 25 // n, position i; a block holds BLOCK_PAYLOAD inflated bytes; its compressed offset comes from the file."""
    import numpy as np
    path = f"{args.dir}/s.bam"
    coff, at, size = [], 0, os.path.getsize(path)
    with open(path, "rb") as f:
        while at < size:
            f.seek(at + 16)
            coff.append(at)
            at += struct.unpack("<H", f.read(2))[0] + 1
    coff = np.array(coff, np.uint64)
    hdr = len(R.header(BC.REFS))
    with open(path, "rb") as f:  # (the last block is the EOF marker; the data block in front of it ends with its ISIZE)
        f.seek(int(coff[-1]) - 4)
        last_isize = struct.unpack("<I", f.read(4))[0]
    n = ((len(coff) - 2) * B.BLOCK_PAYLOAD + last_isize - hdr) // BC.REC
    idx = np.arange(n, dtype=np.int64)
    ref = idx * len(BC.REFS) // n
    pos = idx % 200_000_000

    def voff(off):
        return coff[off // B.BLOCK_PAYLOAD] << np.uint64(16) | (off % B.BLOCK_PAYLOAD).astype(np.uint64)

    start, end = voff(hdr + BC.REC * idx), voff(hdr + BC.REC * (idx + 1))
    bins = np.full(n, 0, np.int64)
    done = np.zeros(n, bool)
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        same = ~done & (pos >> shift == (pos + 149) >> shift)
        bins[same] = first + (pos[same] >> shift)
        done |= same
    out = [b"BAI\x01", struct.pack("<i", len(BC.REFS))]
    for tid in range(len(BC.REFS)):
        lo, hi = np.searchsorted(ref, [tid, tid + 1])
        b, s, e, p = bins[lo:hi], start[lo:hi], end[lo:hi], pos[lo:hi]
        cut = np.flatnonzero(np.diff(b)) + 1
        firsts, lasts = np.concatenate([[0], cut]), np.concatenate([cut, [len(b)]]) - 1
        chunks = {}
        for f0, l0 in zip(firsts.tolist(), lasts.tolist()):
            chunks.setdefault(int(b[f0]), []).append((int(s[f0]), int(e[l0])))
        out.append(struct.pack("<i", len(chunks)))
        for k in sorted(chunks):
            out.append(struct.pack("<Ii", k, len(chunks[k])) + b"".join(struct.pack("<QQ", *c) for c in chunks[k]))
        n_intv = int((p[-1] + 149) >> 14) + 1
        lin = np.full(n_intv, np.iinfo(np.uint64).max, np.uint64)
        for w in (p >> 14, (p + 149) >> 14):
            np.minimum.at(lin, w, s)
        nxt = 0
        for w in range(n_intv - 1, -1, -1):  # empty windows filled from the right
            nxt = int(lin[w]) if lin[w] != np.iinfo(np.uint64).max else nxt
            lin[w] = nxt
        out.append(struct.pack("<i", n_intv) + lin.astype("<u8").tobytes())
    bai = b"".join(out)
    open(path + ".bai", "wb").write(bai)
    region = X.parse_region(REGION, [name for name, _ in BC.REFS])
    q = X.query(X.parse(bai), *region)
    print(json.dumps({"row": "index", "records": int(n), "blocks": len(coff), "bai_bytes": len(bai), "region": REGION,
                      "records_in_region": int(((ref == region[0]) & (pos < region[2]) & (pos + 150 > region[1])).sum()),
                      "blocks_of_range": int(((coff >= q[0] >> 16) & (coff <= (q[1] >> 16 if q[1] & 0xFFFF else (q[1] >> 16) - 1))).sum())}))


def count(args):
    jf, out = f"{os.path.abspath(args.bin)}/jellyfish", f"{args.route}.Jhash"
    bai, away = f"{args.dir}/s.bam.bai", f"{args.dir}/s.bam.bai.away"
    if args.route == "walk" and os.path.exists(bai):
        os.rename(bai, away)
    if args.route == "index" and not os.path.exists(bai):
        os.rename(away, bai)
    region = [] if args.route == "whole" else ["--region", REGION]
    cmd = [jf] + BC.COUNT.split() + ["-o", out, "--bam", f"{args.route}.chr"] + region + ["s.bam"]
    t0 = time.time()
    p = subprocess.run(cmd, cwd=args.dir, stderr=subprocess.PIPE, timeout=args.limit, env=dict(os.environ, RFX_CLI_TRACE="1"))
    s = time.time() - t0
    h = hashlib.sha256()
    if p.returncode == 0:
        with open(f"{args.dir}/{out}", "rb") as f:
            f.read(int(f.read(9)))
            for b in iter(lambda: f.read(1 << 24), b""):
                h.update(b)
    err = p.stderr.decode()
    m = re.search(r"bam route: (\d+) blocks .*", err)
    print(json.dumps({"row": "count", "route": args.route, "bin": args.bin, "s": round(s, 3), "rc": p.returncode,
                      "payload_sha256": h.hexdigest() if p.returncode == 0 else None, "trace": m.group(0) if m else err[-300:]}))
    sys.exit(p.returncode)


def kernel(args):
    from rufus_amd import capi
    sy = capi.Synth.sample(100_000_000, 0)
    hdr = R.header(BC.REFS)
    n_pairs = (args.bytes - len(hdr)) // BC.REC // 2
    data = b"".join([hdr] + [BC.records(f, min(200_000, n_pairs - f), 2 * n_pairs, sy, False)[0] for f in range(0, n_pairs, 200_000)])
    with ProcessPoolExecutor(16) as ex:
        groups = list(ex.map(BC._compress, [(data[i:i + BC.GROUP], args.level) for i in range(0, len(data), BC.GROUP)]))
    L = capi.lib()
    pieces = [b""]
    for g in groups:
        if len(pieces[-1]) + len(g) > 8 << 20:
            pieces.append(b"")
        pieces[-1] += g
    n = 2 * n_pairs
    tid, beg, end = 12, 12 * n // 25 + n // 100, 12 * n // 25 + 2 * n // 100  # 1 % of the arena's records
    reps = []
    with capi.Context(0) as ctx:
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
            n_in = arena.bam_set_region(tid, beg, end)
            blk, _ = arena.bam_parse(3328)
            d = ctx.prof_dict()
            reps.append({"k_bam_region_ms": round(d["k_bam_region"][0], 4), "k_bgzf_inflate_ms": round(d["k_bgzf_inflate"][0], 3),
                         "k_bam_fields_ms": round(d["k_bam_fields"][0], 4), "k_bam_pack_ms": round(d["k_bam_pack"][0], 4),
                         "records": n_rec, "in_region": n_in, "reads": blk.n})
            assert n_rec == n and abs(n_in - n // 100) <= 150, reps[-1]
            blk.free()
            arena.reset()
        L.rfx_host_free(pin)
        arena.close()
    print(json.dumps({"row": "kernel", "inflated_bytes": len(data), "reps": reps}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    i = sub.add_parser("index")
    i.add_argument("dir")
    c = sub.add_parser("count")
    c.add_argument("dir")
    c.add_argument("--route", choices=("index", "walk", "whole"), required=True)
    c.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
    c.add_argument("--limit", type=int, default=600)
    k = sub.add_parser("kernel")
    k.add_argument("--bytes", type=int, default=1 << 30)
    k.add_argument("--level", type=int, default=6)
    k.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    {"index": index, "count": count, "kernel": kernel}[args.what](args)
