"""Recipe of profiles/gzip_inflate.txt: plain gzip inflated on the device (rufus_amd/csrc/rfx_gzip.hip).

One process = one row (a JSON line on stdout), each under a time limit of its own:

    python profiles/gzip_inflate.py kernel --chunk 262144        # 1. the six kernels over 1 GiB of synthetic FASTQ, one chunk size
    python profiles/gzip_inflate.py kernel --chunk 65536 --piece 33554432 ...
    python profiles/gzip_inflate.py sample DIR                   #    the end-to-end leg's sample as s.fq and s.plain.fastq.gz in DIR (tmpfs)
    python profiles/gzip_inflate.py count DIR --route direct     # 2. jellyfish count of s.plain.fastq.gz
    python profiles/gzip_inflate.py count DIR --route pipe       #    gzip -dc s.plain.fastq.gz | jellyfish count ... /dev/stdin

`kernel`: FASTQ text from rfx_synth_text (profiles/bgzf_inflate.py synth_text: 150-base reads, 317 bytes per record) as ONE
gzip member: 16 processes deflate 16 MiB of text each (zlib --level, raw, ended by a full flush; the last one finishes the
stream), the pieces concatenated -- what pigz writes -- and the CRC-32s combined.  The file goes through
rfx_text_append_gzip in pieces of --piece bytes, presented again from `consumed`; the times are the rfx_prof_* spans of the
six kernels and of the copy on the ctx stream, the counts rfx_gzip_stats; the arena's bytes are fetched afterwards and their
CRC-32 compared with the text's.  Beside it, from the same process: k_bgzf_inflate on the same text cut every 65 280 bytes
(the BGZF writer of tests/bgzf_ref.py).  --reps repetitions, the last one reported.  Under `rocprofv3 --pmc ...` (counters
in a run of their own) the same command gives the kernels' counters: --bytes 268435456 --reps 1 --no-bgzf keeps it short.
`count`: wall seconds of the whole process and the sha256 of the output's payload.  Alternate the routes that are compared.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bgzf_inflate as BI  # noqa: E402
from tests import bgzf_ref as B  # noqa: E402

PIECE_TEXT = 16 << 20
COUNT = BI.COUNT
KERNELS = ("k_gz_find", "k_gz_walk", "k_gz_inflate", "k_gz_windows", "k_gz_resolve", "k_gz_crc", "gz_copy")


def _gf2_times(mat, vec):
    s, i = 0, 0
    while vec:
        if vec & 1:
            s ^= mat[i]
        vec >>= 1
        i += 1
    return s


def crc32_combine(crc1, crc2, len2):
    """zlib's crc32_combine: the CRC-32 of A || B from those of A and B and the length of B."""
    if len2 <= 0:
        return crc1
    odd = [0xEDB88320] + [1 << i for i in range(31)]
    even = [_gf2_times(odd, odd[i]) for i in range(32)]
    odd = [_gf2_times(even, even[i]) for i in range(32)]
    while True:
        even = [_gf2_times(odd, odd[i]) for i in range(32)]
        if len2 & 1:
            crc1 = _gf2_times(even, crc1)
        len2 >>= 1
        if not len2:
            break
        odd = [_gf2_times(even, even[i]) for i in range(32)]
        if len2 & 1:
            crc1 = _gf2_times(odd, crc1)
        len2 >>= 1
        if not len2:
            break
    return crc1 ^ crc2


def _deflate(chunk, level, last):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(chunk) + (c.flush() if last else c.flush(zlib.Z_FULL_FLUSH)), zlib.crc32(chunk), len(chunk)


def _deflate_mem(job):
    return _deflate(*job)


def _deflate_range(job):
    path, off, level, last = job
    with open(path, "rb") as f:
        f.seek(off)
        chunk = f.read(PIECE_TEXT)
    return _deflate(chunk, level, last)


def gzip_member(parts, name=b"s.fastq"):
    """One gzip member from [(raw deflate piece, crc, length)] in order."""
    crc, n = 0, 0
    for _, c, ln in parts:
        crc, n = crc32_combine(crc, c, ln), n + ln
    return b"\x1f\x8b\x08\x08\x00\x00\x00\x00\x00\x03" + name + b"\x00", [p for p, _, _ in parts], struct.pack("<II", crc, n & 0xFFFFFFFF)


def kernel(args):
    from rufus_amd import capi
    os.environ["RFX_GZIP_CHUNK"] = str(args.chunk)
    text = BI.synth_text(args.bytes)
    t0 = time.time()
    offs = list(range(0, len(text), PIECE_TEXT))
    with ProcessPoolExecutor(16) as ex:
        parts = list(ex.map(_deflate_mem, [(text[o:o + PIECE_TEXT], args.level, o == offs[-1]) for o in offs]))
        head, raws, tail = gzip_member(parts)
        gz = head + b"".join(raws) + tail
        t_comp = time.time() - t0
        blocks = []
        if not args.no_bgzf:
            blocks = [b for bs in ex.map(BI._compress, [(text[i:i + BI.GROUP], args.level) for i in range(0, len(text), BI.GROUP)]) for b in bs]
    L = capi.lib()
    reps, bgzf_ms = [], []
    with capi.Context(0) as ctx:
        ctx.prof(True)
        arena = capi.TextArena(ctx, len(text) + 4096)
        for rep in range(args.reps):
            ctx.prof_reset()
            w0 = time.time()
            with capi.GzipStream(ctx) as s:
                at, piece, calls = 0, args.piece, 0
                while at < len(gz):
                    n = min(piece, len(gz) - at)
                    got, used = s.append(arena, gz[at:at + n], at + n == len(gz))
                    calls += 1
                    at += used
                    if not got and not used:
                        assert not s.need() and n < len(gz) - at
                        piece *= 2
                st = s.stats()
            wall = time.time() - w0
            d = ctx.prof_dict()
            row = {k + "_ms": round(d[k][0], 3) for k in KERNELS if k in d}
            row.update({"launches_" + k: d[k][1] for k in ("k_gz_walk", "k_gz_inflate") if k in d})
            row.update({"wall_s": round(wall, 3), "calls": calls, "stats": st})
            reps.append(row)
            if rep == args.reps - 1:
                ok = zlib.crc32(arena.fetch()) == zlib.crc32(text)
            arena.reset()
        if blocks:
            piece = 8 << 20
            pin = L.rfx_host_alloc(piece + 65536)
            for rep in range(args.reps):
                ctx.prof_reset()
                i = 0
                while i < len(blocks):
                    j, sz = i, 0
                    while j < len(blocks) and sz + len(blocks[j]) <= piece:
                        sz += len(blocks[j])
                        j += 1
                    buf = b"".join(blocks[i:j])
                    C.memmove(pin, buf, len(buf))
                    t = L.rfx_text_append_bgzf(arena._h, C.cast(pin, C.c_char_p), len(buf))
                    assert t >= 0 and L.rfx_text_wait(arena._h, t) == 0, t
                    i = j
                arena.settle(None)
                bgzf_ms.append(round(ctx.prof_dict()["k_bgzf_inflate"][0], 3))
                arena.reset()
            L.rfx_host_free(pin)
        arena.close()
    last = reps[-1]
    dev_ms = sum(v for k, v in last.items() if k.endswith("_ms") and k != "gz_copy_ms")
    print(json.dumps({"row": "kernel", "chunk": args.chunk, "piece": args.piece, "text_bytes": len(text), "gz_bytes": len(gz),
                      "level": args.level, "compress_s_16_processes": round(t_comp, 2), "six_kernels_ms": round(dev_ms, 3),
                      "out_GBps_of_kernels": round(len(text) / dev_ms / 1e6, 3), "crc_ok": ok, "k_bgzf_inflate_ms": bgzf_ms, "reps": reps}))


def sample(args):
    n_pairs, G = args.pairs, args.pairs * 10
    subprocess.run([f"{ROOT}/rufus_amd/bin/rfx_synth_fastq", str(G), "1", str(max(8, G // 1_000_000)), "12345", "0", str(n_pairs), "s.fq"],
                   cwd=args.dir, check=True, timeout=args.limit)
    size = os.path.getsize(f"{args.dir}/s.fq")
    t0 = time.time()
    offs = list(range(0, size, PIECE_TEXT))
    crc, n = 0, 0
    with ProcessPoolExecutor(16) as ex, open(f"{args.dir}/s.plain.fastq.gz", "wb") as f:
        f.write(b"\x1f\x8b\x08\x08\x00\x00\x00\x00\x00\x03s.fq\x00")
        for raw, c, ln in ex.map(_deflate_range, [(f"{args.dir}/s.fq", o, args.level, o == offs[-1]) for o in offs]):
            f.write(raw)
            crc, n = crc32_combine(crc, c, ln), n + ln
        f.write(struct.pack("<II", crc, n & 0xFFFFFFFF))
    print(json.dumps({"row": "sample", "pairs": n_pairs, "level": args.level, "text_bytes": size,
                      "gz_bytes": os.path.getsize(f"{args.dir}/s.plain.fastq.gz"), "compress_s_16_processes": round(time.time() - t0, 1)}))


def count(args):
    jf, out = f"{os.path.abspath(args.bin)}/jellyfish", f"{args.route}.Jhash"
    cmd = {"direct": f"RFX_CLI_TRACE=1 {jf} {COUNT} -o {out} s.plain.fastq.gz",
           "pipe": f"gzip -dc s.plain.fastq.gz | {jf} {COUNT} -o {out} /dev/stdin"}[args.route]
    if args.route == "pipe" and not shutil.which("gzip"):
        sys.exit("no gzip on this box")
    t0 = time.time()
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=args.dir, stderr=subprocess.PIPE, timeout=args.limit)
    s = time.time() - t0
    h = hashlib.sha256()
    if p.returncode == 0:
        with open(f"{args.dir}/{out}", "rb") as f:
            f.read(int(f.read(9)))
            for b in iter(lambda: f.read(1 << 24), b""):
                h.update(b)
    print(json.dumps({"row": "count", "route": args.route, "bin": args.bin, "s": round(s, 3), "rc": p.returncode,
                      "payload_sha256": h.hexdigest() if p.returncode == 0 else None, "stderr": p.stderr.decode()[-700:]}))
    sys.exit(p.returncode)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--bytes", type=int, default=1 << 30)
    k.add_argument("--level", type=int, default=6)
    k.add_argument("--reps", type=int, default=2)
    k.add_argument("--chunk", type=int, default=1 << 18)
    k.add_argument("--piece", type=int, default=128 << 20)
    k.add_argument("--no-bgzf", action="store_true")
    s = sub.add_parser("sample")
    s.add_argument("dir")
    s.add_argument("--pairs", type=int, default=32_000_000)
    s.add_argument("--level", type=int, default=6)
    s.add_argument("--limit", type=int, default=600)
    c = sub.add_parser("count")
    c.add_argument("dir")
    c.add_argument("--route", choices=("direct", "pipe"), required=True)
    c.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
    c.add_argument("--limit", type=int, default=600)
    args = ap.parse_args()
    {"kernel": kernel, "sample": sample, "count": count}[args.what](args)
