"""Recipe of profiles/bgzf_inflate.txt: BGZF inflated on the device (rufus_amd/csrc/rfx_bgzf.hip).

One process = one row (a JSON line on stdout), each under a time limit of its own:

    python profiles/bgzf_inflate.py kernel                      # 1. k_bgzf_inflate over 1 GiB of synthetic FASTQ
    python profiles/bgzf_inflate.py sample DIR                  #    the end-to-end leg's sample as s.fq and s.fastq.gz in DIR (tmpfs)
    python profiles/bgzf_inflate.py count DIR --route direct    # 2. jellyfish count of s.fastq.gz
    python profiles/bgzf_inflate.py count DIR --route pipe      #    gzip -dc s.fastq.gz | jellyfish count ... /dev/stdin
    python profiles/bgzf_inflate.py count DIR --route plain     # 3. jellyfish count of s.fq
    python profiles/bgzf_inflate.py count DIR --route plain --bin PARENT_TREE/rufus_amd/bin     (a built checkout of the parent)

`kernel`: FASTQ text from rfx_synth_text (150-base reads, 317 bytes per record) cut every 65 280 bytes and compressed by the
tests' BGZF writer (tests/bgzf_ref.py, --level, a pool of 16 processes), appended in pieces of <= 8 MiB from one page-locked
buffer, three repetitions; the times are the rfx_prof_* spans `k_bgzf_inflate` and `bgzf_copy` on the arena's own streams;
the arena's bytes are fetched after the last repetition and their CRC-32 compared with the text's.  Beside it: one
zlib.decompress thread over the first 1000 blocks.  Under `rocprofv3 --pmc ...` (counters in a run of their own) the same
command gives the kernel's counters: --bytes 268435456 --reps 1 keeps that run short.
`count`: wall seconds of the whole process and the sha256 of the output's payload.  Alternate the routes that are compared.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bgzf_ref as B  # noqa: E402

GROUP = 64 * B.BLOCK_PAYLOAD
COUNT = "count --disk -m 25 -L 2 -s 8G -t 16 -C"


def _compress(job):
    chunk, level = job
    return [B.block(chunk[i:i + B.BLOCK_PAYLOAD], level) for i in range(0, len(chunk), B.BLOCK_PAYLOAD)]


def _compress_range(job):
    path, off, level = job
    with open(path, "rb") as f:
        f.seek(off)
        chunk = f.read(4 * GROUP)
    return b"".join(_compress((chunk, level)))


def synth_text(total):
    import numpy as np
    from rufus_amd import capi
    sy = capi.Synth.sample(100_000_000, 0)
    rec = 13 + 151 + 2 + 151
    n = total // rec // 2 * 2
    parts = []
    for first in range(0, n // 2, 200_000):
        m = min(200_000, n // 2 - first)
        seq, qual = sy.text(first, m)
        idx = np.arange(2 * first, 2 * first + 2 * m)
        a = np.empty((2 * m, rec), np.uint8)
        a[:, 0], a[:, 1], a[:, 11], a[:, 12] = ord("@"), ord("r"), ord("/"), 10
        a[:, 2:11] = (idx[:, None] // 10 ** np.arange(8, -1, -1)) % 10 + 48
        a[:, 13:163], a[:, 163], a[:, 164], a[:, 165] = seq, 10, ord("+"), 10
        a[:, 166:316], a[:, 316] = qual, 10
        parts.append(a.tobytes())
    return b"".join(parts)


def kernel(args):
    from rufus_amd import capi
    text = synth_text(args.bytes)
    t0 = time.time()
    with ProcessPoolExecutor(16) as ex:
        blocks = [b for bs in ex.map(_compress, [(text[i:i + GROUP], args.level) for i in range(0, len(text), GROUP)]) for b in bs]
    t_comp = time.time() - t0
    comp_bytes = sum(map(len, blocks))
    t0, done = time.time(), 0
    for b in blocks[:1000]:
        done += len(zlib.decompress(B.parts(b)[1], -15))
    t_z = time.time() - t0
    L = capi.lib()
    reps = []
    with capi.Context(0) as ctx:
        ctx.prof(True)
        arena = capi.TextArena(ctx, len(text) + 4096)
        piece = 8 << 20
        pin = L.rfx_host_alloc(piece + 65536)
        for rep in range(args.reps):
            ctx.prof_reset()
            i, w0 = 0, time.time()
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
            d = ctx.prof_dict()
            reps.append({"k_bgzf_inflate_ms": d["k_bgzf_inflate"][0], "launches": d["k_bgzf_inflate"][1], "bgzf_copy_ms": d["bgzf_copy"][0],
                         "wall_s": time.time() - w0})
            if rep == args.reps - 1:
                ok = zlib.crc32(arena.fetch()) == zlib.crc32(text)
            arena.reset()
        L.rfx_host_free(pin)
        arena.close()
    ms, cms = reps[-1]["k_bgzf_inflate_ms"], reps[-1]["bgzf_copy_ms"]
    print(json.dumps({"row": "kernel", "text_bytes": len(text), "compressed_bytes": comp_bytes, "level": args.level, "blocks": len(blocks),
                      "compress_s_16_processes": round(t_comp, 2), "out_GBps": len(text) / ms / 1e6, "in_GBps": comp_bytes / ms / 1e6,
                      "copy_GBps": comp_bytes / cms / 1e6, "host_zlib_1_thread_GBps": done / t_z / 1e9, "crc_ok": ok, "reps": reps}))


def sample(args):
    n_pairs, G = args.pairs, args.pairs * 10
    subprocess.run([f"{ROOT}/rufus_amd/bin/rfx_synth_fastq", str(G), "1", str(max(8, G // 1_000_000)), "12345", "0", str(n_pairs), "s.fq"],
                   cwd=args.dir, check=True, timeout=args.limit)
    size = os.path.getsize(f"{args.dir}/s.fq")
    t0 = time.time()
    with ProcessPoolExecutor(16) as ex, open(f"{args.dir}/s.fastq.gz", "wb") as f:
        for blob in ex.map(_compress_range, [(f"{args.dir}/s.fq", o, args.level) for o in range(0, size, 4 * GROUP)]):
            f.write(blob)
        f.write(B.EOF)
    print(json.dumps({"row": "sample", "pairs": n_pairs, "level": args.level, "text_bytes": size,
                      "gz_bytes": os.path.getsize(f"{args.dir}/s.fastq.gz"), "compress_s_16_processes": round(time.time() - t0, 1)}))


def count(args):
    jf, out = f"{os.path.abspath(args.bin)}/jellyfish", f"{args.route}.Jhash"
    cmd = {"direct": f"{jf} {COUNT} -o {out} s.fastq.gz",
           "pipe": f"gzip -dc s.fastq.gz | {jf} {COUNT} -o {out} /dev/stdin",
           "plain": f"{jf} {COUNT} -o {out} s.fq"}[args.route]
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
                      "payload_sha256": h.hexdigest() if p.returncode == 0 else None, "stderr": p.stderr.decode()[-300:]}))
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
    s.add_argument("--limit", type=int, default=600)
    c = sub.add_parser("count")
    c.add_argument("dir")
    c.add_argument("--route", choices=("direct", "pipe", "plain"), required=True)
    c.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
    c.add_argument("--limit", type=int, default=600)
    args = ap.parse_args()
    {"kernel": kernel, "sample": sample, "count": count}[args.what](args)
