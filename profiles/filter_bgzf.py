"""Recipe of profiles/filter_bgzf.txt: `RUFUS.Filter HashList A.fastq.gz B.fastq.gz ...`, both mates inflated, parsed,
scanned and the pulled pairs' text gathered on the device (rufus_amd/csrc/rfx_gather.hip, rfx_ingest.hpp BgzfPairFilter;
DESIGN section 4.13).

One process = one row (a JSON line on stdout), each under a time limit of its own:

    python profiles/filter_bgzf.py sample DIR                   # the end-to-end leg's subject as c.m{1,2}.fq and .fastq.gz in DIR (tmpfs), + hl
    python profiles/filter_bgzf.py filter DIR --route gz        # (a) RUFUS.Filter hl c.m1.fastq.gz c.m2.fastq.gz
    python profiles/filter_bgzf.py filter DIR --route pipe      # (b) RUFUS.Filter hl <(gzip -dc c.m1.fastq.gz) <(gzip -dc c.m2.fastq.gz)
    python profiles/filter_bgzf.py filter DIR --route plain     # (c) RUFUS.Filter hl c.m1.fq c.m2.fq
    python profiles/filter_bgzf.py filter DIR --route plain --bin PARENT_TREE/rufus_amd/bin     (a built checkout of the parent)
    python profiles/filter_bgzf.py kernels DIR                  # rfx_prof_* times of one step of the route, 1 GiB arenas

`sample`: rfx_synth_fastq's child of the synthetic trio (bench.py end_to_end: genome 10 x pairs, seed 12345), each mate
compressed by the tests' BGZF writer (tests/bgzf_ref.py, --level, a pool of 16 processes); the hash list holds the 25
k-mers over every planted SNV's alternative allele.
`filter`: wall seconds of the whole process and the sha256 of the two output files.  Alternate the routes that are compared.
`kernels`: the first blocks of both .fastq.gz, as much as fits arenas of 1 GiB, through the calls of one step of the
executable's route -- append_bgzf, records, settle_records, parse, filter, gather -- with the library's HIP-event spans on.
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
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bgzf_ref as B  # noqa: E402

GROUP = 64 * B.BLOCK_PAYLOAD
K, MIN_Q, THRESH, SEED = 25, 15, 1, 12345


def _compress_range(job):
    path, off, level = job
    with open(path, "rb") as f:
        f.seek(off)
        chunk = f.read(4 * GROUP)
    return b"".join(B.block(chunk[i:i + B.BLOCK_PAYLOAD], level) for i in range(0, len(chunk), B.BLOCK_PAYLOAD))


def sample(args):
    from rufus_amd import capi
    n_pairs, G = args.pairs, args.pairs * 10
    n_snv = max(8, G // 1_000_000)
    t0 = time.time()
    subprocess.run([f"{ROOT}/rufus_amd/bin/rfx_synth_fastq", str(G), "0", str(n_snv), str(SEED), "0", str(n_pairs), "c.m1.fq", "c.m2.fq"],
                   cwd=args.dir, check=True, timeout=args.limit)
    t_gen = time.time() - t0
    sy = capi.Synth.sample(G, 0, n_snv=n_snv, seed=SEED)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    n_hl = 0
    with open(f"{args.dir}/hl", "w") as f:
        for p_, _, alt in sy.snvs():
            c = bytearray(sy.genome(p_ - 24, 49))
            c[24:25] = alt
            for i in range(25):
                km = bytes(c[i:i + 25])
                f.write(min(km, km[::-1].translate(comp)).decode() + " 12\n")
                n_hl += 1
    t0 = time.time()
    sizes = {}
    with ProcessPoolExecutor(16) as ex:
        for m in (1, 2):
            src, dst = f"{args.dir}/c.m{m}.fq", f"{args.dir}/c.m{m}.fastq.gz"
            size = os.path.getsize(src)
            with open(dst, "wb") as f:
                for blob in ex.map(_compress_range, [(src, o, args.level) for o in range(0, size, 4 * GROUP)]):
                    f.write(blob)
                f.write(B.EOF)
            sizes[m] = (size, os.path.getsize(dst))
    print(json.dumps({"row": "sample", "pairs": n_pairs, "level": args.level, "hash_list_kmers": n_hl, "generate_s": round(t_gen, 1),
                      "text_bytes": [sizes[1][0], sizes[2][0]], "gz_bytes": [sizes[1][1], sizes[2][1]],
                      "compress_s_16_processes": round(time.time() - t0, 1)}))


def _sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest(), os.path.getsize(path)


def run_filter(args):
    exe, stub = f"{os.path.abspath(args.bin)}/RUFUS.Filter", f"out_{args.route}"
    tail = f"{stub} {K} {MIN_Q} {THRESH} 16"
    cmd = {"gz": f"{exe} hl c.m1.fastq.gz c.m2.fastq.gz {tail}",
           "pipe": f"{exe} hl <(gzip -dc c.m1.fastq.gz) <(gzip -dc c.m2.fastq.gz) {tail}",
           "plain": f"{exe} hl c.m1.fq c.m2.fq {tail}"}[args.route]
    if args.route == "pipe" and not shutil.which("gzip"):
        sys.exit("no gzip on this box")
    t0 = time.time()
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=args.dir, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       timeout=args.limit, env=dict(os.environ, RFX_CLI_TRACE="1"))
    s = time.time() - t0
    err = p.stderr.decode()
    route = [ln for ln in err.splitlines() if "bgzf route: " in ln]
    row = {"row": "filter", "route": args.route, "bin": args.bin, "s": round(s, 3), "rc": p.returncode}
    if p.returncode == 0:
        for m in (1, 2):
            row[f"mate{m}_sha256"], row[f"mate{m}_bytes"] = _sha(f"{args.dir}/{stub}.Mutations.Mate{m}.fastq")
    if route:
        row["trace"] = route[-1].split("] ", 1)[-1]
    if p.returncode != 0:
        row["stderr"] = err[-300:]
    print(json.dumps(row))
    sys.exit(p.returncode)


def kernels(args):
    import numpy as np
    from rufus_amd import capi
    L = capi.lib()
    cap = 1 << 30
    keys = capi.hashlist_keys(open(f"{args.dir}/hl", "rb").read(), K)
    with capi.Context(0) as ctx:
        mset = capi.MutantSet(ctx, keys, K)
        arenas = [(capi.TextArena(ctx, cap), capi.TextArena(ctx, cap)) for _ in range(2)]
        piece = 8 << 20
        pin = L.rfx_host_alloc(piece)
        ctx.prof(True)
        ctx.prof_reset()
        w0 = time.time()
        gz_bytes = 0
        for m in (1, 2):
            a = arenas[m - 1][0]
            with open(f"{args.dir}/c.m{m}.fastq.gz", "rb") as f:
                carry = b""
                while True:
                    buf = carry + f.read(piece - len(carry))
                    nb, used, inf = capi.bgzf_scan(buf)
                    if nb == 0 or inf > cap - a.bytes:
                        break
                    C.memmove(pin, buf, used)
                    t = L.rfx_text_append_bgzf(a._h, C.cast(pin, C.c_char_p), used)
                    assert t >= 0 and L.rfx_text_wait(a._h, t) == 0, t
                    gz_bytes += used
                    carry = buf[used:]
        r = [arenas[m][0].records() for m in range(2)]
        n = min(r)
        text_bytes = 0
        for m in range(2):
            arenas[m][0].settle_records(arenas[m][1], n)
            text_bytes += arenas[m][0].bytes
        mask = None
        for m in range(2):
            blk = arenas[m][0].parse(capi.PACK_FILTER, MIN_Q)
            _, mk, _ = mset.filter(blk, THRESH, True, want_hits=False)
            mask = mk.copy() if mask is None else mask | mk
            blk.free()
        out = [arenas[m][0].gather(mask, n) for m in range(2)]
        wall = time.time() - w0
        d = ctx.prof_dict()
        L.rfx_host_free(pin)
    pulled = int(np.unpackbits(mask.view(np.uint8), bitorder="little")[:n].sum())
    print(json.dumps({"row": "kernels", "records_per_arena": r, "pairs": n, "pulled": pulled, "gathered_bytes": [len(o) for o in out],
                      "text_bytes": text_bytes, "gz_bytes": gz_bytes, "wall_s": round(wall, 3),
                      "spans_ms_launches": {k: [round(v[0], 3), v[1]] for k, v in sorted(d.items())}}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    s = sub.add_parser("sample")
    s.add_argument("dir")
    s.add_argument("--pairs", type=int, default=32_000_000)
    s.add_argument("--level", type=int, default=6)
    s.add_argument("--limit", type=int, default=600)
    c = sub.add_parser("filter")
    c.add_argument("dir")
    c.add_argument("--route", choices=("gz", "pipe", "plain"), required=True)
    c.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
    c.add_argument("--limit", type=int, default=600)
    k = sub.add_parser("kernels")
    k.add_argument("dir")
    args = ap.parse_args()
    {"sample": sample, "filter": run_filter, "kernels": kernels}[args.what](args)
