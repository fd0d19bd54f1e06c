"""Recipe of profiles/fasta_bgzf.txt: `jellyfish count` on a bgzip'd reference FASTA (rufus_amd/csrc/rfx_fasta.hip, DESIGN
section 4.19).

One process = one row (a JSON line on stdout), each under a time limit of its own:

    python profiles/fasta_bgzf.py sample DIR                   # ref.fa and ref.fa.gz in DIR (tmpfs)
    python profiles/fasta_bgzf.py count DIR --route direct     # jellyfish count of ref.fa.gz
    python profiles/fasta_bgzf.py count DIR --route pipe       # gzip -dc ref.fa.gz | jellyfish count ... /dev/stdin
    python profiles/fasta_bgzf.py count DIR --route plain      # jellyfish count of ref.fa
    python profiles/fasta_bgzf.py kernels DIR                  # the k_fa_* kernels beside k_bgzf_inflate, one arena

`sample`: a seeded synthetic FASTA of about --bases bases in 24 sequences of unequal length, 60-column lines, compressed
by the tests' BGZF writer (tests/bgzf_ref.py, level 6, a pool of 16 processes).
`count`: wall seconds of the whole process and the sha256 of the output's payload.  Alternate the routes that are compared.
`kernels`: the direct count under `rocprofv3 --kernel-trace --stats` (a run of its own; the whole file is one 1 GiB
arena), the rows of its kernel statistics whose names begin with k_fa_, k_txt_ or k_bgzf_.
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bgzf_ref as B  # noqa: E402

GROUP = 64 * B.BLOCK_PAYLOAD
COUNT = "count -m 25 -C -s 8G"


def _compress(job):
    chunk, level = job
    return b"".join(B.block(chunk[i:i + B.BLOCK_PAYLOAD], level) for i in range(0, len(chunk), B.BLOCK_PAYLOAD))


def sample(args):
    import numpy as np
    rng = np.random.default_rng(61)
    share = rng.integers(1, 20, 24).astype(np.float64)
    lens = (share / share.sum() * args.bases).astype(np.int64)
    parts = []
    for i, L in enumerate(lens):
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(L))]
        s[rng.integers(0, int(L), int(L) // 1000)] = ord("N")
        rows = -(-int(L) // 60)
        a = np.full((rows, 61), 10, np.uint8)
        flat = np.zeros(rows * 60, np.uint8)
        flat[:int(L)] = s
        a[:, :60] = flat.reshape(rows, 60)
        body = a.tobytes()
        body = body[:len(body) - (rows * 60 - int(L)) - 1] + b"\n"  # the last line is as long as what is left
        parts.append(b">chr%d synthetic len=%d\n" % (i + 1, int(L)) + body)
    text = b"".join(parts)
    with open(f"{args.dir}/ref.fa", "wb") as f:
        f.write(text)
    t0 = time.time()
    with ProcessPoolExecutor(16) as ex, open(f"{args.dir}/ref.fa.gz", "wb") as f:
        for blob in ex.map(_compress, [(text[o:o + GROUP], args.level) for o in range(0, len(text), GROUP)]):
            f.write(blob)
        f.write(B.EOF)
    print(json.dumps({"row": "sample", "sequences": len(lens), "bases": int(lens.sum()), "shortest": int(lens.min()), "longest": int(lens.max()),
                      "level": args.level, "text_bytes": len(text), "gz_bytes": os.path.getsize(f"{args.dir}/ref.fa.gz"),
                      "compress_s_16_processes": round(time.time() - t0, 1)}))


def _command(args, out):
    jf = f"{os.path.abspath(args.bin)}/jellyfish"
    return {"direct": f"{jf} {COUNT} -o {out} ref.fa.gz",
            "pipe": f"gzip -dc ref.fa.gz | {jf} {COUNT} -o {out} /dev/stdin",
            "plain": f"{jf} {COUNT} -o {out} ref.fa"}[args.route]


def _payload_sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        f.read(int(f.read(9)))
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def count(args):
    out = f"{args.route}.jf"
    if args.route == "pipe" and not shutil.which("gzip"):
        sys.exit("no gzip on this box")
    t0 = time.time()
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + _command(args, out)], cwd=args.dir, stderr=subprocess.PIPE, timeout=args.limit,
                       env=dict(os.environ, RFX_CLI_TRACE="1"))
    s = time.time() - t0
    route = [ln for ln in p.stderr.decode().splitlines() if "route:" in ln]
    print(json.dumps({"row": "count", "route": args.route, "bin": args.bin, "s": round(s, 3), "rc": p.returncode,
                      "payload_sha256": _payload_sha(f"{args.dir}/{out}") if p.returncode == 0 else None,
                      "trace": route[-1].strip() if route else None, "stderr": p.stderr.decode()[-300:] if p.returncode else ""}))
    sys.exit(p.returncode)


def kernels(args):
    args.route = "direct"
    prof = f"{args.dir}/rocprof"
    shutil.rmtree(prof, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--"] + _command(args, "prof.jf").split()
    # (RFX_CLEAN_EXIT: the tool returns from main instead of leaving with _exit, so the profiler writes its tables)
    p = subprocess.run(cmd, cwd=args.dir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit,
                       env=dict(os.environ, RFX_CLEAN_EXIT="1"))
    rows = []
    paths = glob.glob(f"{prof}/**/*kernel_stats.csv", recursive=True)
    if not paths:
        sys.exit(f"no kernel statistics under {prof}: " + " ".join(glob.glob(f"{prof}/**/*", recursive=True))[:600] + p.stderr.decode()[-600:])
    for path in paths:
        for r in csv.DictReader(open(path)):
            m = re.search(r"\bk_[a-z0-9_]+", r.get("Name", ""))  # ("(anonymous namespace)::k_fa_pack(unsigned char const*, ...")
            short = m.group(0) if m else ""
            if short.startswith(("k_fa_", "k_txt_", "k_bgzf_", "k_scan_", "k_reads_tile")):
                rows.append({"kernel": short, "calls": int(r["Calls"]), "total_ms": round(int(r["TotalDurationNs"]) / 1e6, 3)})
    fa = sum(r["total_ms"] for r in rows if r["kernel"].startswith("k_fa_"))
    inflate = sum(r["total_ms"] for r in rows if r["kernel"].startswith("k_bgzf_"))
    print(json.dumps({"row": "kernels", "rc": p.returncode, "k_fa_ms": round(fa, 3), "k_bgzf_inflate_ms": round(inflate, 3),
                      "k_fa_share_of_inflate": round(fa / inflate, 4) if inflate else None, "kernels": rows,
                      "stderr": p.stderr.decode()[-300:] if p.returncode else ""}))
    sys.exit(p.returncode)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    s = sub.add_parser("sample")
    s.add_argument("dir")
    s.add_argument("--bases", type=int, default=200_000_000)
    s.add_argument("--level", type=int, default=6)
    for name in ("count", "kernels"):
        c = sub.add_parser(name)
        c.add_argument("dir")
        if name == "count":
            c.add_argument("--route", choices=("direct", "pipe", "plain"), required=True)
        c.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
        c.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    {"sample": sample, "count": count, "kernels": kernels}[args.what](args)
