"""Recipe of profiles/filter_bam.txt: the subject's hit pairs pulled straight from its BAM (RUFUS.Filter --bam; rfx_ingest.hpp
BamPairFilter, rufus_amd/csrc/rfx_bam.hip).

One process = one row (a JSON line on stdout), each under a time limit of its own:

    python profiles/filter_bam.py sample DIR --pairs N      # N pairs as s.bam, the kept records as s.sam, a hash list hl (tmpfs)
    python profiles/filter_bam.py filter DIR --route bam    # RUFUS.Filter --bam CHR hl s.bam ...
    python profiles/filter_bam.py filter DIR --route sam    # RUFUS.Filter --sam CHR hl s.sam ...
    python profiles/filter_bam.py filter DIR --route pipe   # cat s.sam | RUFUS.Filter --sam CHR hl stdin ...   (runRufus.sh:966)

`sample`: profiles/bam_count.py's records (reads of rfx_synth_text, 150 bases, records of 276 bytes, every 16th record with
flag 1024) with a QNAME per PAIR, mate 1 forward (flag 99), mate 2 on the reverse strand (flag 83), mate 2 about 300
records behind mate 1, every 4096th record on the next reference.  The hash list holds every 7th 25-mer of mate 1 of every
--every'th pair: the share of pairs it pulls is in the `filter` rows (pairs / reads * 2).
`filter`: wall seconds of the whole process, the sha256 of the two Mate files and of the chromosome log, and for --bam the
route's trace lines (pass 1 / pass 2 marks).  Alternate the routes that are compared.
"""
import argparse
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
from tests import bam_ref as R  # noqa: E402
from tests import bgzf_ref as B  # noqa: E402

K, MIN_Q, THRESH = 25, 15, 1
CHUNK = 200_000  # pairs made at a time; the mates are shuffled inside a chunk


def records(first_pair, n_pairs, total_reads, sy, every):
    """(BAM records, SAM lines of the kept ones, hash-list lines) of pairs first_pair .. first_pair + n_pairs - 1."""
    import numpy as np
    seq, qual = sy.text(first_pair, n_pairs)
    m = 2 * n_pairs
    idx = np.arange(2 * first_pair, 2 * first_pair + m)
    order = np.argsort(np.where(idx & 1, idx + 600, idx), kind="stable")  # mate 2 about 300 records behind mate 1
    idx, seq, qual = idx[order], seq[order], qual[order]
    at = 2 * first_pair + np.arange(m)  # position in the file
    ref = ((at * len(BC.REFS) // total_reads + (at % 4096 == 7)) % len(BC.REFS)).astype(np.int32)
    mate2 = (idx & 1).astype(bool)
    flag = (np.where(mate2, 83, 99) | np.where(idx % 16 == 5, 1024, 0)).astype(np.uint16)
    # a reverse-strand record stores the reference strand: the stored sequence is the read's reverse complement
    comp = np.zeros(256, np.uint8)
    comp[[65, 67, 71, 84, 78]] = [84, 71, 67, 65, 78]
    seq = np.where(mate2[:, None], comp[seq[:, ::-1]], seq)
    qual = np.where(mate2[:, None], qual[:, ::-1], qual)
    digits = (((idx // 2)[:, None] // 10 ** np.arange(8, -1, -1)) % 10 + 48).astype(np.uint8)
    a = np.zeros((m, BC.REC), np.uint8)
    head = np.zeros(m, np.dtype([("bs", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                                 ("n_cigar", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")]))
    head["bs"], head["ref"], head["pos"], head["l_name"], head["mapq"], head["bin"] = BC.REC - 4, ref, at % 200_000_000, 11, 60, 4680
    head["n_cigar"], head["flag"], head["l_seq"], head["nref"], head["npos"] = 1, flag, 150, ref, at % 200_000_000
    a[:, :36] = head.view(np.uint8).reshape(m, 36)
    a[:, 36], a[:, 37:46] = ord("r"), digits
    a[:, 47:51] = np.frombuffer((150 << 4).to_bytes(4, "little"), np.uint8)
    lut = np.full(256, 15, np.uint8)
    lut[[65, 67, 71, 84]] = [1, 2, 4, 8]
    nib = lut[seq]
    a[:, 51:126] = nib[:, 0::2] << 4 | nib[:, 1::2]
    a[:, 126:276] = qual - 33
    keep = (flag & 1024) == 0
    s = np.full((m, 344), 9, np.uint8)  # name 10, flag 2, chr 3, pos 9, mapq 2, cigar 4, =, pnext 1, tlen 1, seq, qual
    s[:, 0], s[:, 1:10] = ord("r"), digits
    s[:, 11], s[:, 12] = np.where(mate2, 56, 57), np.where(mate2, 51, 57)  # "83" / "99"
    s[:, 14], s[:, 15], s[:, 16] = ord("c"), 48 + ref // 10, 48 + ref % 10
    s[:, 18:27] = ((at[:, None] % 200_000_000 + 1) // 10 ** np.arange(8, -1, -1)) % 10 + 48
    s[:, 28:30] = np.frombuffer(b"60", np.uint8)
    s[:, 31:35] = np.frombuffer(b"150M", np.uint8)
    s[:, 36], s[:, 38], s[:, 40] = ord("="), 49, 48
    s[:, 42:192], s[:, 193:343], s[:, 343] = seq, qual, 10
    hl = []
    for r in np.flatnonzero((~mate2) & ((idx // 2) % every == 0)):
        t = seq[r].tobytes()
        hl += [t[i:i + K] + b" 9\n" for i in range(0, 150 - K, 7)]
    return a.tobytes(), s[keep].tobytes(), b"".join(hl)


def sample(args):
    from rufus_amd import capi
    sy = capi.Synth.sample(args.pairs * 10, 0)
    t0 = time.time()
    with ProcessPoolExecutor(16) as ex, open(f"{args.dir}/s.bam", "wb") as fb, open(f"{args.dir}/s.sam", "wb") as fs, \
            open(f"{args.dir}/hl", "wb") as fh:
        pend, first = R.header(BC.REFS), 0
        while first < args.pairs:
            step = min(args.step, args.pairs - first)
            chunks = [records(f, min(CHUNK, first + step - f), 2 * args.pairs, sy, args.every) for f in range(first, first + step, CHUNK)]
            fs.write(b"".join(c[1] for c in chunks))
            fh.write(b"".join(c[2] for c in chunks))
            pend += b"".join(c[0] for c in chunks)
            first += step
            whole = len(pend) if first >= args.pairs else len(pend) // B.BLOCK_PAYLOAD * B.BLOCK_PAYLOAD
            for blob in ex.map(BC._compress, [(pend[i:min(i + BC.GROUP, whole)], args.level) for i in range(0, whole, BC.GROUP)]):
                fb.write(blob)
            pend = pend[whole:]
        fb.write(B.EOF)
    print(json.dumps({"row": "sample", "pairs": args.pairs, "level": args.level, "every": args.every,
                      "bam_bytes": os.path.getsize(f"{args.dir}/s.bam"), "sam_bytes": os.path.getsize(f"{args.dir}/s.sam"),
                      "hash_list_lines": open(f"{args.dir}/hl", "rb").read().count(b"\n"), "made_in_s": round(time.time() - t0, 1)}))


def run_filter(args):
    exe, stub = f"{os.path.abspath(args.bin)}/RUFUS.Filter", args.route
    tail = f"{stub} {K} {MIN_Q} {THRESH} 16"
    cmd = {"bam": f"{exe} --bam {stub}.chr hl s.bam {tail}",
           "sam": f"{exe} --sam {stub}.chr hl s.sam {tail}",
           "pipe": f"cat s.sam | {exe} --sam {stub}.chr hl stdin {tail}"}[args.route]
    t0 = time.time()
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=args.dir, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       timeout=args.limit, env=dict(os.environ, RFX_CLI_TRACE="1"))
    s = time.time() - t0
    sha = {}
    if p.returncode == 0:
        for f in (f"{stub}.Mutations.Mate1.fastq", f"{stub}.Mutations.Mate2.fastq", f"{stub}.chr"):
            sha[f.split(".", 1)[1]] = hashlib.sha256(open(f"{args.dir}/{f}", "rb").read()).hexdigest()[:16]
        sha["pairs"] = open(f"{args.dir}/{stub}.Mutations.Mate1.fastq", "rb").read().count(b"\n") // 4
    trace = [ln for ln in p.stderr.decode().splitlines() if "--bam" in ln or "bam filter route" in ln or "all pieces done" in ln]
    print(json.dumps({"row": "filter", "route": args.route, "s": round(s, 3), "rc": p.returncode, **sha, "trace": trace[-6:],
                      "stderr": "" if p.returncode == 0 else p.stderr.decode()[-300:]}))
    sys.exit(p.returncode)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    s = sub.add_parser("sample")
    s.add_argument("dir")
    s.add_argument("--pairs", type=int, default=4_000_000)
    s.add_argument("--level", type=int, default=6)
    s.add_argument("--every", type=int, default=200_000, help="the hash list takes mate 1 of every N-th pair")
    s.add_argument("--step", type=int, default=1_000_000, help="pairs made and compressed at a time")
    f = sub.add_parser("filter")
    f.add_argument("dir")
    f.add_argument("--route", choices=("bam", "sam", "pipe"), required=True)
    f.add_argument("--bin", default=f"{ROOT}/rufus_amd/bin")
    f.add_argument("--limit", type=int, default=300)
    args = ap.parse_args()
    {"sample": sample, "filter": run_filter}[args.what](args)
