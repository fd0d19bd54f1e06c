#!/usr/bin/env python3
"""Golden values of the single-end read pull, made by the REFERENCE binaries: for each of testRun's three BAMs, what
`samtools view -F 3328 X.bam | oracle/_ref/PassThroughSamCheck.stranded.se CHR | oracle/_ref/RUFUS.Filter.single
Child.k25_c5.HashList stdin STUB 25 15 1 1` writes (runRufus.sh:1031-1032; `make -C oracle ref` compiles the two from the
reference tree where it lies).  `samtools view` is tests/bam_ref.py's reader, with `\tXS:i:0` behind every line: the
reference feeders walk off a line that ends with QUAL.  Run where the reference tree is; the fixture travels, the
reference does not.  Written: testRun/expected_single_bam.json -- per fixture the sha256 of STUB.Mutations.fastq and of
CHR, and the written records' names and `:MH` values.  Data only."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, ROOT)
K, MIN_Q, THRESH = 25, 15, 1


def reference_single(sam: bytes, hl_path: str, k=K, min_q=MIN_Q, thresh=THRESH):
    """(STUB.Mutations.fastq bytes, chromosome log) of the two reference processes over SAM text."""
    sam = b"".join(line + b"\tXS:i:0\n" for line in sam.split(b"\n") if line)
    with tempfile.TemporaryDirectory() as d:
        fq = subprocess.run([os.path.join(REF, "PassThroughSamCheck.stranded.se"), "ref.chr"], input=sam, cwd=d, stdout=subprocess.PIPE,
                            stderr=subprocess.DEVNULL, check=True, timeout=300).stdout
        subprocess.run([os.path.join(REF, "RUFUS.Filter.single"), hl_path, "stdin", "ref", str(k), str(min_q), str(thresh), "1"], input=fq,
                       cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=300)
        return open(os.path.join(d, "ref.Mutations.fastq"), "rb").read(), open(os.path.join(d, "ref.chr"), "rb").read()


def summary(fastq: bytes, log: bytes):
    heads = fastq.split(b"\n")[0::4][:-1] if fastq else []
    names = [h[1:].rsplit(b":MH", 1) for h in heads]
    return {"fastq_sha256": hashlib.sha256(fastq).hexdigest(), "chr_sha256": hashlib.sha256(log).hexdigest(),
            "names": [n.decode() for n, _ in names], "mh": [int(v) for _, v in names]}


if __name__ == "__main__":
    from tests import bam_ref as R
    hl = os.path.join(R.GOLDEN, "Child.k25_c5.HashList")
    out = {name: summary(*reference_single(R.Bam(R.fixture(name)).sam_text(), hl)) for name in ("Child", "Mother", "Father")}
    with open(os.path.join(R.GOLDEN, "expected_single_bam.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v["names"]) for k, v in out.items()})
