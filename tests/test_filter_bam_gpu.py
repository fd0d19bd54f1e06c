"""GPU, through the executables: `RUFUS.Filter --bam CHR HashList X.bam STUB ...` must write, byte for byte, the three files
`RUFUS.Filter --sam CHR HashList X.sam STUB ...` writes for the SAM text tests/bam_ref.py's reader makes of the same file
(`samtools view -F N X.bam`, N = 3328 unless --bam-exclude says otherwise) -- on the three testRun BAMs, on the crafted
file of tests/filter_bam_ref.py (where the oracle's pull of the feeder's pairs is the second reference) and on
bam_ref.synthetic() with every record kept; with 1 GiB arenas and with RFX_BAM_ARENA=1048576, so that mates lie in
different arenas.  `--sam` itself is held to the reference binaries by tests/test_cli_gpu.py.  Fails without the feature:
`--bam` is not an option of RUFUS.Filter."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bam_ref as R
from tests import bgzf_ref as B
from tests import filter_bam_ref as FB
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
HL = os.path.join(R.GOLDEN, "Child.k25_c5.HashList")
TRACE = re.compile(r"bam filter route: arenas (\d+) records (\d+) reads (\d+) hits (\d+) names (\d+) gathered (\d+) pairs (\d+)")


def _filter(d, route, chr_file, hl, inp, stub, min_q=FB.MIN_Q, threads=4, extra=(), env=None, stdin=None):
    argv = [f"{BIN}/RUFUS.Filter", route, chr_file, hl, inp, stub, str(FB.K), str(min_q), str(FB.THRESH), str(threads)] + list(extra)
    return subprocess.run(argv, cwd=d, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _outputs(d, stub, chr_file):
    return [open(os.path.join(d, f), "rb").read() for f in (f"{stub}.Mutations.Mate1.fastq", f"{stub}.Mutations.Mate2.fastq", chr_file)]


def _counts(r):
    m = TRACE.search(r.stderr.decode())
    assert m, r.stderr[-1500:]
    return dict(zip(("arenas", "records", "reads", "hits", "names", "gathered", "pairs"), map(int, m.groups())))


def _sam(d, bam, hl, min_q=FB.MIN_Q, exclude=3328):
    with open(os.path.join(d, "x.sam"), "wb") as f:
        f.write(bam.sam_text(exclude))
    r = _filter(d, "--sam", "sam.chr", hl, "x.sam", "sam", min_q)
    assert r.returncode == 0, r.stderr[-1500:]
    return _outputs(d, "sam", "sam.chr")


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    """name -> (Bam, the three files of --sam over the reader's SAM text): once, shared."""
    out = {}
    for name in ("Child", "Mother", "Father"):
        bam = R.Bam(R.fixture(name))
        out[name] = (bam, _sam(str(tmp_path_factory.mktemp("sam_" + name)), bam, HL))
    return out


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    blob, hl, _ = FB.crafted()
    bam = R.Bam(blob)
    d = tmp_path_factory.mktemp("crafted")
    (d / "hl").write_bytes(hl)
    return bam, str(d / "hl"), _sam(str(d), bam, str(d / "hl")), FB.expected(bam, hl)


@pytest.mark.parametrize("arena", [None, "1048576"])
@pytest.mark.parametrize("name", ["Child", "Mother", "Father"])
def test_filter_bam_equals_filter_sam_on_the_fixtures(samples, tmp_path, name, arena):
    bam, want = samples[name]
    d = str(tmp_path)
    open(f"{d}/x.bam", "wb").write(bam.bam)
    r = _filter(d, "--bam", "bam.chr", HL, "x.bam", "bam", env={"RFX_BAM_ARENA": arena} if arena else None)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _outputs(d, "bam", "bam.chr")
    assert got == want and got[2] == bam.chr_log()
    c = _counts(r)
    assert (c["records"], c["reads"]) == (len(bam.records), len(bam.kept()))
    assert c["arenas"] == 1 if arena is None else c["arenas"] >= 2
    assert c["pairs"] == got[0].count(b"\n") // 4 and c["gathered"] >= 2 * c["pairs"] and c["hits"] >= c["pairs"]
    if name == "Child":
        assert c["pairs"] == 26


@pytest.mark.parametrize("threads", [1, 5])
@pytest.mark.parametrize("arena", [None, "1048576"])
def test_crafted_file_equals_filter_sam_and_the_oracle(crafted, tmp_path, arena, threads):
    bam, hl, want, (e1, e2, log, idx) = crafted
    d = str(tmp_path)
    open(f"{d}/x.bam", "wb").write(bam.bam)
    r = _filter(d, "--bam", "bam.chr", hl, "x.bam", "bam", threads=threads, env={"RFX_BAM_ARENA": arena} if arena else None)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _outputs(d, "bam", "bam.chr")
    assert got == want
    assert got == [e1, e2, log] and len(idx) >= 20  # names and bytes, in the order the pairs complete
    c = _counts(r)
    assert c["pairs"] == len(idx) and (c["arenas"] >= 2) == (arena is not None)


def test_bam_exclude_0_on_the_synthetic_file(tmp_path):
    bam = R.Bam(R.synthetic())
    d = str(tmp_path)
    hl = FB.own_hash_list(bam, 0)
    e1, e2, log, idx = FB.expected(bam, hl, 0, min_q=0)  # (asserts that no later record of a pair is an empty read)
    assert len(idx) >= 3
    open(f"{d}/hl", "wb").write(hl)
    open(f"{d}/x.bam", "wb").write(bam.bam)
    want = _sam(d, bam, "hl", 0, 0)
    r = _filter(d, "--bam", "bam.chr", "hl", "x.bam", "bam", 0, extra=["--bam-exclude", "0"])
    assert r.returncode == 0, r.stderr[-1500:]
    assert _outputs(d, "bam", "bam.chr") == want == [e1, e2, log]
    assert _counts(r)["reads"] == len(bam.records)


def test_a_hash_list_that_hits_nothing(samples, tmp_path):
    bam = samples["Father"][0]
    d = str(tmp_path)
    open(f"{d}/x.bam", "wb").write(bam.bam)
    rng = np.random.default_rng(8)
    kmers = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 25)) for _ in range(4)]
    text = b"|".join(FB.stranded_printed(r)[0] for r in bam.kept())
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    assert not any(km in text or km.translate(comp)[::-1] in text for km in kmers)  # k-mers the file does not hold
    open(f"{d}/hl", "wb").write(b"".join(km + b" 7\n" for km in kmers))
    r = _filter(d, "--bam", "bam.chr", "hl", "x.bam", "bam")
    assert r.returncode == 0, r.stderr[-1500:]
    assert _outputs(d, "bam", "bam.chr") == [b"", b"", bam.chr_log()]
    c = _counts(r)
    assert (c["hits"], c["names"], c["gathered"], c["pairs"]) == (0, 0, 0, 0) and c["reads"] == len(bam.kept())
    assert b"pass 1 done" in r.stderr and b"pass 2 done" not in r.stderr


def test_refusals(samples, tmp_path):
    bam = samples["Father"][0]
    d = str(tmp_path)
    open(f"{d}/f.bam", "wb").write(bam.bam)

    def refused(r, *texts):
        assert r.returncode != 0 and b"--bam" in r.stderr and all(t in r.stderr for t in texts), r.stderr[-1500:]
        assert b"HIP" not in r.stderr and b"memory access" not in r.stderr

    open(f"{d}/plain", "wb").write(bam.sam_text())
    refused(_filter(d, "--bam", "x.chr", HL, "plain", "x"), b"not BGZF")
    open(f"{d}/fq.gz", "wb").write(B.write(b"@r\nACGT\n+\nIIII\n" * 10))
    refused(_filter(d, "--bam", "x.chr", HL, "fq.gz", "x"), b"BAM header")
    with open(f"{d}/f.bam", "rb") as f:  # a pipe
        cat = subprocess.Popen(["cat"], stdin=f, stdout=subprocess.PIPE)
        r = _filter(d, "--bam", "x.chr", HL, "/dev/stdin", "x", stdin=cat.stdout)
        cat.stdout.close()
        cat.wait()
    refused(r, b"not a pipe")
    open(f"{d}/cut.bam", "wb").write(b"".join(B.split(bam.bam)[:10]) + B.EOF)  # (every block boundary lies inside a record)
    refused(_filter(d, "--bam", "x.chr", HL, "cut.bam", "x"), b"inside a record")
    open(f"{d}/torn.bam", "wb").write(bam.bam[:len(bam.bam) // 2])  # the container cut inside a block
    refused(_filter(d, "--bam", "x.chr", HL, "torn.bam", "x"), b"truncated BGZF block")
    refused(_filter(d, "--bam", "x.chr", HL, "f.bam", "x", env={"RUFUS_GPUS": "0,0"}), b"one device")  # (two contexts)
    refused(_filter(d, "--bam", "x.chr", HL, "f.bam", "x", extra=["--bam-what", "1"]), b"unknown argument")
