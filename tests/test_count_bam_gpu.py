"""GPU, through the executable: `jellyfish count --bam CHR X.bam` on the three testRun BAMs, with 1 GiB arenas and with
RFX_BAM_ARENA=1048576 (the 1.6 MB of a file then cross arenas), against `jellyfish count --sam CHR2` over the SAM text
tests/bam_ref.py's reader makes of the same file and against the oracle's count of the reader's SEQ strings; the two
chromosome logs must be the same bytes.  Fails without the feature: `--bam` does not exist."""
import hashlib
import os
import subprocess

import pytest

import oracle
from tests import bam_ref as R
from tests import bgzf_ref as B
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
SAMPLES = ("Child", "Mother", "Father")


def _count(d, out, inputs, k=25, canonical=True, extra=(), env=None):
    argv = [f"{BIN}/jellyfish", "count", "--disk", "-m", str(k), "-L", "2", "-s", "100M", "-t", "6", "-o", out] + \
           (["-C"] if canonical else []) + list(extra) + list(inputs)
    return subprocess.run(argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _payload_sha(path):
    blob = open(path, "rb").read()
    return hashlib.sha256(blob[9 + int(blob[:9]):]).hexdigest()


def _oracle_sha(bam, k=25, canonical=True):
    fastq = b"".join(b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for s in bam.kept_seqs())
    return hashlib.sha256(oracle.count([fastq], k, 100_000_000, lower=2, canonical=canonical).payload()).hexdigest()


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> (Bam, payload sha256 of --sam over the reader's SAM text, its chromosome log, the oracle's sha256): once."""
    d = tmp_path_factory.mktemp("bam_sam")
    out = {}
    for name in SAMPLES:
        bam = R.Bam(R.fixture(name))
        (d / f"{name}.sam").write_bytes(bam.sam_text())
        r = _count(str(d), f"{name}.sam.Jhash", [f"{name}.sam"], extra=["--sam", f"{name}.chr2"])
        assert r.returncode == 0, r.stderr
        log = (d / f"{name}.chr2").read_bytes()
        assert log == bam.chr_log()  # the reader's own idea of src/PassThroughSamCheck.cpp:140-155
        out[name] = (bam, _payload_sha(str(d / f"{name}.sam.Jhash")), log, _oracle_sha(bam))
    return out


@pytest.mark.parametrize("arena", [None, "1048576"])
@pytest.mark.parametrize("name", SAMPLES)
def test_count_bam_equals_count_sam_and_the_oracle(reference, tmp_path, name, arena):
    bam, sam_sha, sam_log, oracle_sha = reference[name]
    d = str(tmp_path)
    open(f"{d}/{name}.bam", "wb").write(bam.bam)
    r = _count(d, "x.Jhash", [f"{name}.bam"], extra=["--bam", "x.chr"], env={"RFX_BAM_ARENA": arena} if arena else None)
    assert r.returncode == 0, r.stderr
    assert sam_sha == oracle_sha
    assert _payload_sha(f"{d}/x.Jhash") == sam_sha
    assert open(f"{d}/x.chr", "rb").read() == sam_log
    trace = r.stderr.decode()
    counts = trace[trace.index("bam route: "):].split()
    n_arenas, n_records, n_reads = int(counts[7]), int(counts[9]), int(counts[11])
    assert (n_records, n_reads) == (len(bam.records), len(bam.kept()))
    assert n_arenas == 1 if arena is None else n_arenas >= 2


@pytest.mark.parametrize("k,canonical", [(31, True), (25, False)])
def test_count_bam_other_k_and_not_canonical(reference, tmp_path, k, canonical):
    bam = reference["Father"][0]
    d = str(tmp_path)
    open(f"{d}/f.bam", "wb").write(bam.bam)
    r = _count(d, "x.Jhash", ["f.bam"], k=k, canonical=canonical, extra=["--bam", "x.chr"], env={"RFX_BAM_ARENA": "1048576"})
    assert r.returncode == 0, r.stderr
    assert _payload_sha(f"{d}/x.Jhash") == _oracle_sha(bam, k, canonical)


def test_count_bam_exclude_flags(reference, tmp_path):
    bam = reference["Child"][0]
    d = str(tmp_path)
    open(f"{d}/c.bam", "wb").write(bam.bam)
    r = _count(d, "x.Jhash", ["c.bam"], extra=["--bam", "x.chr", "--bam-exclude", "0"])
    assert r.returncode == 0, r.stderr
    fastq = b"".join(b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for s in bam.kept_seqs(0))
    assert _payload_sha(f"{d}/x.Jhash") == hashlib.sha256(oracle.count([fastq], 25, 100_000_000, lower=2).payload()).hexdigest()
    assert open(f"{d}/x.chr", "rb").read() == bam.chr_log(0)


def test_refusals(reference, tmp_path):
    bam = reference["Father"][0]
    d = str(tmp_path)
    open(f"{d}/f.bam", "wb").write(bam.bam)
    r = _count(d, "x.Jhash", ["f.bam"])  # a BAM without --bam: the message says --bam, not FASTQ
    assert r.returncode != 0 and b"--bam" in r.stderr and b"FASTQ" not in r.stderr, r.stderr
    for extra in (["--sam", "s.chr"], ["--spool", "sp"], ["--sam", "s.chr", "--keep-packed", "kp"]):
        r = _count(d, "x.Jhash", ["f.bam"], extra=["--bam", "x.chr"] + extra)
        assert r.returncode != 0 and b"--bam" in r.stderr and b"one device" in r.stderr, (extra, r.stderr)
    r = _count(d, "x.Jhash", ["f.bam"], extra=["--bam", "x.chr"], env={"RUFUS_GPUS": "0,0"})  # (a device named twice: two contexts)
    assert r.returncode != 0 and b"one device" in r.stderr, r.stderr
    with open(f"{d}/f.bam", "rb") as f:  # a pipe
        cat = subprocess.Popen(["cat"], stdin=f, stdout=subprocess.PIPE)
        r = subprocess.run([f"{BIN}/jellyfish", "count", "-m", "25", "-s", "100M", "-t", "6", "-o", "x.Jhash", "--bam", "x.chr",
                            "/dev/stdin"], cwd=d, stdin=cat.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        cat.stdout.close()
        cat.wait()
    assert r.returncode != 0 and b"not a pipe" in r.stderr, r.stderr
    open(f"{d}/fq.gz", "wb").write(B.write(b"@r\nACGT\n+\nIIII\n" * 10))
    r = _count(d, "x.Jhash", ["fq.gz"], extra=["--bam", "x.chr"])
    assert r.returncode != 0 and b"BAM header" in r.stderr, r.stderr
    open(f"{d}/cut.bam", "wb").write(b"".join(B.split(bam.bam)[:10]) + B.EOF)  # (every block boundary lies inside a record)
    r = _count(d, "x.Jhash", ["cut.bam"], extra=["--bam", "x.chr"])
    assert r.returncode != 0 and b"inside a record" in r.stderr, r.stderr
