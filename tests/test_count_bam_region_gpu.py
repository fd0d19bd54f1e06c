"""GPU, through the executable: `jellyfish count --bam CHR --region REG X.bam` against `jellyfish count --sam CHR2` over the
SAM text of exactly the records `samtools view -F 3328 X.bam REG` prints (tests/bai_ref.py in_region over tests/bam_ref.py's
reader) and against the oracle's count of their SEQ strings; the chromosome logs must be the same bytes.  Every file runs
without an index (the whole file is walked, the device decides), with a fine index (X.bam.bai) and with a coarse one
(X.bai), with 1 GiB arenas and with RFX_BAM_ARENA=1048576.  On the sorted synthetic file: a whole reference, NAME:BEG, a
region that holds nothing, the blocks the trace says were inflated against the index's range, the refusals, a damaged
index.  Fails without the feature: `--region` does not exist."""
import copy
import hashlib
import os
import re
import subprocess

import pytest

import oracle
from tests import bai_ref as X
from tests import bam_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
SAMPLES = ("Child", "Mother", "Father")
REGION = "5:177640001-177645000"
# file: (kept records, of them in REGION, of those starting in front of BEG) -- counted on the CPU
FIGURES = {"Child": (4094, 1307, 35), "Mother": (4030, 1243, 46), "Father": (3278, 961, 30)}


def _count(d, out, inputs, extra=(), env=None):
    argv = [f"{BIN}/jellyfish", "count", "--disk", "-m", "25", "-L", "2", "-s", "100M", "-t", "6", "-o", out, "-C"] + list(extra) + \
           list(inputs)
    return subprocess.run(argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _payload_sha(path):
    blob = open(path, "rb").read()
    return hashlib.sha256(blob[9 + int(blob[:9]):]).hexdigest()


def _subset(bam, region):
    """The Bam with only the records of the region: what `samtools view X.bam REGION` leaves of it."""
    sub = copy.copy(bam)
    sub.records = [r for r in bam.records if X.in_region(r, *region)]
    return sub


def _sam_reference(d, tag, sub):
    """(payload sha256, chromosome log) of `jellyfish count --sam` over the subset's SAM text."""
    open(f"{d}/{tag}.sam", "wb").write(sub.sam_text())
    r = _count(d, f"{tag}.sam.Jhash", [f"{tag}.sam"], extra=["--sam", f"{tag}.chr2"])
    assert r.returncode == 0, r.stderr
    log = open(f"{d}/{tag}.chr2", "rb").read()
    assert log == sub.chr_log()
    return _payload_sha(f"{d}/{tag}.sam.Jhash"), log


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> (Bam, region, --sam's payload sha256, its log): computed once, shared, never changed."""
    d = str(tmp_path_factory.mktemp("region_sam"))
    out = {}
    for name in SAMPLES:
        bam = R.Bam(R.fixture(name))
        region = X.parse_region(REGION, [n for n, _ in bam.refs])
        sub = _subset(bam, region)
        kept = sub.kept()
        assert (len(bam.kept()), len(kept), sum(r["pos"] < region[1] for r in kept)) == FIGURES[name]
        assert any(op == "D" for r in kept for op, _ in r["cigar"])
        sha, log = _sam_reference(d, name, sub)
        fastq = b"".join(b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for s in sub.kept_seqs())
        assert sha == hashlib.sha256(oracle.count([fastq], 25, 100_000_000, lower=2, canonical=True).payload()).hexdigest()
        out[name] = (bam, region, sha, log)
    return out


@pytest.fixture(scope="module")
def synthetic():
    return R.Bam(X.sorted_bam())


def _put(d, bam, index):
    """X.bam and its index: "fine" as X.bam.bai, "coarse" as X.bai (the second name that is tried), None: no index."""
    open(f"{d}/X.bam", "wb").write(bam.bam)
    if index == "fine":
        open(f"{d}/X.bam.bai", "wb").write(X.build(bam, "fine", "next"))
    elif index == "coarse":
        open(f"{d}/X.bai", "wb").write(X.build(bam, "coarse", "same"))


def _inflated(r):
    return int(re.search(r"(\d+) blocks inflated", r.stderr.decode()).group(1))


@pytest.mark.parametrize("arena", [None, "1048576"])
@pytest.mark.parametrize("index", [None, "fine", "coarse"])
@pytest.mark.parametrize("name", SAMPLES)
def test_region_equals_sam_of_the_region_and_the_oracle(reference, tmp_path, name, index, arena):
    bam, region, sam_sha, sam_log = reference[name]
    d = str(tmp_path)
    _put(d, bam, index)
    r = _count(d, "x.Jhash", ["X.bam"], extra=["--bam", "x.chr", "--region", REGION], env={"RFX_BAM_ARENA": arena} if arena else None)
    assert r.returncode == 0, r.stderr
    assert _payload_sha(f"{d}/x.Jhash") == sam_sha
    assert open(f"{d}/x.chr", "rb").read() == sam_log
    err = r.stderr.decode()
    assert ("has no .bai index" in err) == (index is None) and "not a usable" not in err
    assert "index %s:" % ("used" if index else "none") in err
    assert "%d records in the region" % sum(X.in_region(x, *region) for x in bam.records) in err
    n_blocks = len(bam.block_starts)
    if index is None:
        assert _inflated(r) == n_blocks  # (the header lies in the first block, the EOF marker is the last)
    else:
        q = X.query(X.parse(X.build(bam, index)), *region)
        assert _inflated(r) == X.blocks_between(bam, *q) <= n_blocks


@pytest.mark.parametrize("text", ["chrB:1", "chrA:2,900,000", "chrA:500001-510000", "chrC:10000000-10001000", "chrC:39,990"])
@pytest.mark.parametrize("index", [None, "fine", "coarse"])
def test_synthetic_regions(synthetic, tmp_path, text, index):
    bam = synthetic
    d = str(tmp_path)
    region = X.parse_region(text, [n for n, _ in bam.refs])
    sub = _subset(bam, region)
    sam_sha, sam_log = _sam_reference(d, "ref", sub)
    if text.startswith("chrC:1000"):
        assert not sub.records and sam_log == b"notachr\n"  # nothing: the outputs of an empty input
    else:
        assert sub.kept() and len(sub.records) < len(bam.records)
    _put(d, bam, index)
    r = _count(d, "x.Jhash", ["X.bam"], extra=["--bam", "x.chr", "--region", text], env={"RFX_BAM_ARENA": "1048576"})
    assert r.returncode == 0, r.stderr
    assert _payload_sha(f"{d}/x.Jhash") == sam_sha
    assert open(f"{d}/x.chr", "rb").read() == sam_log
    if index:
        q = X.query(X.parse(X.build(bam, index)), *region)
        want = 0 if q is None else X.blocks_between(bam, *q)
        assert _inflated(r) == want
        if index == "fine" and text == "chrA:500001-510000":
            assert 0 < want < len(bam.block_starts) / 4  # the index was used: a fraction of the file was inflated


def test_refusals(synthetic, tmp_path):
    d = str(tmp_path)
    _put(d, synthetic, "fine")
    open(f"{d}/Y.bam", "wb").write(synthetic.bam)
    open(f"{d}/x.sam", "wb").write(_subset(synthetic, (0, 0, 1000)).sam_text())
    cases = [(["--sam", "s.chr", "--region", "chrA"], ["x.sam"], b"--region goes with --bam"),
             (["--region", "chrA"], ["X.bam"], b"--region goes with --bam"),
             (["--bam", "x.chr", "--region", "chrA", "--keep-packed", "kp"], ["X.bam"], b"does not record a region"),
             (["--bam", "x.chr", "--region", "chrA", "--region", "chrC"], ["X.bam"], b"given twice"),
             (["--bam", "x.chr", "--region", "chrA"], ["X.bam", "Y.bam"], b"ONE input"),
             (["--bam", "x.chr", "--region", "chrD:5"], ["X.bam"], b"region 'chrD:5'"),
             (["--bam", "x.chr", "--region", "chrA:0-5"], ["X.bam"], b"region 'chrA:0-5'"),
             (["--bam", "x.chr", "--region", "chrA:9-5"], ["X.bam"], b"region 'chrA:9-5'"),
             (["--bam", "x.chr", "--region", "chrA:5-9x"], ["X.bam"], b"region 'chrA:5-9x'")]
    for extra, inputs, message in cases:
        r = _count(d, "x.Jhash", inputs, extra=extra)
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr)


@pytest.mark.parametrize("damage", ["magic", "n_ref", "truncated", "chunk", "block"])
def test_a_damaged_index_is_named_and_not_used(synthetic, tmp_path, damage):
    bam = synthetic
    d = str(tmp_path)
    text = "chrA:500001-510000"
    region = X.parse_region(text, [n for n, _ in bam.refs])
    sam_sha, sam_log = _sam_reference(d, "ref", _subset(bam, region))
    _put(d, bam, None)
    bai = bytearray(X.build(bam, "fine"))
    if damage == "magic":
        bai[3] = 2
    elif damage == "n_ref":
        bai[4] += 1
    elif damage == "truncated":
        bai = bai[:len(bai) // 2]
    elif damage == "chunk":  # reference 0, its first bin's first chunk: an end beyond the file
        bai[8 + 4 + 8 + 8:8 + 4 + 8 + 16] = (len(bam.bam) << 16).to_bytes(8, "little")
    else:  # the index of the same records in another block layout: sound as an index, but its chunks begin at no block of X.bam
        bai = X.build(R.Bam(X.sorted_bam(cut=4000)), "fine")
    open(f"{d}/X.bam.bai", "wb").write(bytes(bai))
    r = _count(d, "x.Jhash", ["X.bam"], extra=["--bam", "x.chr", "--region", text])
    assert r.returncode == 0, r.stderr
    assert r.stderr.count(b"is not a usable BAM index") == 1, r.stderr
    assert _inflated(r) == len(bam.block_starts)  # the whole file was walked
    assert _payload_sha(f"{d}/x.Jhash") == sam_sha
    assert open(f"{d}/x.chr", "rb").read() == sam_log
