"""GPU, through the executables: `RUFUS.Filter.single --bam CHR HashList X.bam STUB K MinQ Threshold Threads` must write, byte
for byte, STUB.Mutations.fastq and CHR as `samtools view -F N X.bam [REG] | PassThroughSamCheck.stranded.se CHR |
RUFUS.Filter.single HashList stdin STUB K MinQ Threshold 1` writes them (runRufus.sh:1031-1032).  Three statements of that
are held against each other: the Python statement of tests/filter_single_ref.py (pinned to the reference's binaries by
tests/test_filter_single_host.py), `RUFUS.Filter.single --sam` over tests/bam_ref.py's SAM text, and this project's own two
text processes -- on the three testRun BAMs (and the golden values the reference binaries made of them), on the crafted file
of tests/filter_single_ref.py, on bam_ref.synthetic() with every record kept, with a region; with 1 GiB arenas and with
RFX_BAM_ARENA=1048576.  Fails without the feature: `--bam` is read as the hash list's path."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bai_ref as X
from tests import bam_ref as R
from tests import bgzf_ref as B
from tests import filter_bam_ref as FB
from tests import filter_single_ref as S
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
HL = os.path.join(R.GOLDEN, "Child.k25_c5.HashList")
TRACE = re.compile(r"bam single route: arenas (\d+) records (\d+) reads (\d+) selected (\d+) windows (\d+)")
SMALL = {"RFX_BAM_ARENA": "1048576"}


def _single(d, route, chr_file, hl, inp, stub, min_q=S.MIN_Q, thresh=1, threads=4, extra=(), env=None, stdin=None):
    argv = [f"{BIN}/RUFUS.Filter.single", route, chr_file, hl, inp, stub, str(S.K), str(min_q), str(thresh), str(threads)] + list(extra)
    return subprocess.run(argv, cwd=d, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _outputs(d, stub, chr_file):
    return open(os.path.join(d, f"{stub}.Mutations.fastq"), "rb").read(), open(os.path.join(d, chr_file), "rb").read()


def _bam(d, blob, hl, stub="bam", **kw):
    """(the two files, the trace's counts, stderr) of `--bam` over the file's bytes."""
    open(f"{d}/x.bam", "wb").write(blob)
    r = _single(d, "--bam", f"{stub}.chr", hl, "x.bam", stub, **kw)
    assert r.returncode == 0, r.stderr[-1500:]
    m = TRACE.search(r.stderr.decode())
    assert m, r.stderr[-1500:]
    assert b"pass 1 done" in r.stderr and b"pass 2" not in r.stderr
    assert not os.path.exists(f"{d}/{stub}.Mutations.Mate1.fastq")
    return _outputs(d, stub, f"{stub}.chr"), dict(zip(("arenas", "records", "reads", "selected", "windows"), map(int, m.groups()))), r.stderr


def _sam(d, bam, hl, exclude=3328, **kw):
    open(f"{d}/x.sam", "wb").write(bam.sam_text(exclude))
    r = _single(d, "--sam", "sam.chr", hl, "x.sam", "sam", **kw)
    assert r.returncode == 0, r.stderr[-1500:]
    return _outputs(d, "sam", "sam.chr")


def _two_processes(d, bam, hl, min_q=S.MIN_Q, thresh=1):
    """The text route: this project's feeder and its RUFUS.Filter.single on stdin (every line ends with an aux field, as
    samtools view's do: the feeders walk off a line that ends with QUAL)."""
    sam = b"".join(ln + b"\tXS:i:0\n" for ln in bam.sam_text().split(b"\n") if ln)
    fq = subprocess.run([f"{BIN}/PassThroughSamCheck.stranded.se", "two.chr"], input=sam, cwd=d, stdout=subprocess.PIPE, check=True,
                        timeout=180).stdout
    r = subprocess.run([f"{BIN}/RUFUS.Filter.single", hl, "stdin", "two", str(S.K), str(min_q), str(thresh), "2"], input=fq, cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    assert r.returncode == 0, r.stderr[-1500:]
    return _outputs(d, "two", "two.chr")


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    """name -> (Bam, the Python statement, --sam's two files, the two text processes' two files): once, shared."""
    out, hl = {}, open(HL, "rb").read()
    for name in ("Child", "Mother", "Father"):
        bam = R.Bam(R.fixture(name))
        d = str(tmp_path_factory.mktemp("single_" + name))
        out[name] = (bam, S.expected_single(bam, hl), _sam(d, bam, HL), _two_processes(d, bam, HL))
    return out


@pytest.mark.parametrize("arena", [None, "1048576"])
@pytest.mark.parametrize("name", ["Child", "Mother", "Father"])
def test_the_fixtures(samples, tmp_path, name, arena):
    bam, (text, log, idx, hits), sam, two = samples[name]
    got, c, _ = _bam(str(tmp_path), bam.bam, HL, env={"RFX_BAM_ARENA": arena} if arena else None)
    assert got == sam == two == (text, log) and log == bam.chr_log()
    golden = json.load(open(os.path.join(R.GOLDEN, "expected_single_bam.json")))[name]
    assert (hashlib.sha256(got[0]).hexdigest(), hashlib.sha256(got[1]).hexdigest()) == (golden["fastq_sha256"], golden["chr_sha256"])
    heads = got[0].split(b"\n")[0::4][:-1]
    assert [h[1:].rsplit(b":MH", 1)[0].decode() for h in heads] == golden["names"]
    assert [int(h.rsplit(b":MH", 1)[1]) for h in heads] == golden["mh"]
    assert (c["records"], c["reads"]) == (len(bam.records), len(bam.kept()))
    assert c["arenas"] == 1 if arena is None else c["arenas"] >= 2
    assert c["selected"] == got[0].count(b"\n") // 4 == len(idx) and c["windows"] == sum(hits[i] for i in idx)
    if name == "Child":
        assert c["selected"] >= 26


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    blob, hl, _ = S.crafted_single()
    bam = R.Bam(blob)
    d = tmp_path_factory.mktemp("single_crafted")
    (d / "hl").write_bytes(hl)
    want = {t: S.expected_single(bam, hl, thresh=t) for t in (1, 2)}
    sam = {t: _sam(str(d), bam, str(d / "hl"), thresh=t) for t in (1, 2)}
    # the text route refuses an empty sequence line: it sees the clean subset, where the statement must hold as well
    clean = R.Bam(S.clean_subset(bam))
    two = {t: (_two_processes(str(d), clean, str(d / "hl"), thresh=t), S.expected_single(clean, hl, thresh=t)[:2]) for t in (1, 2)}
    return bam, str(d / "hl"), want, sam, clean, two


@pytest.mark.parametrize("thresh", [1, 2])
@pytest.mark.parametrize("threads", [1, 5])
@pytest.mark.parametrize("arena", [None, "1048576"])
def test_the_crafted_file(crafted, tmp_path, arena, threads, thresh):
    bam, hl, want, sam, clean, two = crafted
    text, log, idx, hits = want[thresh]
    env = {"RFX_BAM_ARENA": arena} if arena else None
    got, c, _ = _bam(str(tmp_path), bam.bam, hl, thresh=thresh, threads=threads, env=env)
    assert got == sam[thresh] == (text, log)
    assert (c["arenas"] >= 2) == (arena is not None) and c["selected"] == len(idx) and c["windows"] == sum(hits[i] for i in idx)
    assert (c["records"], c["reads"]) == (len(bam.records), len(bam.kept()))
    if threads == 1:
        got_clean, _, _ = _bam(str(tmp_path), clean.bam, hl, stub="clean", thresh=thresh, env=env)
        assert got_clean == two[thresh][0] == two[thresh][1]


def test_bam_exclude_0_on_the_synthetic_file(tmp_path):
    bam = R.Bam(R.synthetic())
    d = str(tmp_path)
    # its own hash list, and windows of a duplicate-flagged read: kept only because nothing is excluded
    dup = [FB.stranded_printed(r)[0] for r in bam.records if r["flag"] & 1024]
    dup = [s for s in dup if len(s) >= 60 and set(s) <= set(b"ACGT")][:2]
    assert len(dup) == 2
    hl = FB.own_hash_list(bam, 0) + b"".join(s[i:i + S.K] + b" 9\n" for s in dup for i in range(0, len(s) - S.K + 1, 5))
    text, log, idx, hits = S.expected_single(bam, hl, 0, min_q=0)
    kept = bam.kept(0)
    assert len(idx) >= 5 and any(kept[i]["flag"] & 1024 for i in idx) and len(kept) == len(bam.records)
    open(f"{d}/hl", "wb").write(hl)
    sam = _sam(d, bam, "hl", 0, min_q=0)
    got, c, _ = _bam(d, bam.bam, "hl", min_q=0, extra=["--bam-exclude", "0"])
    assert got == sam == (text, log) and c["reads"] == len(bam.records)
    # ... and with the default flags those records are gone
    got, c, _ = _bam(d, bam.bam, "hl", stub="dflt", min_q=0)
    assert got == S.expected_single(bam, hl, min_q=0)[:2] and c["reads"] == len(bam.kept()) < len(bam.records)


@pytest.mark.parametrize("arena", [None, "1048576"])
@pytest.mark.parametrize("index", [None, "fine"])
def test_region_with_and_without_an_index(crafted, tmp_path, index, arena):
    bam, hl = crafted[0], crafted[1]
    text_region = "chr2:1200-1500"
    region = X.parse_region(text_region, [n for n, _ in bam.refs])
    inside = [r for r in bam.kept() if X.in_region(r, *region)]
    want = S.expected_single(bam, open(hl, "rb").read(), records=inside)
    assert 300 <= len(inside) <= 600 and len(want[2]) >= 30 and want[1] == b"notachr\nchr2\n"
    d = str(tmp_path)
    if index:
        open(f"{d}/x.bam.bai", "wb").write(X.build(bam, index, "next"))
    got, c, err = _bam(d, bam.bam, hl, extra=["--region", text_region], env={"RFX_BAM_ARENA": arena} if arena else None)
    assert got == want[:2] and c["reads"] == len(inside) and c["selected"] == len(want[2])
    assert (b"has no .bai index" in err) == (index is None) and b"not a usable" not in err
    assert (b"index used" in err) == (index is not None)
    if index:
        assert c["records"] < len(bam.records)  # only the index's range was inflated


def test_edge_cases_and_refusals(samples, tmp_path):
    bam = samples["Father"][0]
    d = str(tmp_path)
    # a hash list that hits nothing: an empty file, the whole log
    rng = np.random.default_rng(8)
    kmers = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 25)) for _ in range(4)]
    text = b"|".join(FB.stranded_printed(r)[0] for r in bam.kept())
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    assert not any(km in text or km.translate(comp)[::-1] in text for km in kmers)
    open(f"{d}/none", "wb").write(b"".join(km + b" 7\n" for km in kmers))
    got, c, _ = _bam(d, bam.bam, "none")
    assert got == (b"", bam.chr_log()) and (c["selected"], c["windows"], c["reads"]) == (0, 0, len(bam.kept()))
    # Threshold 0 (and below) on a 129-record file: every kept record is written, the `*` of the reverse strand as an empty line
    plant, hl = S.make_plant(200, 3)
    recs = S.planted_records(126, range(0, 126, 9), plant) + [R.record(b"star_rev", 16, 2, 500), R.record(b"star_fwd", 0, 2, 501),
                                                              R.record(b"dup", 1024, 2, 502, [("M", 4)], "ACGT", bytes([30] * 4))]
    small = R.Bam(R.write(R.REFS, recs))
    assert len(small.records) == 129 and len(small.kept()) == 128
    open(f"{d}/hl129", "wb").write(hl)
    for thresh in (0, -1):
        want = S.expected_single(small, hl, thresh=thresh)
        assert len(want[2]) == 128 and b":MH0\n" in want[0] and b"@star_rev:MH0\n\n+\n*\n" in want[0]
        got, c, _ = _bam(d, small.bam, "hl129", stub="t%d" % (thresh + 1), thresh=thresh)
        assert got == want[:2] and c["selected"] == 128
    # refusals, one line each, before the device does anything
    open(f"{d}/f.bam", "wb").write(bam.bam)

    def refused(r, *texts):
        assert r.returncode != 0 and all(t in r.stderr for t in texts), r.stderr[-1500:]
        assert b"RUFUS.Filter.single" in r.stderr and b"HIP" not in r.stderr and b"memory access" not in r.stderr

    with open(f"{d}/f.bam", "rb") as f:  # a pipe
        cat = subprocess.Popen(["cat"], stdin=f, stdout=subprocess.PIPE)
        r = _single(d, "--bam", "x.chr", HL, "/dev/stdin", "x", stdin=cat.stdout)
        cat.stdout.close()
        cat.wait()
    refused(r, b"--bam", b"not a pipe")
    open(f"{d}/fq.gz", "wb").write(B.write(b"@r\nACGT\n+\nIIII\n" * 10))
    refused(_single(d, "--bam", "x.chr", HL, "fq.gz", "x"), b"--bam", b"BAM header")
    refused(_single(d, "--bam", "x.chr", HL, "f.bam", "x", env={"RUFUS_GPUS": "0,0"}), b"--bam", b"one device")
    refused(_single(d, "--bam", "x.chr", HL, "f.bam", "x", extra=["--region", "chr1", "--region", "chr2"]), b"--bam", b"given twice")
    refused(_single(d, "--bam", "x.chr", HL, "f.bam", "x", extra=["--bam-what", "1"]), b"--bam", b"unknown argument")
    refused(_single(d, "--packed", "cache", HL, "f.bam", "x"), b"--packed", b"paired")
