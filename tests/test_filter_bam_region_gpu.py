"""GPU, through the executables: `RUFUS.Filter --bam CHR HashList Child.bam STUB ... --region 5:177642801-177643000` must
write, byte for byte, the three files `RUFUS.Filter --sam` writes for the SAM text of exactly the records `samtools view -F
3328 Child.bam REGION` prints -- without an index and with one, both passes ranged.  Only the records of the region take
part in the pairing by name: a hit read whose mate lies outside the region pairs with nothing and writes nothing, as behind
the pipe.  Fails without the feature: `--region` is an unknown argument."""
import collections
import copy
import os
import subprocess

import pytest

from tests import bai_ref as X
from tests import bam_ref as R
from tests import filter_bam_ref as FB
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
HL = os.path.join(R.GOLDEN, "Child.k25_c5.HashList")
REGION = "5:177642801-177643000"


def _filter(d, route, chr_file, inp, stub, extra=(), env=None):
    argv = [f"{BIN}/RUFUS.Filter", route, chr_file, HL, inp, stub, str(FB.K), str(FB.MIN_Q), str(FB.THRESH), "4"] + list(extra)
    return subprocess.run(argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _outputs(d, stub, chr_file):
    return [open(os.path.join(d, f), "rb").read() for f in (f"{stub}.Mutations.Mate1.fastq", f"{stub}.Mutations.Mate2.fastq", chr_file)]


def _names(fastq):
    return {line[1:] for line in fastq.split(b"\n")[0::4] if line}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """(Bam, region, --sam's three files over the region's SAM text): once, shared, never changed."""
    d = str(tmp_path_factory.mktemp("filter_region"))
    bam = R.Bam(R.fixture("Child"))
    region = X.parse_region(REGION, [n for n, _ in bam.refs])
    sub = copy.copy(bam)
    sub.records = [r for r in bam.records if X.in_region(r, *region)]
    answers = []
    for tag, b in (("region", sub), ("whole", bam)):
        open(f"{d}/{tag}.sam", "wb").write(b.sam_text())
        r = _filter(d, "--sam", f"{tag}.chr", f"{tag}.sam", tag)
        assert r.returncode == 0, r.stderr[-1500:]
        answers.append(_outputs(d, tag, f"{tag}.chr"))
    want, whole = answers
    assert want[0] and want[1] and want != whole  # something is pulled, and it is not the whole file's answer
    assert want[2] == sub.chr_log()
    # a name the whole file pulls with only ONE mate inside the region: where subset pairing could go wrong
    inside = collections.Counter(FB.qname(r) for r in sub.kept())
    lone = {n for n in _names(whole[0]) if inside.get(n, 0) == 1}
    assert lone and not lone & _names(want[0])
    assert any(inside.get(n, 0) == 2 for n in _names(want[0]))  # ... and pairs with both mates inside
    return bam, region, want


@pytest.mark.parametrize("arena", [None, "1048576"])
@pytest.mark.parametrize("index", [None, "fine", "coarse"])
def test_filter_region_equals_filter_sam_of_the_region(reference, tmp_path, index, arena):
    bam, region, want = reference
    d = str(tmp_path)
    open(f"{d}/X.bam", "wb").write(bam.bam)
    if index:
        open(f"{d}/X.bam.bai", "wb").write(X.build(bam, index, "same" if index == "fine" else "next"))
    r = _filter(d, "--bam", "bam.chr", "X.bam", "bam", extra=["--region", REGION], env={"RFX_BAM_ARENA": arena} if arena else None)
    assert r.returncode == 0, r.stderr[-1500:]
    assert _outputs(d, "bam", "bam.chr") == want
    err = r.stderr.decode()
    assert err.count("has no .bai index") == (1 if index is None else 0)  # one line, not one per pass
    assert "pass 2 done" in err and "index %s:" % ("used" if index else "none") in err
    assert "%d records in the region" % sum(X.in_region(x, *region) for x in bam.records) in err


def test_refusals(reference, tmp_path):
    bam = reference[0]
    d = str(tmp_path)
    open(f"{d}/X.bam", "wb").write(bam.bam)
    for extra, message in ((["--region", "5:1-2", "--region", "5:3-4"], b"given twice"), (["--region", "55:1-2"], b"region '55:1-2'"),
                           (["--region", "5:9-1"], b"region '5:9-1'"), (["--region"], b"unknown argument")):
        r = _filter(d, "--bam", "bam.chr", "X.bam", "bam", extra=extra)
        assert r.returncode != 0 and message in r.stderr, (extra, r.stderr[-1500:])
    argv = [f"{BIN}/RUFUS.Filter", "--packed", "no.cache", "p.chr", HL, "X.bam", "p", str(FB.K), str(FB.MIN_Q), str(FB.THRESH), "4",
            "--region", REGION]
    r = subprocess.run(argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    assert r.returncode != 0 and b"does not record a region" in r.stderr, r.stderr[-1500:]
