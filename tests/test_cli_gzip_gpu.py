"""GPU: `jellyfish count` on plain-gzip FASTQ -- what a sequencer or an archive hands out, and what runRufus.sh feeds
through `zcat` (runRufus.sh:157-160) -- inflated on the device (rfx_ingest.hpp GzipIngest; rufus_amd/csrc/rfx_gzip.hip).
The route is the default (RFX_GZIP_DEVICE=0 turns it off).  The testRun mates are
recompressed by Python's gzip (an FNAME header, no `BC` subfield: not BGZF); payload and histogram must be the text route's
and tests/golden/testRun/expected.json's."""
import gzip
import hashlib
import io
import os
import subprocess

import pytest

from tests import bgzf_ref as B
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")


def plain_gzip(text: bytes, name: str, level=6) -> bytes:
    buf = io.BytesIO()
    with gzip.GzipFile(filename=name, mode="wb", compresslevel=level, fileobj=buf, mtime=0) as f:
        f.write(text)
    blob = buf.getvalue()
    assert blob[:4] == b"\x1f\x8b\x08\x08"  # FNAME and nothing else: plain gzip
    return blob


def count(d, out, inputs, extra=(), env=None, stdin=None):
    return subprocess.run([f"{BIN}/jellyfish", "count", "-m", "25", "-C", "-s", "100M", "-L", "2", "-t", "6", "-o", out, *extra, *inputs],
                          cwd=d, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env={**os.environ, "RFX_CLI_TRACE": "1", **(env or {})})


def payload_sha(path):
    blob = open(path, "rb").read()
    return hashlib.sha256(blob[9 + int(blob[:9]):]).hexdigest()


def histo(d, jhash):
    r = subprocess.run([f"{BIN}/jellyfish", "histo", "-f", jhash], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("env", [None, {"RFX_GZIP_CHUNK": "4096", "RFX_INGEST_PIECE": "70000", "RFX_GZIP_ARENA": str(1 << 20)}])
def test_jellyfish_count_reads_plain_gzip_fastq(testrun, tmp_path, env):
    d = str(tmp_path)
    m1, m2 = testrun["Child"]
    open(f"{d}/m1.fastq", "wb").write(m1)
    open(f"{d}/m2.fastq", "wb").write(m2)
    open(f"{d}/m1.fastq.gz", "wb").write(plain_gzip(m1, "Child.mate1.fastq"))
    open(f"{d}/m2.fastq.gz", "wb").write(plain_gzip(m2, "Child.mate2.fastq", 9))
    open(f"{d}/both.fastq.gz", "wb").write(plain_gzip(m1, "Child.mate1.fastq", 1) + plain_gzip(m2, "Child.mate2.fastq"))
    r = count(d, "text.Jhash", ["m1.fastq", "m2.fastq"])
    assert r.returncode == 0 and b"gzip route" not in r.stderr, r.stderr
    want = testrun["expected"]["samples"]["Child"]["s100M"]
    assert payload_sha(f"{d}/text.Jhash") == want["payload_sha256"]
    for out, inputs, members in (("two.Jhash", ["m1.fastq.gz", "m2.fastq.gz"], 2), ("cat.Jhash", ["both.fastq.gz"], 2)):
        r = count(d, out, inputs, env=env)
        assert r.returncode == 0, r.stderr
        assert payload_sha(f"{d}/{out}") == want["payload_sha256"], out
        h = histo(d, out)
        assert h == histo(d, "text.Jhash") and hashlib.md5(h).hexdigest() == want["histo_full_md5"], out
        trace = r.stderr.decode()
        assert "count: gzip route, text arenas open" in trace and "bgzf route" not in trace
        last = trace[trace.rindex("gzip route: "):]
        assert f"members {members}," in last and f"bytes {len(m1) + len(m2)}" in last, last
        if env:  # small chunks, small pieces, arenas of 1 MiB: many chunks, several arenas
            assert int(last.split("confirmed ")[1].split(",")[0]) > 10 and int(last.split(" arenas")[0].split()[-1]) >= 2, last


def test_bgzf_keeps_its_route_and_the_variable_turns_the_gzip_route_off(testrun, tmp_path):
    d = str(tmp_path)
    m1 = testrun["Child"][0]
    open(f"{d}/b.fastq.gz", "wb").write(B.write(m1))
    r = count(d, "b.Jhash", ["b.fastq.gz"])
    assert r.returncode == 0 and b"bgzf route" in r.stderr and b"gzip route" not in r.stderr, r.stderr
    open(f"{d}/g.fastq.gz", "wb").write(plain_gzip(m1, "Child.mate1.fastq"))
    r = count(d, "g.Jhash", ["g.fastq.gz"])
    assert r.returncode == 0 and payload_sha(f"{d}/g.Jhash") == payload_sha(f"{d}/b.Jhash"), r.stderr
    r = count(d, "off.Jhash", ["g.fastq.gz"], env={"RFX_GZIP_DEVICE": "0"})
    assert b"gzip route" not in r.stderr


def test_jellyfish_count_refuses_what_the_gzip_route_cannot_take(testrun, tmp_path):
    d = str(tmp_path)
    m1 = testrun["Child"][0]
    good = plain_gzip(m1, "Child.mate1.fastq")
    open(f"{d}/g.fastq.gz", "wb").write(good)
    open(f"{d}/ref.fa.gz", "wb").write(plain_gzip(b">chr1\n" + b"ACGTTGCAAC" * 500 + b"\n", "ref.fa"))
    r = count(d, "x.Jhash", ["ref.fa.gz"])
    assert r.returncode == 1 and b"is plain gzip and its first inflated byte is not '@'" in r.stderr and b"zcat" in r.stderr, r.stderr
    r = count(d, "x.Jhash", ["g.fastq.gz"], extra=["--sam", "s.chr", "--keep-packed", "kept.bin"])
    assert r.returncode == 1 and b"plain-gzip input is inflated on the device, which needs one device and none of --sam, --spool, " \
        b"--keep-packed" in r.stderr, r.stderr
    p = subprocess.Popen(["bash", "-c", f"cat g.fastq.gz | {BIN}/jellyfish count -m 25 -C -s 100M -L 2 -t 6 -o x.Jhash /dev/stdin"],
                         cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    _, err = p.communicate(timeout=120)
    assert p.returncode == 1 and b"gzip input needs a regular file, not a pipe" in err, err
    # a damaged file is refused with the decoder's text
    blob = bytearray(good)
    blob[len(blob) // 2] ^= 0x5A
    open(f"{d}/flip.fastq.gz", "wb").write(bytes(blob))
    r = count(d, "x.Jhash", ["flip.fastq.gz"])
    assert r.returncode != 0 and b"rufus_amd jellyfish count: rfx_gzip: member 0" in r.stderr, r.stderr
    r = count(d, "x.Jhash", ["g.fastq.gz"], extra=["--bam", "x.chr"])
    assert r.returncode == 1 and b"is not BGZF" in r.stderr, r.stderr
