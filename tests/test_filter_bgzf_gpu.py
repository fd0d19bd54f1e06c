"""GPU: `RUFUS.Filter HashList A.fastq.gz B.fastq.gz STUB K MinQ Thresh Threads` -- both mates bgzip'd, inflated, parsed,
scanned and the pulled pairs' text gathered on the device (rufus_amd/csrc/host/rfx_ingest.hpp BgzfPairFilter,
rufus_amd/csrc/rfx_gather.hip) -- against the same binary on the plain-text files, the golden outputs of the reference's
test trio and the reference's own binary.  The driver's logic runs without a GPU in tests/test_filter_bgzf_host.py."""
import hashlib
import os
import subprocess

import pytest

from tests import bgzf_ref as B
from tests import filter_bgzf_ref as F
from tests.conftest import ROOT, require_ref

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
STRICT = b"compressed input must be strict 4-line FASTQ: inflate it and pipe it in"


def run_filter(d, hl, m1, m2, stub, env=None, k=F.K):
    return subprocess.run([f"{BIN}/RUFUS.Filter", hl, m1, m2, stub, str(k), str(F.MIN_Q), str(F.THRESH), "5"], cwd=d,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def outputs(d, stub):
    return [open(f"{d}/{stub}.Mutations.Mate{m}.fastq", "rb").read() for m in (1, 2)]


def trace_counts(stderr):
    """{blocks, appends, steps, pairs, pulled} of the trace line of the BGZF route."""
    t = stderr.decode()
    w = t[t.index("filter: bgzf route: "):].replace(",", "").split()
    return {"blocks": int(w[3]), "appends": int(w[6]), "steps": int(w[8]), "pairs": int(w[10]), "pulled": int(w[12])}


def test_testrun_child_compressed_equals_text_and_the_goldens(testrun, tmp_path):
    d = str(tmp_path)
    open(f"{d}/hl", "w").write(testrun["hashlist"])
    for m in (1, 2):
        open(f"{d}/m{m}.fq", "wb").write(testrun["Child"][m - 1])
        open(f"{d}/m{m}.fastq.gz", "wb").write(B.write(testrun["Child"][m - 1]))
    r = run_filter(d, "hl", "m1.fq", "m2.fq", "text")
    assert r.returncode == 0 and b"bgzf route" not in r.stderr, r.stderr
    r = run_filter(d, "hl", "m1.fastq.gz", "m2.fastq.gz", "gz")
    assert r.returncode == 0, r.stderr
    assert b"Done running RUFUS.Filter.cpp" in r.stdout
    got = outputs(d, "gz")
    assert got == outputs(d, "text")
    exp = testrun["expected"]
    for m in (1, 2):
        assert hashlib.sha256(got[m - 1]).hexdigest() == exp["filter_paired_sha256"][str(m)]
    names = [ln for ln in got[0].split(b"\n")[0::4] if ln]
    assert len(names) == 26 and [n.decode() for n in names] == exp["filter_paired_names"]
    c = trace_counts(r.stderr)
    assert c["pairs"] == testrun["Child"][0].count(b"\n") // 4 and c["pulled"] == 26


@pytest.fixture(scope="module")
def ragged():
    genome, m1, m2 = F.ragged_pairs(20_000)
    hl = F.hash_list(genome, 40)
    idx, want1, want2 = F.pulled(hl, m1, m2)
    assert 0.001 * len(m1) <= len(idx) <= 0.05 * len(m1)  # the comparisons below are not of empty files
    return hl, m1, m2, want1, want2


@pytest.mark.parametrize("level", [0, 1, 6])
def test_ragged_mates_equal_the_text_route_and_the_reference_binary(ragged, tmp_path, level):
    ref = require_ref("RUFUS.Filter")
    hl, m1, m2, want1, want2 = ragged
    d = str(tmp_path)
    open(f"{d}/hl", "wb").write(hl)
    for name, recs in (("m1", m1), ("m2", m2)):
        open(f"{d}/{name}.fq", "wb").write(b"".join(recs))
        open(f"{d}/{name}.fastq.gz", "wb").write(B.write(b"".join(recs), level))
    r = subprocess.run([ref, "hl", "m1.fq", "m2.fq", "ref", str(F.K), str(F.MIN_Q), str(F.THRESH), "1"], cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0
    want = outputs(d, "ref")
    assert want == [want1, want2] and len(want1) > 5000  # (the reference pulls what the oracle pulls: 0.1 % .. 5 % of the pairs)
    r = run_filter(d, "hl", "m1.fq", "m2.fq", "text")
    assert r.returncode == 0, r.stderr
    assert outputs(d, "text") == want
    r = run_filter(d, "hl", "m1.fastq.gz", "m2.fastq.gz", "gz", {"RFX_FILTER_ARENA": "1048576", "RFX_INGEST_PIECE": "70000"})
    assert r.returncode == 0, r.stderr
    assert outputs(d, "gz") == want
    c = trace_counts(r.stderr)
    assert c["steps"] > 3 and c["pairs"] == len(m1) and c["appends"] > c["steps"]


def test_ends_and_refusals(ragged, tmp_path):
    hl, m1, m2, want1, want2 = ragged
    m1, m2 = m1[:6000], m2[:6000]
    _, want1, want2 = F.pulled(hl, m1, m2)
    assert len(want1) > 1000
    d = str(tmp_path)
    open(f"{d}/hl", "wb").write(hl)
    t1, t2 = b"".join(m1), b"".join(m2)
    env = {"RFX_FILTER_ARENA": "1048576", "RFX_INGEST_PIECE": "70000"}

    def run(gz1, gz2, stub):
        open(f"{d}/a.fastq.gz", "wb").write(gz1)
        open(f"{d}/b.fastq.gz", "wb").write(gz2)
        return run_filter(d, "hl", "a.fastq.gz", "b.fastq.gz", stub, env)

    def refused(r, message):
        assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr[-500:])

    # mate 2 with extra records: the same output
    r = run(B.write(t1, 1), B.write(t2 + b"".join(m2[:900]), 1), "extra")
    assert r.returncode == 0 and outputs(d, "extra") == [want1, want2], r.stderr
    # a last line without a newline: the same output as with one
    r = run(B.write(t1[:-1], 1), B.write(t2[:-1], 1), "nonl")
    assert r.returncode == 0 and outputs(d, "nonl") == [want1, want2], r.stderr
    # mate 2 short
    refused(run(B.write(t1, 1), B.write(b"".join(m2[:-1]), 1), "short"), b"mate files hold different numbers of records")
    # one mate compressed, one as text
    open(f"{d}/m2.fq", "wb").write(t2)
    open(f"{d}/a.fastq.gz", "wb").write(B.write(t1, 1))
    r = run_filter(d, "hl", "a.fastq.gz", "m2.fq", "mixed", env)
    refused(r, b"give both mates compressed or both as text")
    # a blank line in mate 2
    at = t2.index(b"\n@", len(t2) // 2) + 1
    refused(run(B.write(t1, 1), B.write(t2[:at] + b"\n" + t2[at:], 1), "blank"), STRICT)
    # mate 1 ends inside a record
    refused(run(B.write(t1[:-40], 1), B.write(t2, 1), "cut"), STRICT)
    # an empty sequence line in mate 1
    bad = list(m1)
    bad[3000] = b"@empty\n\n+\n\n"
    refused(run(B.write(b"".join(bad), 1), B.write(t2, 1), "empty"), b"empty sequence line (undefined behaviour in the reference) -- rejected")
    # more than one device is refused, as the count refuses it
    r = run_filter(d, "hl", "a.fastq.gz", "a.fastq.gz", "two", dict(env, RUFUS_GPUS="0,0"))
    refused(r, b"needs one device")


def test_a_block_that_does_not_inflate_is_named(ragged, tmp_path):
    """A flipped byte in the payload of mate 2's third block (the corrupt set of tests/bgzf_ref.py has passed on the host
    and on the device, tests/test_bgzf_host.py and tests/test_bgzf_gpu.py: this is one more CRC mismatch).  One run."""
    hl, m1, m2, _, _ = ragged
    d = str(tmp_path)
    open(f"{d}/hl", "wb").write(hl)
    open(f"{d}/a.fastq.gz", "wb").write(B.write(b"".join(m1[:6000]), 1))
    blob = bytearray(B.write(b"".join(m2[:6000]), 1))
    blocks = B.split(bytes(blob))
    blob[sum(map(len, blocks[:2])) + 18 + len(B.parts(blocks[2])[1]) // 2] ^= 0x5A
    open(f"{d}/b.fastq.gz", "wb").write(bytes(blob))
    r = run_filter(d, "hl", "a.fastq.gz", "b.fastq.gz", "flip")
    assert r.returncode != 0 and b"rfx_bgzf: block 2" in r.stderr, r.stderr
