"""CPU-only: the lock-step driver of `RUFUS.Filter A.fastq.gz B.fastq.gz` (rufus_amd/csrc/host/rfx_ingest.hpp,
BgzfPairFilter) through tests/host/filter_bgzf_harness.cpp -- the class over host stand-ins for the device entry points,
a stand-alone program built plain and with -fsanitize=address,undefined.  The harness compares what the driver pulled with
its own direct computation on the whole inflated files; here the same bytes are also compared with the oracle's filter.
The real tool is compared with the text route and the reference binary in tests/test_filter_bgzf_gpu.py."""
import os
import subprocess

import pytest

from tests import bgzf_ref as B
from tests import filter_bgzf_ref as F
from tests.conftest import ROOT

HARNESS_SRC = os.path.join(ROOT, "tests", "host", "filter_bgzf_harness.cpp")
HOST_SRC = os.path.join(ROOT, "rufus_amd", "csrc", "rfx_host.cpp")
STRICT = b"compressed input must be strict 4-line FASTQ: inflate it and pipe it in"
ARENA, PIECE = 4 * 65536, 70000  # the smallest arena the driver takes


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fbgzf") / ("harness_" + request.param))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", out, HARNESS_SRC, HOST_SRC]
    if request.param == "sanitized":
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        if subprocess.run(cmd, stderr=subprocess.DEVNULL).returncode == 0:
            return out
        cmd = cmd[:-2]  # (a compiler without the sanitizers: the plain build twice, as tests/test_bgzf_host.py does)
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def data():
    genome, m1, m2 = F.ragged_pairs(3000)
    hl = F.hash_list(genome, 12)
    idx, want1, want2 = F.pulled(hl, m1, m2)
    assert 3 <= len(idx) <= 150  # 0.1 % .. 5 % of the pairs: the comparisons are not of empty files
    return hl, m1, m2, want1, want2


def run(harness, d, hl, gz1, gz2, arena=ARENA, piece=PIECE, stub="out"):
    for name, blob in (("hl", hl), ("a.gz", gz1), ("b.gz", gz2)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(blob)
    r = subprocess.run([harness, "hl", "a.gz", "b.gz", str(F.K), str(F.MIN_Q), str(F.THRESH), str(arena), str(piece), stub], cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def ok(r):
    assert r.returncode == 0, r.stderr[-2000:]
    w = r.stdout.split()
    assert w[0] == b"ok"
    return {w[i].decode(): int(w[i + 1]) for i in range(1, len(w), 2)}


def outputs(d, stub="out"):
    return [open(os.path.join(d, f"{stub}.Mate{m}.fastq"), "rb").read() for m in (1, 2)]


@pytest.mark.parametrize("level,arena,piece,steps", [(1, ARENA, PIECE, 4), (6, ARENA, 1024, 4), (0, 3 * ARENA, 200000, 2),
                                                     (1, 1 << 24, 8 << 20, 1)])
def test_unequal_mates_in_lock_step_equal_the_direct_computation_and_the_oracle(harness, data, tmp_path, level, arena, piece, steps):
    hl, m1, m2, want1, want2 = data
    s = ok(run(harness, str(tmp_path), hl, B.write(b"".join(m1), level), B.write(b"".join(m2), level), arena, piece))
    assert s["pairs"] == len(m1) and outputs(str(tmp_path)) == [want1, want2]
    # (mate 2's records are longer: its arena fills first, and mate 1's text moves on by carries)
    assert s["steps"] >= steps and (steps > 1 or s["steps"] == 1)


def test_ends_of_the_two_files(harness, data, tmp_path):
    hl, m1, m2, want1, want2 = data
    d = str(tmp_path)
    t1, t2 = b"".join(m1), b"".join(m2)
    extra = b"".join(m2[:700])
    # mate 2 goes on after mate 1's end: ignored
    ok(run(harness, d, hl, B.write(t1, 1), B.write(t2 + extra, 1)))
    assert outputs(d) == [want1, want2]
    # no newline after the last line, in either file and in both
    for a, b in ((t1[:-1], t2), (t1, t2[:-1]), (t1[:-1], t2[:-1])):
        ok(run(harness, d, hl, B.write(a, 1), B.write(b, 1)))
        assert outputs(d) == [want1, want2]
    # the file's last block is no EOF marker; an EOF marker in the middle
    blocks = B.split(B.write(t1, 1, eof=False))
    ok(run(harness, d, hl, b"".join(blocks[:3]) + B.EOF + b"".join(blocks[3:]), B.write(t2, 1)))
    assert outputs(d) == [want1, want2]
    # an empty mate 1: nothing to do, whatever mate 2 holds
    s = ok(run(harness, d, hl, B.write(b"", 1), B.write(t2, 1)))
    assert s["pairs"] == 0 and outputs(d) == [b"", b""]


def test_refusals(harness, data, tmp_path):
    hl, m1, m2, _, _ = data
    d = str(tmp_path)
    t1, t2 = b"".join(m1), b"".join(m2)

    def refused(gz1, gz2, message):
        r = run(harness, d, hl, gz1, gz2)
        assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr[-500:])

    # mate 2 runs out first: at a record boundary, and one record short over many steps
    refused(B.write(t1, 1), B.write(b"".join(m2[:-1]), 1), b"mate files hold different numbers of records")
    refused(B.write(t1, 1), B.write(b"".join(m2[:1200]), 1), b"mate files hold different numbers of records")
    refused(B.write(t1, 1), B.write(b"", 1), b"mate files hold different numbers of records")
    # a blank line between two records of mate 2
    at = t2.index(b"\n@", len(t2) // 2) + 1
    refused(B.write(t1, 1), B.write(t2[:at] + b"\n" + t2[at:], 1), STRICT)
    # a file that ends inside a record (whole blocks: the text is cut, not the container)
    refused(B.write(t1[:-40], 1), B.write(t2, 1), STRICT)
    refused(B.write(t1, 1), B.write(t2[:len(t2) // 2 - 7], 1), STRICT)
    # a "record" longer than an arena
    long_line = b"@long\n" + b"A" * (2 * ARENA) + b"\n+\n" + b"I" * (2 * ARENA) + b"\n"
    refused(B.write(long_line + t1, 1), B.write(t2, 1), STRICT)
    # the container cut inside a block
    refused(B.write(t1, 1), B.write(t2, 1)[:-100], b"truncated BGZF block")
    # a flipped byte in the payload of mate 2's third block
    blob = bytearray(B.write(t2, 1))
    blocks = B.split(bytes(blob))
    blob[sum(map(len, blocks[:2])) + 18 + len(B.parts(blocks[2])[1]) // 2] ^= 0x5A
    refused(B.write(t1, 1), bytes(blob), b"rfx_bgzf: block 2")
    # an empty sequence line in mate 1 (the text route's message)
    bad = list(m1)
    bad[1500] = b"@empty\n\n+\n\n"
    refused(B.write(b"".join(bad), 1), B.write(t2, 1), b"empty sequence line (undefined behaviour in the reference) -- rejected")
