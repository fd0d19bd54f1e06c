"""Host: the BGZF decoder before it ever runs on a GPU.  rfx_bgzf_scan (the one function that cuts a BGZF file) against
this file's own reading of the container, and the decoder core rufus_amd/csrc/rfx_bgzf_core.h -- the statements the kernel
k_bgzf_inflate runs -- in tests/host/bgzf_harness.cpp with a serial copy, built with -fsanitize=address,undefined when the
compiler has it: over the corpus of tests/bgzf_ref.py (output CRC = zlib.crc32 of the original; the statistics prove that
every shape the decoder branches on was reached) and over the corrupt set (one mutation per refusal, 200 seeded flips and
truncations: refused with a status, or decoded to bytes whose CRC and ISIZE match; never a sanitizer report, never a run
that does not end).  tests/test_bgzf_gpu.py sends the same corrupt bytes to the device only after this has passed."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import pytest

from rufus_amd import capi
from tests import bgzf_ref as B
from tests.conftest import ROOT


def scan(buf, max_blocks=0xFFFFFFFF, n=None):
    nb, used, inf = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    rc = capi.lib().rfx_bgzf_scan(buf, len(buf) if n is None else n, max_blocks, C.byref(nb), C.byref(used), C.byref(inf))
    return rc, nb.value, used.value, inf.value


@pytest.fixture(scope="module")
def corpus():
    return B.corpus()


def test_scan_reports_an_incomplete_tail_at_every_cut(corpus):
    blocks = [b for _, _, b in corpus[:3]]
    data = b"".join(blocks)
    ends = [len(blocks[0]), len(blocks[0]) + len(blocks[1]), len(data)]
    sizes = [len(d) for _, d, _ in corpus[:3]]
    for cut in range(len(data) + 1):
        rc, nb, used, inf = scan(data, n=cut)
        whole = sum(1 for e in ends if e <= cut)
        assert (rc, nb, used, inf) == (0, whole, ([0] + ends)[whole], sum(sizes[:whole])), cut


def test_scan_walks_every_byte_offset_of_the_first_block(corpus):
    blk = corpus[5][2]  # (a short one: every prefix of it)
    for cut in range(len(blk) + 1):
        rc, nb, used, _ = scan(blk[:cut])
        assert rc == 0 and nb == (cut == len(blk)) and used == (len(blk) if cut == len(blk) else 0), cut


def test_scan_finds_a_bc_subfield_that_is_not_first():
    data = b"some bytes to deflate" * 9
    blk = B.block(data, extra_before=b"XY\x03\x00abc" + b"ZZ\x00\x00")
    assert scan(blk) == (0, 1, len(blk), len(data))
    assert capi.bgzf_scan(blk + B.EOF) == (2, len(blk) + 28, len(data))


def test_scan_refuses_what_is_not_bgzf():
    blk = B.block(b"hello")
    bad_magic = b"\x1f\x8c" + blk[2:]
    no_fextra = blk[:3] + b"\x00" + blk[4:]
    gz = zlib.compressobj(6, zlib.DEFLATED, 31)
    plain_gzip = gz.compress(b"hello") + gz.flush()
    other_subfield = blk[:12] + b"BD" + blk[14:]
    for bad in (bad_magic, no_fextra, plain_gzip, other_subfield):
        assert scan(bad)[0] == capi.E_FORMAT
        rc, nb, used, _ = scan(blk + bad)  # what lies before it is reported
        assert (rc, nb, used) == (capi.E_FORMAT, 1, len(blk))
    with pytest.raises(capi.RufusError):
        capi.bgzf_scan(bad_magic)
    huge = blk[:-4] + struct.pack("<I", 65537)
    assert scan(huge)[0] == capi.E_FORMAT


def test_scan_honours_max_blocks(corpus):
    blocks = [b for _, _, b in corpus[6:12]]
    data = b"".join(blocks)
    for m in range(len(blocks) + 2):
        rc, nb, used, _ = scan(data, m)
        k = min(m, len(blocks))
        assert (rc, nb, used) == (0, k, sum(map(len, blocks[:k])))


# ---- the decoder core under the sanitizers --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bgzf") / "bgzf_harness")
    base = ["g++", "-O1", "-g", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "host", "bgzf_harness.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(base)
    return out


def run_harness(harness, tmp_path, named_blobs):
    """{name: {"blocks": [(status, isize)], "format": bool, "crc": int, "bytes": int, stats...}} of one harness run."""
    paths = []
    for name, blob in named_blobs:
        p = tmp_path / (name + ".bgzf")
        p.write_bytes(blob)
        paths.append(str(p))
    r = subprocess.run([harness] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stdout.decode().splitlines():
        w = line.split()
        if w[0] == "file":
            cur = out[os.path.basename(w[1])[:-5]] = {"blocks": [], "format": False}
        elif w[0] == "block":
            cur["blocks"].append((int(w[3]), int(w[5])))
        elif w[0] == "format":
            cur["format"] = True
        elif w[0] == "crc":
            cur["crc"], cur["bytes"] = int(w[1], 16), int(w[3])
        elif w[0] == "types":
            cur.update({k: int(v) for k, v in (x.split("=") for x in w[1:])})
        elif w[0] in ("dist", "len"):
            cur[w[0]] = (int(w[1]), int(w[2]))
        else:
            cur[w[0]] = int(w[1])
    assert len(out) == len(named_blobs)
    return out


def test_core_inflates_the_corpus_and_reaches_every_shape(harness, tmp_path, corpus):
    got = run_harness(harness, tmp_path, [(name, blk) for name, _, blk in corpus])
    for name, data, _ in corpus:
        g = got[name]
        assert g["blocks"] == [(0, len(data))] and (g["crc"], g["bytes"]) == (zlib.crc32(data), len(data)), name
    kinds = lambda g: (g["stored"] > 0, g["fixed"] > 0, g["dynamic"] > 0)
    # FASTQ text: several dynamic blocks, long codes, matches from distance 1 to near the window's end
    for name in ("fastq_l6", "fastq_l1"):
        g = got[name]
        assert kinds(g) == (False, False, True) and g["deflate_blocks_max"] >= 2 and g["longest_code"] >= 12
        assert g["dist"][0] == 1 and g["dist"][1] > 32000 and g["len"][0] == 3
    assert kinds(got["fastq_l9_mem1"])[2] and got["fastq_l9_mem1"]["deflate_blocks_max"] >= 100  # a table build per 128 symbols
    assert kinds(got["fastq_fixed"]) == (False, True, False) and got["fastq_fixed"]["dist"][1] > 32000
    assert kinds(got["fastq_l0"]) == (True, False, False) and got["fastq_l0"]["stored"] == 2
    assert kinds(got["isize_65536"])[1:] == (True, True)  # fixed and dynamic in one BGZF block
    assert got["all_A"]["dist"] == (1, 1) and got["all_A"]["len"] == (4, 258)
    for p in B.PERIODS:  # overlapping matches of the longest length at distances around the lane count
        g = got["period_%d" % p]
        assert g["dist"][1] == p and g["len"][1] == 258, p
    assert got["fibonacci"]["longest_code"] == 15 and got["fibonacci"]["dist"] == (0, 0)
    assert got["empty"]["bytes"] == 0 and got["one_byte"]["bytes"] == 1
    assert got["hand_far_match"]["dist"] == (32768, 32768) and got["hand_far_match"]["len"] == (258, 258)
    assert kinds(got["hand_far_match"]) == (True, True, False)
    assert got["hand_run_across"]["cl_cross"] == 1 and got["hand_one_dist_code"]["one_dist_code"] == 1
    assert not any(got[n]["cl_cross"] or got[n]["one_dist_code"] for n in got if not n.startswith("hand_"))  # (zlib never writes them)


def test_core_inflates_the_big_file(harness, tmp_path):
    data, blocks = B.big_file()
    g = run_harness(harness, tmp_path, [("big", b"".join(blocks))])["big"]
    assert len(g["blocks"]) == len(blocks) >= 300 and all(s == 0 for s, _ in g["blocks"]) and not g["format"]
    assert (g["crc"], g["bytes"]) == (zlib.crc32(data), len(data)) and len(data) > 5 << 20


def test_core_refuses_each_malformation_with_its_own_status(harness, tmp_path):
    cases = B.refusals()
    assert sorted({s for _, s, _ in cases}) == list(range(1, 17))  # every refusal of rfx_bgzf_core.h but "no such code"
    got = run_harness(harness, tmp_path, [(name, blk) for name, _, blk in cases])
    for name, status, _ in cases:
        assert [s for s, _ in got[name]["blocks"]] == [status] and got[name]["bytes"] == 0, name
    hdr = open(os.path.join(ROOT, "rufus_amd", "csrc", "rfx_bgzf_core.h")).read()
    assert {int(v) for v in re.findall(r"BGZF_E_\w+ = (\d+),", hdr)} == set(range(1, 18))


def test_core_survives_seeded_damage(harness, tmp_path):
    cases = B.seeded_damage()
    assert len(cases) == 200
    good = B.block(b"a good block behind the damaged one")
    got = run_harness(harness, tmp_path, [(name, blk + good) for name, blk, _ in cases])
    passed = 0
    for name, blk, may_pass in cases:
        g = got[name]
        # refused with a status, or cut off by the container walk -- or decoded, CRC and ISIZE matching (status 0 says so)
        refused = g["format"] or (g["blocks"] and g["blocks"][0][0] != 0)
        assert refused or may_pass, name
        passed += not refused
    assert passed < 20
