"""Host: the BAM index before it ever steers a GPU run.  rufus_amd/csrc/host/rfx_bai.hpp -- the region's text, the BAI
reader, the one-range query -- and the region test of rufus_amd/csrc/rfx_bam_core.h (the statements k_bam_region runs) in
tests/host/bai_harness.cpp, a stand-alone program built with -fsanitize=address,undefined when the compiler has it, against
tests/bai_ref.py: the specification's values, every form and every refusal of a region text, START / STOP / "empty" of 200
seeded regions over four files and four indexes each, every index the reader must refuse (never a sanitizer report), and
bam_end_pos / bam_in_region on the record table the GPU test uses.  Fails without the feature: neither header has these."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bai_ref as X
from tests import bam_ref as R
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bai") / "bai_harness")
    base = ["g++", "-O1", "-g", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "host", "bai_harness.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(base)
    return out


def _harness(harness, args, timeout=120):
    r = subprocess.run([harness] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    return r.stdout.decode()


@pytest.fixture(scope="module")
def bams():
    """name -> Bam: the three testRun files and the sorted synthetic one.  Read once, never changed."""
    out = {name: R.Bam(R.fixture(name)) for name in ("Child", "Mother", "Father")}
    out["sorted"] = R.Bam(X.sorted_bam())
    return out


# ---- the specification's values ---------------------------------------------------------------------------------------
def test_binning_scheme(harness):
    assert (X.reg2bin(0, 1 << 14), X.reg2bin(0, 1 << 29), len(X.reg2bins(123456, 123457))) == (4681, 0, 6)
    out = _harness(harness, ["spec"]).split("\n")
    assert out[0] == "reg2bin 4681 0 4682"
    assert out[1] == "reg2bins_one 6"
    assert out[2] == "reg2bins_all %d" % len(X.reg2bins(0, 1 << 29)) == "reg2bins_all 37449"
    assert out[3] == "reg2bins_none 0 0"


# ---- region texts -----------------------------------------------------------------------------------------------------
NAMES = ["4", "5", "chrB:1", "HLA-A*01:01", "5:7"]


@pytest.mark.parametrize("text,want", [
    ("5", (1, 0, 1 << 29)),
    ("5:7", (4, 0, 1 << 29)),                       # a name as a whole wins over NAME:BEG
    ("5:8", (1, 7, 1 << 29)),
    ("5:1,000-2,000", (1, 999, 2000)),
    ("5:177640001-177645000", (1, 177640000, 177645000)),
    ("5:7-7", (1, 6, 7)),
    ("chrB:1", (2, 0, 1 << 29)),                    # a name with a colon
    ("chrB:1:10-20", (2, 9, 20)),                   # ... cut at the LAST colon
    ("HLA-A*01:01", (3, 0, 1 << 29)),
    ("HLA-A*01:01:5", (3, 4, 1 << 29)),
    ("5:7:3-4", (4, 2, 4)),
    ("5:2147483654-2147483658", (1, 2147483653, 2147483658)),
])
def test_region_forms(harness, text, want):
    assert X.parse_region(text, [n.encode() for n in NAMES]) == want
    assert _harness(harness, ["region", text] + NAMES) == "ok %d %d %d\n" % want


@pytest.mark.parametrize("text", ["6", "6:1-2", "chrB", "5:0-10", "5:0", "5:10-9", "5:10-20x", "5:10-", "5:-10", "5:", "5:1-2-3",
                                  "5:a-b", "5:1 -2", "", ":", "5:99999999999999999999", "5:1-99999999999999999999"])
def test_region_refusals(harness, text):
    assert X.parse_region(text, [n.encode() for n in NAMES]) is None
    out = _harness(harness, ["region", text] + NAMES)
    assert out.startswith("refused region '%s': " % text), out  # the message names the region


# ---- reader and query against bai_ref ---------------------------------------------------------------------------------
def _regions(bam, rng, n):
    """Seeded (tid, beg, end): around the records, at window and bin boundaries, whole references, beyond the data."""
    placed = [r for r in bam.records if r["ref_id"] >= 0]
    out = []
    while len(out) < n:
        kind = len(out) % 5
        r = placed[int(rng.integers(0, len(placed)))]
        tid = r["ref_id"]
        if kind == 0:
            beg = max(0, r["pos"] - int(rng.integers(0, 300)))
            out.append((tid, beg, beg + int(rng.integers(1, 5000))))
        elif kind == 1:
            edge = (r["pos"] >> 14 << 14) + int(rng.integers(-2, 3))
            out.append((tid, max(0, edge), max(0, edge) + int(rng.integers(1, 40000))))
        elif kind == 2:
            out.append((tid, 0, 1 << 29))
        elif kind == 3:
            out.append((int(rng.integers(0, len(bam.refs))), int(rng.integers(0, 1 << 28)), int(rng.integers(1 << 28, 1 << 29))))
        else:
            beg = X.end_pos(r) - 1 + int(rng.integers(0, 2))  # the record's last base, or the base behind it
            out.append((tid, beg, beg + 1))
    return out


@pytest.mark.parametrize("kind,spelling", [("fine", "next"), ("fine", "same"), ("coarse", "next"), ("coarse", "same")])
@pytest.mark.parametrize("name", ["Child", "Mother", "Father", "sorted"])
def test_query_equals_the_reference(harness, bams, tmp_path, name, kind, spelling):
    bam = bams[name]
    bai = X.build(bam, kind, spelling)
    index = X.parse(bai)
    regions = _regions(bam, np.random.default_rng(71), 200)
    (tmp_path / "x.bai").write_bytes(bai)
    (tmp_path / "q.txt").write_text("".join("%d %d %d\n" % r for r in regions))
    got = _harness(harness, ["query", tmp_path / "x.bai", len(bam.bam), len(bam.refs), tmp_path / "q.txt"]).split("\n")[:-1]
    want = [X.query(index, *r) for r in regions]
    assert got == ["empty" if w is None else "%d %d" % w for w in want]
    assert sum(w is not None for w in want) >= 100
    if kind == "fine":  # (a coarse index answers "empty" only for a reference without records)
        assert sum(w is None for w in want) >= 1
    # the range is a superset: every record of the region starts inside it
    v = X._Voff(bam)
    for reg, w in zip(regions[:40], want[:40]):
        inside = [v.start(r["start"]) for r in bam.records if X.in_region(r, *reg)]
        assert (not inside) if w is None else all(w[0] <= s < w[1] for s in inside), reg


def test_the_sorted_file_is_what_the_tests_need(bams):
    bam = bams["sorted"]
    assert 5900 <= len(bam.records) <= 6100 and len(bam.block_starts) >= 200 and len(bam.refs) == 3
    assert any(r["flag"] & 4 and r["ref_id"] >= 0 for r in bam.records) and any(r["ref_id"] < 0 for r in bam.records)
    assert bam.straddlers() >= 100
    both = {X.build(bam, "fine", s) for s in ("next", "same")}
    assert len(both) == 2  # some chunk ends with its block: the two spellings differ


# ---- indexes the reader must refuse -----------------------------------------------------------------------------------
def _small():
    rng = np.random.default_rng(72)
    recs = [R.record(b"q%d" % i, 0, i // 20, 1000 * i + 5, [("M", 30)], R._seq(rng, 30, True)) for i in range(40)]
    return R.Bam(R.write(R.REFS, recs, cut=700))


def test_every_truncation_is_refused(harness, tmp_path):
    bam = _small()
    for kind in ("fine", "coarse"):
        bai = X.build(bam, kind)
        assert 100 < len(bai) < 2000
        (tmp_path / "s.bai").write_bytes(bai)
        out = _harness(harness, ["trunc", tmp_path / "s.bai", len(bam.bam), len(bam.refs)])
        # whole, and without the optional n_no_coor: the only prefixes that are indexes
        assert out == "trunc accepted %d %d\n" % (len(bai) - 8, len(bai)), out


def _patched(bai, at, fmt, value):
    blob = bytearray(bai)
    struct.pack_into(fmt, blob, at, value)
    return bytes(blob)


def test_damaged_indexes_are_refused(harness, tmp_path):
    bam = _small()
    bai = X.build(bam, "coarse")
    # coarse layout: magic, n_ref, then per reference with records n_bin = 1 | bin 0, n_chunk = 1 | beg, end | n_intv = 1 | ioffset
    assert struct.unpack_from("<iIi", bai, 8) == (1, 0, 1)
    beg, end = struct.unpack_from("<QQ", bai, 20)
    cases = {
        "no BAI magic": b"BAM\x01" + bai[4:],
        "n_ref differs": _patched(bai, 4, "<i", len(bam.refs) + 1),
        "negative n_bin": _patched(bai, 8, "<i", -1),
        "negative n_chunk": _patched(bai, 16, "<i", -1),
        "a chunk beyond": _patched(bai, 28, "<Q", len(bam.bam) << 16),
        "does not end behind its start": _patched(bai, 28, "<Q", beg),
        "negative n_intv": _patched(bai, 36, "<i", -1),
        "truncated": _patched(bai, 16, "<i", 1 << 30),
        "a linear index entry beyond": _patched(bai, 40, "<Q", (len(bam.bam) + 5) << 16),
    }
    (tmp_path / "q.txt").write_text("0 0 100000\n")
    for why, blob in cases.items():
        (tmp_path / "bad.bai").write_bytes(blob)
        out = _harness(harness, ["query", tmp_path / "bad.bai", len(bam.bam), len(bam.refs), tmp_path / "q.txt"])
        assert out.startswith("refused ") and why in out, (why, out)
    (tmp_path / "ok.bai").write_bytes(_patched(bai, 28, "<Q", beg + 1))  # (beg < end by one: still an index)
    out = _harness(harness, ["query", tmp_path / "ok.bai", len(bam.bam), len(bam.refs), tmp_path / "q.txt"])
    assert out == "%d %d\n" % (beg, beg + 1) and end > beg + 1


# ---- the record core --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", X.TABLE_REGIONS)
def test_end_pos_and_in_region_on_the_table(harness, tmp_path, region):
    recs = X.region_table(400)
    data = b"".join(recs)
    parsed = R.read_records(data, 0)
    (tmp_path / "recs.bin").write_bytes(data)
    got = _harness(harness, ["recs", tmp_path / "recs.bin", len(X.TABLE_REFS)] + list(region)).split("\n")[:-1]
    want = ["%d %d" % (X.end_pos(r), X.in_region(r, *region)) for r in parsed]
    assert got == want
    assert max(X.end_pos(r) for r in parsed) >= 1 << 32 and any(X.in_region(r, *region) for r in parsed)
