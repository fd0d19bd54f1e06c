"""Host: BAM before it ever runs on a GPU.  The reader of tests/bam_ref.py against the known figures of the three testRun
BAMs, rfx_bam_header (pure host code) against it, and the record core rufus_amd/csrc/rfx_bam_core.h -- the statements the
kernels of rfx_bam.hip run -- in tests/host/bam_harness.cpp, guess / walk / repair written serially and built with
-fsanitize=address,undefined when the compiler has it: the record starts must be the reader's for every tile size, with and
without guesses; every prefix and 200 seeded byte flips must end in a status or a chain that equals the naive walk (never a
sanitizer report, never a walk that does not end); every bam_valid refusal and the wrong-guess path must have been
reached."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from rufus_amd import capi
from tests import bam_ref as R
from tests import bgzf_ref as B
from tests.conftest import ROOT

# file: (BGZF blocks, records, kept with flag & 3328 == 0, header ends at, records that straddle a block, non-ACGT bases)
FIGURES = {"Child": (26, 4456, 4094, 6534, 24, 101), "Mother": (28, 4824, 4030, 6292, 26, 81),
           "Father": (21, 3625, 3278, 6420, 19, 115)}


@pytest.fixture(scope="module")
def fixtures():
    return {name: R.Bam(R.fixture(name)) for name in FIGURES}


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_reader_reproduces_the_known_figures(fixtures, name):
    bam = fixtures[name]
    blocks = B.split(bam.bam)  # (the EOF marker is one of them)
    non_acgt = sum(sum(c not in "ACGT" for c in r["seq"]) for r in bam.records if r["l_seq"])
    lens = [r["l_seq"] for r in bam.records]
    assert (len(blocks), len(bam.records), len(bam.kept()), bam.first, bam.straddlers(), non_acgt) == FIGURES[name]
    assert len(bam.refs) == 87 and 30 <= min(lens) and max(lens) == 151
    all_lens = [r["l_seq"] for b in fixtures.values() for r in b.records]
    assert (min(all_lens), max(all_lens)) == (30, 151)
    assert {r["flag"] & 3328 for b in fixtures.values() for r in b.records} == {0, 1024, 2048, 3072}


def _expect(bam: R.Bam):
    """(first_block, skip) of the block that holds inflated byte bam.first."""
    blocks, at = B.split(bam.bam), 0
    for blk, start in zip(blocks, bam.block_starts):
        isize = B.parts(blk)[3]
        if start <= bam.first < start + isize:
            return at, bam.first - start
        at += len(blk)
    return at, 0


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_header_of_the_fixtures(fixtures, name):
    bam = fixtures[name]
    h = capi.bam_header(bam.bam[:65536])
    assert h["n_ref"] == 87 and h["names"] == [n for n, _ in bam.refs]
    assert (h["first_block"], h["skip"]) == _expect(bam) == (0, FIGURES[name][3])


@pytest.mark.parametrize("n_blocks", [1, 2, 3, 4, 5])
def test_header_spanning_blocks_at_every_cut(n_blocks):
    refs = [(b"contig_%d_with_a_long_name" % i, 1000 + i) for i in range(60)]
    recs = [R.record(b"r%d" % i, 0, i % 60, i, [("M", 10)], "ACGTACGTAC") for i in range(5)]
    text = b"@HD\tVN:1.6\n"
    text += b"@CO\t" + b"x" * (-len(R.header(refs, text + b"@CO\t\n")) % 4) + b"\n"  # the header's length a multiple of 4
    hdr_len = len(R.header(refs, text))
    assert hdr_len % 4 == 0
    # the header ends inside block n_blocks; n_blocks == 5: exactly with block 4, so the first record begins block 5
    cut = hdr_len // 4 if n_blocks == 5 else -(-(hdr_len + 1) // n_blocks)
    bam = R.Bam(R.write(refs, recs, text, cut, 6))
    assert bam.first == hdr_len
    first_block, skip = _expect(bam)
    blocks = B.split(bam.bam)
    assert first_block == sum(len(b) for b in blocks[:n_blocks - 1]) and (skip == 0) == (n_blocks == 5)
    need = first_block if skip == 0 else first_block + len(blocks[n_blocks - 1])  # bytes that make the header whole
    for n in range(len(bam.bam) + 1):
        h = capi.bam_header(bam.bam[:n])
        if n < need:
            assert h is None, n
        else:
            assert h == {"n_ref": 60, "names": [x for x, _ in refs], "first_block": first_block, "skip": skip}, n


def test_header_refuses_what_is_not_bam():
    fastq = B.write(b"@r\nACGT\n+\nIIII\n" * 100)
    with pytest.raises(capi.RufusError, match=r"\(-8\)"):
        capi.bam_header(fastq)
    bad_magic = B.write(b"BAM\x02" + R.header([(b"chr1", 10)])[4:])
    with pytest.raises(capi.RufusError, match=r"\(-8\)"):
        capi.bam_header(bad_magic)
    with pytest.raises(capi.RufusError, match=r"\(-8\)"):
        capi.bam_header(b"@r\nACGT\n+\nIIII\n")  # not BGZF at all
    good = R.write([(b"chr1", 10)], [])
    blob = bytearray(good)
    blob[20] ^= 0x55  # inside the first block's payload
    with pytest.raises(capi.RufusError, match=r"\(-8\)"):
        capi.bam_header(bytes(blob))
    assert capi.bam_header(good) == {"n_ref": 1, "names": [b"chr1"], "first_block": len(B.split(good)[0]), "skip": 0}
    assert capi.bam_header(b"") is None


# ---- the record core under the sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bam") / "bam_harness")
    base = ["g++", "-O1", "-g", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "host", "bam_harness.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(base)
    return out


def _harness(harness, args, timeout=120):
    r = subprocess.run([harness] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    return r.stdout.decode()


def _run(harness, tmp_path, data, n_ref, skip, tile, no_guess):
    src, dst = tmp_path / "in.bin", tmp_path / "starts.bin"
    src.write_bytes(data)
    out = _harness(harness, ["run", src, n_ref, skip, tile, int(no_guess), dst])
    m = re.search(r"status (\d+) bad_at (\d+) records (\d+) cut (\d+) changed (\d+) rounds (\d+)", out)
    res = dict(zip(("status", "bad_at", "records", "cut", "changed", "rounds"), map(int, m.groups())))
    res["starts"] = np.fromfile(str(dst), np.uint32).tolist()
    res["refusals"] = list(map(int, re.search(r"refusals (.*)", out).group(1).split()))
    return res


def test_pack_word_maps_every_nibble(harness):
    assert _harness(harness, ["pack"]).startswith("pack ok")


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_record_starts_of_the_fixtures(fixtures, harness, tmp_path, name):
    bam = fixtures[name]
    for tile, no_guess in ((256, False), (4096, False), (16384, False), (16384, True), (256, True)):
        res = _run(harness, tmp_path, bam.data, 87, bam.first, tile, no_guess)
        assert res["starts"] == bam.starts and res["cut"] == len(bam.data) and res["status"] == 0, (tile, no_guess)
        if no_guess:
            assert res["changed"] > 0 and res["rounds"] >= res["changed"]
    # a cut inside the last record: the chain ends in front of it
    res = _run(harness, tmp_path, bam.data[:-7], 87, bam.first, 1024, False)
    assert res["starts"] == bam.starts[:-1] and res["cut"] == bam.starts[-1]


@pytest.mark.parametrize("tile", [256, 512, 1024, 4096, 16384])
def test_record_starts_of_synthetic_and_adversarial_files(harness, tmp_path, tile):
    wrong = 0
    for bam in (R.Bam(R.synthetic(cut=777)), R.Bam(R.adversarial(tile))):
        for no_guess in (False, True):
            res = _run(harness, tmp_path, bam.data, len(bam.refs), bam.first, tile, no_guess)
            assert res["starts"] == bam.starts and res["cut"] == len(bam.data) and res["status"] == 0, (tile, no_guess)
            wrong += res["changed"] if not no_guess else 0
    assert wrong >= 1  # the adversarial file's guesses land inside the aux array: repair changed them


def _small():
    rng = np.random.default_rng(41)
    recs = [R.record(b"q%d" % i, int(rng.choice([0, 16, 1024])), int(rng.integers(-1, 5)), i, [("M", 20 + i)],
                     R._seq(rng, 20 + i), bytes(rng.integers(0, 42, 20 + i, dtype=np.uint8)), b"NMC\x02" if i % 2 else b"")
            for i in range(40)]
    return R.Bam(R.write(R.REFS, recs))


def test_every_prefix_and_seeded_flips_end_in_a_status_or_a_chain(harness, tmp_path):
    bam = _small()
    assert 3000 < len(bam.data) < 8000
    src = tmp_path / "small.bin"
    src.write_bytes(bam.data)
    out = _harness(harness, ["trunc", src, 5, bam.first, 256], timeout=300)
    assert "trunc ok %d" % (2 * (len(bam.data) - bam.first + 1)) in out
    big = R.Bam(R.synthetic(n=300))
    src.write_bytes(big.data)
    out = _harness(harness, ["flips", src, 5, big.first, 512, 7, 200], timeout=300)
    assert "flips ok 200" in out
    assert int(re.search(r"refused (\d+)", out).group(1)) > 0  # some flips break a field, the others leave a valid chain
    assert int(re.search(r"wrong_guess (\d+)", out).group(1)) > 0


def test_every_refusal_of_bam_valid_is_reached_and_named(harness, tmp_path):
    bam = _small()
    target = bam.starts[len(bam.starts) // 2]
    patches = {1: (0, struct.pack("<I", 10)),            # block_size = 10
               2: (12, b"\0"),                           # l_read_name = 0
               3: (20, struct.pack("<i", -5)),           # l_seq < 0
               4: (20, struct.pack("<i", 100000)),       # the sequence does not fit block_size
               5: (4, struct.pack("<i", 5))}             # refID == n_ref
    seen = [0] * 5
    for status, (off, val) in patches.items():
        data = bytearray(bam.data)
        data[target + off:target + off + len(val)] = val
        for no_guess in (False, True):
            res = _run(harness, tmp_path, bytes(data), 5, bam.first, 256, no_guess)
            assert (res["status"], res["bad_at"]) == (status, target), (status, res)
            assert res["starts"][:len(bam.starts) // 2 + 1] == bam.starts[:len(bam.starts) // 2 + 1]
            seen = [a + b for a, b in zip(seen, res["refusals"])]
    assert all(seen), seen
    res = _run(harness, tmp_path, bam.data, 5, bam.first, 256, False)
    assert res["refusals"] == [0] * 5 and res["status"] == 0
