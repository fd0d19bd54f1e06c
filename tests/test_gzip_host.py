"""Host: the plain-gzip route before it ever runs on a GPU.  tests/host/gzip_harness.cpp -- a stand-alone program, built
plain and with -fsanitize=address,undefined and run directly -- runs the host side of rufus_amd/csrc/rfx_gzip_core.h end to
end (find, walk, the chain rule gz_append the library itself runs, marker inflate, windows, resolve, CRC: the statements
the kernels of rfx_gzip.hip run) and the ingest class GzipIngest of rufus_amd/csrc/host/rfx_ingest.hpp over host stand-ins
for the arenas.  Truth is tests/gzip_ref.py: zlib's bytes, zlib's own Z_BLOCK walk for the block starts.  Every written
buffer has guard bytes on both sides; the input is an exact heap copy.  tests/test_gzip_gpu.py sends the same files to the
device."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import gzip_ref as G
from tests.conftest import ROOT

HARNESS_SRC = os.path.join(ROOT, "tests", "host", "gzip_harness.cpp")
HOST_SRC = os.path.join(ROOT, "rufus_amd", "csrc", "rfx_host.cpp")
MiB = 1 << 20


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gzip") / ("harness_" + request.param))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", out, HARNESS_SRC, HOST_SRC]
    if request.param == "sanitized":
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        if subprocess.run(cmd, stderr=subprocess.DEVNULL).returncode == 0:
            return out
        cmd = cmd[:-2]  # (a compiler without the sanitizers: the plain build twice, as tests/test_bgzf_host.py does)
    subprocess.check_call(cmd)
    return out


def run(harness, d, args):
    r = subprocess.run([harness] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def core(harness, d, files, chunk, piece, arena=MiB):
    """{name: {"format": text | None, "crc", "bytes", "stats": dict, "starts": [bits], "prefilter", "probes"}}"""
    names = []
    for name, blob in files:
        names.append(name + ".gz")
        open(os.path.join(d, names[-1]), "wb").write(blob)
    r = run(harness, d, ["core", str(chunk), str(piece), str(arena)] + names)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    keys = ("found", "confirmed", "dropped", "inserted", "rounds", "members", "batches", "bytes")
    for line in r.stdout.decode().splitlines():
        w = line.split()
        if w[0] == "file":
            cur = out[w[1][:-3]] = {"format": None}
        elif w[0] == "format":
            cur["format"] = " ".join(w[2:])
        elif w[0] == "crc":
            cur["crc"], cur["bytes"] = int(w[1], 16), int(w[3])
        elif w[0] == "stats":
            cur["stats"] = dict(zip(keys, map(int, w[1:])))
        elif w[0] == "prefilter":
            cur["prefilter"], cur["probes"] = int(w[1]), int(w[3])
        elif w[0] == "starts":
            cur["starts"] = [int(x) for x in w[1:]]
        else:
            assert line == "guards ok", line
            cur["guards"] = True
    assert len(out) == len(files) and all(g.get("guards") for g in out.values())
    return out


@pytest.mark.parametrize("chunk,piece,arena", [(1024, 5000, MiB), (16384, 300000, MiB), (1 << 22, 1 << 23, 4 * MiB)])
def test_core_inflates_the_corpus_like_zlib(harness, tmp_path, chunk, piece, arena):
    """1 KiB: several chunks inside one 32 KiB window, a chunk's output under 32 KiB, pieces that end inside a block;
    4 MiB: a chunk larger than any file (a member is then ONE chunk, which must fit an arena: 4 MiB)."""
    corpus = G.corpus()
    got = core(harness, str(tmp_path), [(n, gz) for n, _, gz in corpus], chunk, piece, arena)
    for name, data, _ in corpus:
        g = got[name]
        assert g["format"] is None, (name, g["format"])
        assert (g["crc"], g["bytes"]) == (zlib.crc32(data), len(data)), name
        assert g["stats"]["bytes"] == len(data) and g["stats"]["confirmed"] == len(g["starts"]), name
    assert got["three_members"]["stats"]["members"] == 3
    assert got["fixed"]["stats"]["found"] == 0 and got["stored"]["stats"]["found"] == 0  # no candidate anywhere: one chunk
    assert got["fixed"]["stats"]["confirmed"] == 1
    if chunk == 1024:
        assert got["fastq_l6"]["stats"]["batches"] > 3  # 3.6 MB through an arena of 1 MiB
        assert got["planted"]["stats"]["dropped"] >= 1  # the finder reported the planted block, the chain dropped it
        assert got["full_flush"]["stats"]["confirmed"] >= 20  # a block per 10 KB of text: chunks under 32 KiB of output
    if chunk > MiB:
        # one chunk per member; the planted block is the one candidate of its file: dropped, and a chunk inserted behind it
        assert all(g["stats"]["confirmed"] == g["stats"]["members"] for n, g in got.items() if n != "planted")
        assert (got["planted"]["stats"]["dropped"], got["planted"]["stats"]["inserted"]) == (1, 1)


def test_confirmed_chunks_start_at_true_block_starts(harness, tmp_path):
    corpus = {n: (d, gz) for n, d, gz in G.corpus()}
    names = ("fastq_l6", "fastq_l1", "fastq_l9", "full_flush", "hand_window_edge", "planted")
    got = core(harness, str(tmp_path), [(n, corpus[n][1]) for n in names], 1024, MiB, arena=4 * MiB)
    for n in names:
        truth = G.file_block_starts(corpus[n][1])
        assert set(got[n]["starts"]) <= {b for b, _, _ in truth}, n
        dyn = [b for b, f, t in truth if f == 0 and t == 2]
        if n.startswith("fastq") or n == "full_flush":  # every true non-final dynamic start is found where chunks are tiny
            assert got[n]["stats"]["confirmed"] >= 0.75 * len(dyn), n
    # the match of distance 32768 at the very start of the second chunk: that chunk was cut where the hand-written block begins
    _, _, second_bit = G.hand_window_edge(np.random.default_rng(51))
    gz = corpus["hand_window_edge"][1]
    assert 8 * G.header_len(gz) + second_bit in got["hand_window_edge"]["starts"]
    # the planted block was reported by the finder, and is no chunk
    _, pgz, planted_bit = G.planted_false_positive(np.random.default_rng(0))
    g = core(harness, str(tmp_path), [("p", pgz)], 1024, MiB)["p"]
    assert g["stats"]["dropped"] >= 1 and planted_bit not in g["starts"] and g["format"] is None


def test_core_refuses_malformed_files(harness, tmp_path):
    cases = G.refusals()
    got = core(harness, str(tmp_path), cases, 1024, 7000)
    for name, _ in cases:
        assert got[name]["format"] is not None and got[name]["format"].startswith("rfx_gzip: member "), (name, got[name])
    assert "CRC mismatch" in got["crc_flipped"]["format"] and "ISIZE mismatch" in got["isize_wrong"]["format"]
    assert "member 1: no gzip member header" in got["second_member_bad_magic"]["format"]
    assert "member 0: no gzip member header" in got["reserved_flg_bit"]["format"]


def test_core_survives_seeded_damage(harness, tmp_path):
    """Each damaged file is refused with a status or yields exactly zlib's bytes."""
    cases = G.seeded_damage()
    assert len(cases) == 200
    got = core(harness, str(tmp_path), [(n, blob) for n, blob, _ in cases], 1024, 9000)
    passed = 0
    for name, _, want in cases:
        g = got[name]
        if g["format"] is None:
            assert want is not None and (g["crc"], g["bytes"]) == (zlib.crc32(want), len(want)), name
            passed += 1
        else:
            assert g["format"].startswith("rfx_gzip:"), name
    assert passed < 20


# ---- the ingest driver over host stand-ins ---------------------------------------------------------------------------------
def ingest(harness, d, files, arena, piece, chunk):
    names = []
    for i, blob in enumerate(files):
        names.append("in%d.gz" % i)
        open(os.path.join(d, names[-1]), "wb").write(blob)
    return run(harness, d, ["ingest", str(arena), str(piece), str(chunk)] + names)


def whole_records(text, n):
    """The first whole records of `text` within n bytes."""
    lines = text[:n].split(b"\n")
    return b"\n".join(lines[:(len(lines) - 1) // 4 * 4]) + b"\n"


@pytest.mark.parametrize("piece,chunk", [(300000, 16384), (1000, 1024)])
def test_ingest_carries_records_across_arenas_and_members(harness, tmp_path, piece, chunk):
    big = G.big_text()
    a, b = whole_records(big, 2500000), whole_records(big, 700000)[:-1]  # (the second file ends without its newline)
    c = whole_records(big, 400000)  # (fixed blocks: no chunk starts, so the member is one chunk and must fit an arena)
    two = G.member(a[:1200000], fname=b"x") + G.member(b"") + G.member(a[1200000:], level=1)
    r = ingest(harness, str(tmp_path), [two, G.member(b), G.member(c, strategy=zlib.Z_FIXED)], MiB, piece, chunk)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.decode().splitlines()
    text = a + b + b"\n" + c
    assert lines[-2] == "text crc %08x bytes %d records %d" % (zlib.crc32(text), len(text), text.count(b"\n") // 4)
    assert lines[-1] == "guards ok"
    arenas = [ln for ln in lines if ln.startswith("A ")]
    assert len(arenas) >= 5 and all(int(ln.split()[1]) <= MiB for ln in arenas)
    oks = [ln for ln in lines if ln.startswith("ok gzip route")]
    assert len(oks) == 3 and "members 3," in oks[0]


def test_ingest_refusals(harness, tmp_path):
    big = G.big_text()
    a = whole_records(big, 300000)
    good = G.member(a)
    r = ingest(harness, str(tmp_path), [good[:-8] + bytes([good[-8] ^ 4]) + good[-7:]], MiB, 100000, 16384)
    assert r.returncode == 1 and b"rufus_amd jellyfish count: rfx_gzip: member 0: CRC mismatch" in r.stderr, r.stderr[-500:]
    r = ingest(harness, str(tmp_path), [good[:len(good) // 2]], MiB, 100000, 16384)
    assert r.returncode == 1 and b"rufus_amd jellyfish count: rfx_gzip: member 0, chunk " in r.stderr and b"input exhausted" in r.stderr
    r = ingest(harness, str(tmp_path), [G.member(a[:-40])], MiB, 100000, 16384)  # the file ends inside a record
    assert r.returncode == 1 and b"strict 4-line FASTQ" in r.stderr, r.stderr[-500:]
    r = ingest(harness, str(tmp_path), [G.member(b"A" * (3 * MiB))], MiB, 100000, 16384)  # one chunk, larger than an arena
    assert r.returncode == 1 and b"does not fit an empty text arena" in r.stderr, r.stderr[-500:]
