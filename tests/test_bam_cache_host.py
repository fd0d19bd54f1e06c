"""Host: the BAM-kind packed-read cache (rufus_amd/csrc/host/rfx_bam_cache.hpp) before an executable uses it.
tests/host/bam_cache_harness.cpp -- a stand-alone program over the header, built with -fsanitize=address,undefined -- plans
fetches that a brute-force Python statement accepts, reads and writes the format exactly as tests/bam_cache_ref.py (written
from the header's description) does, and refuses every damaged file.  The fixture check at the end keeps the GPU test of the
sparse fetch from passing trivially.  Fails without the feature: the header does not exist."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_cache_ref as C
from tests import bam_ref as R
from tests import bgzf_ref as B
from tests import filter_bam_ref as FB
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bamcache") / "bam_cache_harness")
    base = ["g++", "-O1", "-g", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "host", "bam_cache_harness.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(base)
    return out


def _harness(harness, args):
    r = subprocess.run([harness] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    return r.stdout.decode()


# ---- plan_fetch -----------------------------------------------------------------------------------------------------
def _random_case(rng):
    """(isizes, records ascending) -- blocks of ISIZE 0 (in the middle and at the end), 1, 1024 and 65536; records over one,
    two and three blocks, from a block's first byte, to a block's last byte, side by side and identical."""
    isizes = [int(x) for x in rng.choice([0, 1, 1024, 1024, 1024, 65536], int(rng.integers(6, 30)))]
    isizes += [1024, 0, 1024, 1024, 1, 1, 1024, 0]
    starts = np.concatenate([[0], np.cumsum(isizes)])
    total = int(starts[-1])
    full = [i for i, n in enumerate(isizes) if n]
    recs = []
    for _ in range(int(rng.integers(1, 40))):
        j = int(rng.integers(0, len(full)))
        span = int(rng.integers(1, 4))
        first, last = full[j], full[min(j + span - 1, len(full) - 1)]
        lo, hi = int(starts[first]), int(starts[last + 1])  # the bytes of `span` blocks
        kind = int(rng.integers(0, 4))
        a = lo if kind in (0, 2) else int(rng.integers(lo, min(lo + isizes[first], hi)))
        e = hi if kind in (1, 2) else int(rng.integers(max(a + 1, int(starts[last]) + 1), hi + 1))
        recs.append((a, e - a))
        if rng.random() < 0.2:
            recs.append((a, e - a))                       # identical
        if rng.random() < 0.2 and e < total:
            recs.append((e, min(int(rng.integers(1, 3000)), total - e)))  # side by side
    return isizes, sorted(recs, key=lambda r: r[0])


def _plan(harness, tmp_path, isizes, recs, cap):
    path = tmp_path / "plan.txt"
    path.write_text("%d\n" % len(isizes) + "".join("%d %d\n" % (28 + n // 3, n) for n in isizes) + "%d\n" % len(recs) +
                    "".join("%d %d\n" % r for r in recs))
    out = _harness(harness, ["plan", path, cap]).splitlines()
    if out and out[0].startswith("error"):
        return out[0]
    batches = []
    for i in range(0, len(out), 3):
        _, inflated, first, n = out[i].split()
        batches.append((int(inflated), int(first), int(n), [int(x) for x in out[i + 1].split()[1:]], [int(x) for x in out[i + 2].split()[1:]]))
    return batches


def test_plan_fetch_against_the_brute_force_statement(harness, tmp_path):
    rng = np.random.default_rng(41)
    seen_spans, multi = set(), 0
    for case in range(25):
        isizes, recs = _random_case(rng)
        stream = rng.integers(0, 256, sum(isizes), dtype=np.uint8).tobytes()
        own = [sum(isizes[k] for k in C.blocks_of(isizes, a, n)) for a, n in recs]
        seen_spans.update(len(C.blocks_of(isizes, a, n)) for a, n in recs)
        everything = sum(isizes[k] for k in {k for a, n in recs for k in C.blocks_of(isizes, a, n)})
        for cap in sorted({max(own), max(own) + 1, (max(own) + everything) // 2, everything, everything + 5}):
            batches = _plan(harness, tmp_path, isizes, recs, cap)
            assert isinstance(batches, list), (case, cap, batches)
            C.check_plan(isizes, recs, cap, batches, stream)
            multi += len(batches) > 1
            if cap >= everything:
                assert len(batches) == 1
        # one byte less than the largest record's blocks: that record is refused, by its index
        worst = own.index(max(own))
        assert _plan(harness, tmp_path, isizes, recs, max(own) - 1) == "error record %d: its blocks exceed the arena" % worst
    assert seen_spans >= {1, 2, 3} and multi >= 10
    # not ascending, and outside the stream
    assert _plan(harness, tmp_path, [1024, 1024], [(100, 10), (99, 10)], 4096).startswith("error record 1: not ascending")
    assert _plan(harness, tmp_path, [1024, 1024], [(2040, 9)], 4096).startswith("error record 0: outside the stream")
    assert _plan(harness, tmp_path, [1024, 1024], [], 4096) == []


# ---- round trip and refusals ------------------------------------------------------------------------------------------
MIN_Q = 15


@pytest.fixture(scope="module")
def content():
    """The cache of bam_ref.synthetic() in three chunks, as the count would leave it."""
    bam = R.Bam(R.synthetic())
    kept = bam.kept()
    packed = FB.packed(bam, MIN_Q)
    hashes = np.array([FB.name_hash(FB.qname(r)) for r in kept], np.uint64)
    starts = np.array([r["start"] for r in kept], np.int64)
    sizes = np.array([4 + struct.unpack_from("<I", bam.data, r["start"])[0] for r in kept], np.int64)
    chunks = []
    cuts = [0, len(kept) // 3, len(kept) // 3 + 1, len(kept)]
    for a, b in zip(cuts, cuts[1:]):
        base = int(starts[a]) - 5 * (a > 0)
        w0, w1 = int(packed.word_off[a]), int(packed.word_off[b])
        runs = []
        for i in range(a, b):
            if i == a or kept[i]["ref_id"] != kept[i - 1]["ref_id"]:
                runs += [i - a, kept[i]["ref_id"] & 0xFFFFFFFF]
        chunks.append({"stream_off": base, "hash": hashes[a:b], "start": (starts[a:b] - base).astype(np.uint32),
                       "rbytes": sizes[a:b].astype(np.uint32), "len": packed.len[a:b], "word_off": packed.word_off[a:b + 1] - w0,
                       "codes": packed.codes[w0:w1], "good": packed.good[w0:w1], "runs": np.array(runs, np.uint32)})
    blocks = [(len(blk), B.parts(blk)[3]) for blk in B.split(bam.bam)]
    return {"min_q": MIN_Q, "exclude_flags": 3328, "names": [n for n, _ in bam.refs], "chunks": chunks, "blocks": blocks}


def test_round_trip_python_and_cpp(harness, content, tmp_path):
    blob = C.write(content)
    assert C.same(C.read(blob), content)
    (tmp_path / "a").write_bytes(blob)
    line = _harness(harness, ["read", tmp_path / "a"]).split()
    n, words = sum(len(c["hash"]) for c in content["chunks"]), sum(len(c["codes"]) for c in content["chunks"])
    assert line[:11] == ["ok", "chunks", "3", "records", str(n), "blocks", str(len(content["blocks"])), "names", "5", "words", str(words)]
    assert line[11:15] == ["min_q", str(MIN_Q), "exclude", "3328"]
    # the C++ reader's parts through the C++ writer: the same bytes, which Python reads back as the content
    assert _harness(harness, ["copy", tmp_path / "a", tmp_path / "b"]).strip() == "ok"
    again = (tmp_path / "b").read_bytes()
    assert again == blob and C.same(C.read(again), content)
    # either reader refuses the other kind
    assert _harness(harness, ["sam", tmp_path / "a"]).strip() == "refused"


def _refused(harness, tmp_path, blobs):
    paths = []
    for i, b in enumerate(blobs):
        p = tmp_path / ("r%d" % i)
        p.write_bytes(b)
        paths.append(p)
    return _harness(harness, ["read"] + paths).split("\n")[:-1]


def test_refusals(harness, content, tmp_path):
    blob = C.write(content)
    good = C.read(blob)
    H = C.HEADER.size
    # the boundaries: header, names, every chunk, the index, the last header
    bounds, at = [0, H], H + sum(len(n) + 1 for n in content["names"])
    at += -at % 8
    bounds.append(at)
    for i, ch in enumerate(content["chunks"]):
        at += len(C.chunk_bytes(i, ch))
        bounds.append(at)
    assert at == good["index_off"]
    bounds += [at + 16, len(blob) - H, len(blob) - 8]
    cuts = sorted({max(b + d, 0) for b in bounds for d in (-8, -1, 0, 1, 8)} - {len(blob)})
    assert all(line == "refused" for line in _refused(harness, tmp_path, [blob[:c] for c in cuts]))
    # a cut file with a whole header pasted behind it is no cache either
    assert _refused(harness, tmp_path, [blob[:bounds[4]] + blob[:H]]) == ["refused"]

    def patched(at, fmt, value):
        b = bytearray(blob)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    def both(at, fmt, value):  # the same field of the header at the start and of the one behind the index
        b = bytearray(blob)
        for base in (0, len(blob) - H):
            struct.pack_into(fmt, b, base + at, value)
        return bytes(b)

    done_at, bam_bytes_at = 16, 24
    beyond = dict(content, chunks=[dict(c) for c in content["chunks"]])
    last = beyond["chunks"][-1]
    last["rbytes"] = last["rbytes"].copy()
    last["rbytes"][-1] = good["stream_bytes"] + 1 - last["stream_off"] - int(last["start"][-1])
    exact = dict(content, chunks=[dict(c) for c in content["chunks"]])
    exact["chunks"][-1]["rbytes"] = last["rbytes"] - np.array([0] * (len(last["rbytes"]) - 1) + [1], np.uint32)
    entry = good["index_off"] + 16 + 24 * 3
    bad_woff = dict(content, chunks=[dict(c) for c in content["chunks"]])
    bad_woff["chunks"][0]["word_off"] = bad_woff["chunks"][0]["word_off"].copy()
    bad_woff["chunks"][0]["word_off"][5] = bad_woff["chunks"][0]["word_off"][6] + 1
    cases = {"done missing in both headers": both(done_at, "<Q", 0), "done missing in the first header": patched(done_at, "<Q", 0),
             "a SAM-kind magic": both(0, "<Q", C.SAM_FILE_MAGIC), "a record one byte beyond the stream": C.write(beyond),
             "a gap in the block index": patched(entry, "<Q", struct.unpack_from("<Q", blob, entry)[0] + 1),
             "a gap in the inflated offsets": patched(entry + 8, "<Q", struct.unpack_from("<Q", blob, entry + 8)[0] + 1),
             "the index ends in front of the BAM's size": both(bam_bytes_at, "<Q", good["bam_bytes"] + 1),
             "word_off not monotone": C.write(bad_woff), "a chunk magic": patched(bounds[2], "<Q", C.SAM_FILE_MAGIC)}
    got = _refused(harness, tmp_path, list(cases.values()))
    assert got == ["refused"] * len(cases), dict(zip(cases, got))
    # (the record that ends exactly with the stream is accepted: the bound is the stream's length, not one less)
    assert _refused(harness, tmp_path, [C.write(exact)])[0].startswith("ok ")
    # 200 seeded byte flips: refused, or read to the end without a sanitizer report (_harness asserts that)
    rng = np.random.default_rng(43)
    flips = []
    for _ in range(200):
        b = bytearray(blob)
        region = int(rng.integers(0, 3))  # headers and chunk headers are few bytes of many: aim at them too
        at = int(rng.integers(0, H)) if region == 0 else int(rng.choice(bounds[2:-2])) + int(rng.integers(0, 48)) if region == 1 else \
            int(rng.integers(0, len(b)))
        b[min(at, len(b) - 1)] ^= 1 << int(rng.integers(0, 8))
        flips.append(bytes(b))
    got = _refused(harness, tmp_path, flips)
    assert len(got) == 200 and all(g == "refused" or g.startswith("ok ") for g in got)
    assert sum(g == "refused" for g in got) >= 40


# ---- the fixture of the sparse-fetch GPU test -------------------------------------------------------------------------
def test_the_recut_crafted_file_is_sparse_in_the_blocks_of_its_hit_names():
    import oracle
    blob, hl, _ = FB.crafted()
    bam = R.Bam(blob)
    recut = R.Bam(B.write(bam.data, cut=4096))
    assert recut.data == bam.data and recut.starts == bam.starts
    payload = [n for n in (B.parts(b)[3] for b in B.split(recut.bam)) if n]
    fs = oracle.FilterSet(hl)
    kept = [(r, s) for r, s in zip(recut.records, recut.starts) if not r["flag"] & 3328]
    hashes = [FB.name_hash(FB.qname(r)) for r, _ in kept]
    printed = [(0, FB.qname(r)) + FB.stranded_printed(r) for r, _ in kept]
    hit = {h for p, h in zip(printed, hashes) if p[2] and FB.scan(fs, p) >= FB.THRESH}
    selected = [(s, 4 + struct.unpack_from("<I", recut.data, s)[0]) for (r, s), h in zip(kept, hashes) if h in hit]
    blocks = {k for s, n in selected for k in C.blocks_of(payload, s, n)}
    straddlers = sum(1 for s, n in selected if len(C.blocks_of(payload, s, n)) > 1)
    assert len(hit) >= 20
    assert len(blocks) <= len(payload) // 4 and straddlers >= 5, (len(selected), len(blocks), len(payload), straddlers)
