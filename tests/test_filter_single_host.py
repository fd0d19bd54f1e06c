"""CPU: what the `RUFUS.Filter.single --bam` GPU tests stand on.

1. The crafted file of tests/filter_single_ref.py holds every case by name, on the oracle's word.
2. The Python statement (filter_single_ref.expected_single) is pinned to the reference's own two processes,
   `oracle/_ref/PassThroughSamCheck.stranded.se | oracle/_ref/RUFUS.Filter.single ... 1`, on the three testRun BAMs and on
   the crafted file's clean subset, and to tests/golden/testRun/expected_single_bam.json.
3. tests/host/filter_single_harness.cpp: the route's host tail (rufus_amd/csrc/host/rfx_bam_single.hpp: the stranded printer
   and the `:MH` formatting) as it is, under AddressSanitizer and UBSan, over gathered-record bytes in exact-size heap
   copies -- hit counts of one to ten digits, truncated and inconsistent input refused and never read past.
Tests 1 and 2 pass without the feature by design: they check the reference side."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle
from tests import bam_ref as R
from tests import filter_bam_ref as FB
from tests import filter_single_ref as S
from tests.conftest import ROOT, require_ref
from tests.golden.make_golden_single_bam import reference_single, summary

HL = os.path.join(R.GOLDEN, "Child.k25_c5.HashList")


@pytest.fixture(scope="module")
def crafted():
    blob, hl, special = S.crafted_single()
    bam = R.Bam(blob)
    return bam, hl, special, S.expected_single(bam, hl)


def test_the_crafted_file_holds_what_the_gpu_tests_rely_on(crafted):
    bam, hl, special, (text, log, idx, hits) = crafted
    kept = bam.kept()
    at = {}
    for i, r in enumerate(kept):
        at.setdefault(FB.qname(r), []).append(i)

    def one(case):
        assert len(at[special[case]]) == 1, case
        return at[special[case]][0]

    assert len(bam.data) > 1 << 20 and 4400 <= len(kept) == len(bam.records) - 1
    sizes = np.diff(bam.starts + [len(bam.data)])
    assert 260 <= float(np.mean(sizes)) <= 290
    paired = oracle.FilterSet(hl)
    # the last base: the paired scan never examines it
    i = one("last_base")
    assert hits[i] == 1 and S.single_scan(paired, kept[i], single_end=False) == 0 and not kept[i]["flag"] & 16
    # vanished IUPAC bases close up on the reverse strand only
    i, j = one("vanish_hit"), one("iupac_fwd")
    assert kept[i]["flag"] & 16 and hits[i] == 6 and hits[j] == 0 and kept[i]["seq"] == kept[j]["seq"]
    assert set(kept[i]["seq"]) - set("ACGT") == set("RYK")
    # one, two and three digits of :MH
    assert [hits[one(c)] for c in ("hits1", "hits2", "hits40", "hits126", "hits126_rev")] == [1, 2, 40, 126, 126]
    for c, digits in (("hits1", b":MH1\n"), ("hits40", b":MH40\n"), ("hits126", b":MH126\n")):
        assert b"@" + special[c] + digits in text
    # spoiled windows
    i, j = one("low_q_spoils"), one("n_spoils")
    assert hits[i] == 0 and hits[j] == 0 and "N" in kept[j]["seq"] and min(kept[i]["qual"]) == S.MIN_Q - 1
    assert S.single_scan(oracle.FilterSet(hl, single_end=True), kept[i], min_q=S.MIN_Q - 1) == 1
    assert kept[i]["seq"].replace("N", "") != kept[j]["seq"] and sum(a != b for a, b in zip(kept[i]["seq"], kept[j]["seq"])) == 1
    # `*`, forward and reverse; no qualities; an excluded flag
    i, j = one("star_fwd"), one("star_rev")
    assert kept[i]["l_seq"] == 0 == kept[j]["l_seq"] and not kept[i]["flag"] & 16 and kept[j]["flag"] & 16
    assert FB.stranded_printed(kept[i]) == (b"*", b"*") and FB.stranded_printed(kept[j]) == (b"", b"*")
    i = one("noqual_would_hit")
    assert kept[i]["qual"][0] == 0xFF and hits[i] == 0
    with_q = dict(kept[i], qual=bytes([30]) * kept[i]["l_seq"])
    assert S.single_scan(oracle.FilterSet(hl, single_end=True), with_q) == 5
    excl = [r for r in bam.records if r["flag"] & 3328]
    assert len(excl) == 1 and excl[0]["name"] == special["excluded_would_hit"] and special["excluded_would_hit"] not in at
    assert S.single_scan(oracle.FilterSet(hl, single_end=True), excl[0]) == 5
    assert bam.records.index(excl[0]) == S.EXCLUDED_AT > 65
    # two records of one name, both written
    assert [hits[i] for i in at[b"twin"]] == [2, 4] and text.count(b"@twin:MH") == 2
    # the edges of a wave, the ends of the file
    assert {0, 63, 64, 65, len(kept) - 1} <= set(idx)
    # a selected record across every BGZF block boundary: an arena is cut at one of them
    inflated_cuts = set(bam.block_starts[1:])
    straddlers = [i for i, r in enumerate(kept) if any(r["start"] < c < r["start"] + int(sizes[bam.records.index(r)]) for c in inflated_cuts)]
    assert len(straddlers) >= 15 and set(straddlers) <= set(idx)
    assert any(c > (1 << 20) - 65536 * 4 for c in inflated_cuts)
    # ... and right where the refID changes
    runs = [i for i, _ in bam.runs()]
    assert len(runs) == 6 and set(runs[1:]) <= set(idx) and log == bam.chr_log() == b"notachr\nchr1\nchr2\nchr3\nchr4\nchr5\n*\n"
    assert {s % 4 for s in bam.starts} == {0, 1, 2, 3} and {len(FB.qname(r)) % 4 for r in kept} == {0, 1, 2, 3}
    # between 10 and 30 % are selected at Threshold 1, strictly fewer at 2
    assert 0.10 <= len(idx) / len(kept) <= 0.30
    idx2 = S.expected_single(bam, hl, thresh=2)[2]
    assert 0 < len(idx2) < len(idx) and set(idx2) < set(idx)


@pytest.mark.parametrize("name", ["Child", "Mother", "Father"])
def test_the_python_statement_is_the_reference_on_the_fixtures(name):
    require_ref("RUFUS.Filter.single")
    require_ref("PassThroughSamCheck.stranded.se")
    bam = R.Bam(R.fixture(name))
    hl = open(HL, "rb").read()
    text, log, idx, hits = S.expected_single(bam, hl)
    ref_text, ref_log = reference_single(bam.sam_text(), HL)
    assert (text, log) == (ref_text, ref_log)
    golden = json.load(open(os.path.join(R.GOLDEN, "expected_single_bam.json")))[name]
    assert summary(text, log) == golden
    assert golden["fastq_sha256"] == hashlib.sha256(text).hexdigest() and len(golden["names"]) == len(idx)
    if name == "Child":
        assert len(idx) >= 26
        # the pulled pairs of the paired route are a subset: a pair is pulled for a record the single-end scan selects too
        m1, m2, _ = FB.feeder_pairs(bam)
        _, _, _, pairs = FB.expected(bam, hl)
        assert len(pairs) == 26
        selected = {FB.qname(bam.kept()[i]) for i in idx}
        assert {m1[p][1] for p in pairs} <= selected


def test_the_python_statement_is_the_reference_on_the_crafted_clean_subset(crafted, tmp_path):
    require_ref("RUFUS.Filter.single")
    require_ref("PassThroughSamCheck.stranded.se")
    bam, hl, _, _ = crafted
    clean = R.Bam(S.clean_subset(bam))
    assert len(bam.kept()) - 10 < len(clean.records) < len(bam.kept())
    (tmp_path / "hl").write_bytes(hl)
    for thresh in (1, 2):
        text, log, idx, _ = S.expected_single(clean, hl, thresh=thresh)
        assert (text, log) == reference_single(clean.sam_text(), str(tmp_path / "hl"), thresh=thresh) and len(idx) > 400


# ---- the host side under the sanitizers: a stand-alone program, nothing loaded into python --------------------------------
HARNESS_SRC = [os.path.join(ROOT, "tests", "host", "filter_single_harness.cpp"), os.path.join(ROOT, "rufus_amd", "csrc", "rfx_host.cpp")]


def _build(tmp_path_factory, tag, flags):
    exe = str(tmp_path_factory.mktemp("single_" + tag) / "filter_single_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-DRFX_SINGLE_END"] + flags + ["-o", exe] + HARNESS_SRC, check=True,
                   timeout=600)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory, "asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def harness_tsan(tmp_path_factory):
    return _build(tmp_path_factory, "tsan", ["-fsanitize=thread"])


def _run(harness, d, records, hits):
    """The harness's tail over `records` (raw gathered-record bytes, one behind the other) with the counts `hits`."""
    open(f"{d}/in.bin", "wb").write(records)
    open(f"{d}/hits.bin", "wb").write(struct.pack("<%dI" % len(hits), *hits))
    return subprocess.run([harness, "--tail", f"{d}/in.bin", f"{d}/hits.bin", f"{d}/out.fastq"], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("sanitizer", ["asan_ubsan", "tsan"])
def test_filter_single_sam_host_side_equals_the_statement(harness, harness_tsan, tmp_path, sanitizer):
    """`RUFUS.Filter.single --sam`'s own main() over host stand-ins for the device: reader, helper threads, recycled pieces of
    16 KB, the ordered `:MH` output -- a shuffled SAM of 6000 names with IUPAC and lower-case bases on both strands and
    quality strings shorter than their read, from a pipe and from a file, Threads 1 and 5."""
    from tests.test_filter_sam_host import _hash_list, _shuffled_sam
    exe = harness if sanitizer == "asan_ubsan" else harness_tsan
    d = str(tmp_path)
    rng = np.random.default_rng(5)
    sam = _shuffled_sam(rng)
    hl = _hash_list(rng, sam, 1500)
    open(f"{d}/in.sam", "wb").write(sam)
    open(f"{d}/hl", "wb").write(hl)
    env = dict(os.environ, RFX_INGEST_PIECE="16384")
    n_written = {t: S.expected_single_sam(sam, hl, thresh=t)[0].count(b"\n") // 4 for t in (1, 2)}
    assert n_written[1] >= 20 and 0 < n_written[2] < n_written[1]  # (a selection worth the name at both thresholds)
    for thresh in (1, 2):
        want = S.expected_single_sam(sam, hl, thresh=thresh)
        for stub, src, threads in (("p1", "stdin", "1"), ("p5", "stdin", "5"), ("f5", "in.sam", "5")):
            r = subprocess.run([exe, "--sam", f"{stub}.chr", "hl", src, stub, str(S.K), str(S.MIN_Q), str(thresh), threads], cwd=d, env=env,
                               input=sam if src == "stdin" else None, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            assert r.returncode == 0 and b"Sanitizer" not in r.stderr, r.stderr[-2000:]
            assert (open(f"{d}/{stub}.Mutations.fastq", "rb").read(), open(f"{d}/{stub}.chr", "rb").read()) == want, (stub, thresh)
            assert not os.path.exists(f"{d}/{stub}.Mutations.Mate1.fastq")


@pytest.mark.parametrize("name", ["synthetic", "adversarial", "crafted"])
def test_tail_prints_what_the_statement_prints_under_asan_ubsan(harness, tmp_path, name):
    bam = R.Bam({"synthetic": R.synthetic, "adversarial": R.adversarial, "crafted": lambda: S.crafted_single()[0]}[name]())
    kept = bam.kept(0)[:1500]
    slices = FB.record_slices(bam, 0)[:1500]
    values = (0, 1, 9, 10, 99, 100, 4294967295)
    hits = [values[i % len(values)] for i in range(len(kept))]
    r = _run(harness, str(tmp_path), b"".join(slices), hits)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "out.fastq").read_bytes() == b"".join(S.fastq_mh(rec, h) for rec, h in zip(kept, hits))
    assert any(FB.stranded_printed(rec)[0] == b"" for rec in kept) or name == "adversarial"  # the empty sequence line is printed


def test_tail_refuses_truncated_and_inconsistent_records(harness, tmp_path):
    bam = R.Bam(R.synthetic())
    slices = FB.record_slices(bam, 0)[:40]
    whole = b"".join(slices)
    d = str(tmp_path)
    for cut in (1, 3, 4, 20, 35, 36, len(slices[-1]) - 1):  # the last record cut: inside block_size, the fixed fields, the body
        r = _run(harness, d, whole[:len(whole) - len(slices[-1]) + cut], [1] * 40)
        assert r.returncode == 3 and b"cut by the end" in r.stderr and b"Sanitizer" not in r.stderr, (cut, r.stderr[-800:])
    # a length word that disagrees: one byte more (the next record's fields are then garbage), and far too large
    for delta in (1, 1 << 20):
        bad = bytearray(whole)
        at = sum(map(len, slices[:10]))
        bad[at:at + 4] = struct.pack("<I", struct.unpack_from("<I", bad, at)[0] + delta)
        r = _run(harness, d, bytes(bad), [1] * 40)
        assert r.returncode == 3 and b"rfx_bam_single" in r.stderr and b"Sanitizer" not in r.stderr, r.stderr[-800:]
    # fewer counts than records: the bytes do not add up
    r = _run(harness, d, whole, [1] * 39)
    assert r.returncode == 3 and b"do not add up" in r.stderr
