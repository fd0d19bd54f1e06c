"""Host: `RUFUS.Filter --bam` before it runs on a GPU.  The crafted file of tests/filter_bam_ref.py must hold what it says
it holds (so that the GPU tests cannot pass on an empty pull), and tests/host/filter_bam_harness.cpp -- the RFX_BAM_HD
functions of the stranded filter pack and the name hash, and the host printer and pairing walk of the route, built with
-fsanitize=address,undefined -- must give the host packer's arrays of the printed forms at MinQ 0, 15 and 42 and the
feeder's pairs filtered by the oracle, on bam_ref.synthetic(), bam_ref.adversarial() and the crafted file.
Not here: the executable's host pipeline over a stand-in device library (tests/fake_capi.py has no BAM entry points, and
carrying them would mean a copy of the kernels' logic in the stand-in)."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import bam_ref as R
from tests import filter_bam_ref as FB
from tests.conftest import ROOT

ARENA = 1 << 20


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fbam") / "filter_bam_harness")
    base = ["g++", "-O1", "-g", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "host", "filter_bam_harness.cpp")]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.check_call(base)
    return out


def _harness(harness, args):
    r = subprocess.run([harness] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-2000:]
    return r.stdout.decode()


@pytest.fixture(scope="module")
def files():
    """name -> (Bam, hash list, exclude flags, MinQ).  The files without a hash list get the windows of a few of their own
    paired reads; their qualities are random, so they are filtered at MinQ 0."""
    bam, hl, _ = FB.crafted()
    out = {"crafted": (R.Bam(bam), hl, 3328, FB.MIN_Q)}
    for name, b, exclude in (("synthetic", R.Bam(R.synthetic()), 3328), ("synthetic_all", None, 0), ("adversarial", R.Bam(R.adversarial()), 3328)):
        b = b or out["synthetic"][0]
        out[name] = (b, FB.own_hash_list(b, exclude), exclude, 0)
    return out


def test_the_crafted_file_holds_what_the_gpu_tests_rely_on():
    blob, hl, special = FB.crafted()
    bam = R.Bam(blob)
    assert 8000 <= len(bam.records) <= 10000 and 2 * ARENA < len(bam.data) < 3 * ARENA
    m1, m2, _ = FB.feeder_pairs(bam)
    _, _, _, idx = FB.expected(bam, hl)
    assert len(idx) >= 20 and len(idx) < len(m1) // 10  # a small share
    pulled = {m1[i][1]: (m1[i], m2[i]) for i in idx}
    # cross-arena pairs at 1 MiB arenas, in both orders: the hit record first, the hit record second
    kept_starts = [s for r, s in zip(bam.records, bam.starts) if not r["flag"] & 3328]
    fs = oracle.FilterSet(hl)
    orders = set()
    for name in special["cross"]:
        a, b = pulled[name]  # a: the later record
        assert (kept_starts[a[0]] - bam.first) // ARENA > (kept_starts[b[0]] - bam.first) // ARENA
        ha, hb = FB.scan(fs, a) >= FB.THRESH, FB.scan(fs, b) >= FB.THRESH
        assert ha != hb
        orders.add("second" if ha else "first")
    assert orders == {"first", "second"} and len(special["cross"]) >= 2
    # a pair whose only hit lies in a reverse-strand record with vanished bases, and only once they have closed up
    kept = bam.kept()
    for name in special["vanish"]:
        a, b = pulled[name]
        (hit,) = [x for x in (a, b) if FB.scan(fs, x) >= FB.THRESH]
        r = kept[hit[0]]
        assert r["flag"] & 16 and len(hit[2]) < r["l_seq"]
        kept_letters = "".join(FB._COMP.get(ord(c), "A") for c in reversed(r["seq"])).encode()  # nothing vanishes: no hit
        assert fs.scan(kept_letters, hit[3], FB.K, FB.MIN_Q) == 0
    # the cases by name
    names = [FB.qname(r) for r in kept]
    assert names.count(b"three") == 3 and b"three" in pulled and b"hit_alone" not in pulled and names.count(b"hit_alone") == 1
    assert b"pfx1" in pulled and b"pfx" not in pulled and b"pfx12" not in pulled and b"L" * 254 in pulled
    for fl in (256, 1024, 2048):
        assert sum(FB.qname(r) == b"excl%d" % fl for r in bam.records) == 3 and names.count(b"excl%d" % fl) == 2
        assert b"excl%d" % fl in pulled
    assert {r["l_seq"] for r in kept} >= set(FB.EDGE_L)
    assert any(r["l_seq"] and r["qual"][0] == 0xFF for r in kept)
    assert any(r["flag"] & 16 and set(r["seq"]) - set("ACGTN*") for r in kept)
    assert len(bam.runs()) >= 8 and any(ref == -1 for _, ref in bam.runs())


@pytest.mark.parametrize("name", ["crafted", "synthetic", "synthetic_all", "adversarial"])
def test_pack_and_hashes_equal_the_host_packer_of_the_printed_forms(harness, files, tmp_path, name):
    bam, _, exclude, _ = files[name]
    src = tmp_path / "in.bin"
    src.write_bytes(bam.data)
    kept = bam.kept(exclude)
    for min_q in (0, 15, 42):
        out = str(tmp_path / f"p{min_q}")
        assert _harness(harness, ["pack", src, bam.first, len(bam.refs), exclude, min_q, out]).startswith("ok")
        want = FB.packed(bam, min_q, exclude)
        nw = int(want.word_off[-1])
        assert np.array_equal(np.fromfile(out + ".len", np.uint32), want.len[:len(kept)])
        assert np.array_equal(np.fromfile(out + ".codes", np.uint64), want.codes[:nw])
        assert np.array_equal(np.fromfile(out + ".good", np.uint32), want.good[:nw])
    assert np.fromfile(out + ".hash", np.uint64).tolist() == [FB.name_hash(FB.qname(r)) for r in kept]


@pytest.mark.parametrize("name", ["crafted", "synthetic", "adversarial"])
@pytest.mark.parametrize("subset", [False, True])
def test_printer_and_pairing_walk_equal_the_feeder_and_the_oracle(harness, files, tmp_path, name, subset):
    bam, hl, exclude, min_q = files[name]
    src, flags = tmp_path / "in.bin", tmp_path / "flags.bin"
    src.write_bytes(bam.data)
    fs = oracle.FilterSet(hl)
    kept = bam.kept(exclude)
    hit = [fs.scan(*FB.stranded_printed(r), FB.K, min_q) >= FB.THRESH for r in kept]
    # the subset the route's second pass gathers: every record whose name hash is a hit record's
    hashes = {FB.name_hash(FB.qname(r)) for r, h in zip(kept, hit) if h}
    take = [not subset or FB.name_hash(FB.qname(r)) in hashes for r in kept]
    flags.write_bytes(bytes(int(h) | 2 * int(t) for h, t in zip(hit, take)))
    out = str(tmp_path / "o")
    assert _harness(harness, ["pairs", src, bam.first, len(bam.refs), exclude, flags, out]).startswith("ok")
    e1, e2, _, idx = FB.expected(bam, hl, exclude, min_q=min_q)
    assert len(idx) >= 3
    assert open(out + ".m1", "rb").read() == e1 and open(out + ".m2", "rb").read() == e2
