"""GPU, through the executables: `jellyfish count --bam CHR --keep-packed CACHE X.bam` must count exactly what it counts
without the option and leave a cache that describes the file -- every kept record's address, name hash and filter arrays,
read back with tests/bam_cache_ref.py and held to tests/bam_ref.py and tests/filter_bam_ref.py -- and `RUFUS.Filter
--packed CACHE CHR HashList X.bam STUB ...` must write, byte for byte, the three files `RUFUS.Filter --bam` writes
(which tests/test_filter_bam_gpu.py holds to `--sam` and the oracle), while it inflates only the blocks of the hit names'
records.  Fails without the feature: `--bam --keep-packed` is refused."""
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle
from tests import bam_cache_ref as C
from tests import bam_ref as R
from tests import bgzf_ref as B
from tests import filter_bam_ref as FB
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
HL = os.path.join(R.GOLDEN, "Child.k25_c5.HashList")
SAMPLES = ("Child", "Mother", "Father")
UNUSABLE = b"is not a usable packed-read cache"
TRACE = re.compile(r"bam cache route: chunks (\d+) records (\d+) hits (\d+) names (\d+) selected (\d+) blocks (\d+) of (\d+) batches (\d+) "
                   r"pairs (\d+)")


def _count(d, out, inputs, extra=(), env=None):
    argv = [f"{BIN}/jellyfish", "count", "--disk", "-m", "25", "-L", "2", "-s", "100M", "-t", "6", "-o", out, "-C"] + list(extra) + list(inputs)
    return subprocess.run(argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _filter(d, route, args, stub, min_q=FB.MIN_Q, env=None):
    argv = [f"{BIN}/RUFUS.Filter", route] + list(args) + [stub, str(FB.K), str(min_q), str(FB.THRESH), "4"]
    return subprocess.run(argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _outputs(d, stub, chr_file):
    return [open(os.path.join(d, f), "rb").read() for f in (f"{stub}.Mutations.Mate1.fastq", f"{stub}.Mutations.Mate2.fastq", chr_file)]


def _payload_sha(path):
    blob = open(path, "rb").read()
    return hashlib.sha256(blob[9 + int(blob[:9]):]).hexdigest()


def _trace(r):
    m = TRACE.search(r.stderr.decode())
    assert m, r.stderr[-1500:]
    return dict(zip(("chunks", "records", "hits", "names", "selected", "blocks", "of", "batches", "pairs"), map(int, m.groups())))


def _two_routes(d, hl, min_q=FB.MIN_Q):
    """The three files of `--bam` on x.bam of directory d."""
    r = _filter(d, "--bam", ["bam.chr", hl, "x.bam"], "bam", min_q)
    assert r.returncode == 0, r.stderr[-1500:]
    return _outputs(d, "bam", "bam.chr")


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    """name -> (directory with x.bam, Bam, payload sha and chromosome log of the count without the option, --bam's three
    files, the cache `kp` of the count with the option at the default arena): once, shared."""
    out = {}
    for name in SAMPLES:
        d = str(tmp_path_factory.mktemp("cache_" + name))
        bam = R.Bam(R.fixture(name))
        open(f"{d}/x.bam", "wb").write(bam.bam)
        r = _count(d, "plain.Jhash", ["x.bam"], extra=["--bam", "plain.chr"])
        assert r.returncode == 0, r.stderr[-1500:]
        r = _count(d, "kept.Jhash", ["x.bam"], extra=["--bam", "kept.chr", "--keep-packed", "kp"])
        assert r.returncode == 0, r.stderr[-1500:]
        out[name] = (d, bam, _payload_sha(f"{d}/plain.Jhash"), open(f"{d}/plain.chr", "rb").read(), _two_routes(d, HL))
    return out


def _check_cache(blob, bam, min_q, multi_chunk):
    c = C.read(blob)
    kept = bam.kept()
    assert (c["min_q"], c["exclude_flags"], c["names"]) == (min_q, 3328, [n for n, _ in bam.refs])
    assert c["blocks"] == [(len(b), B.parts(b)[3]) for b in B.split(bam.bam)]
    assert (c["bam_bytes"], c["stream_bytes"]) == (len(bam.bam), len(bam.data))
    assert len(c["chunks"]) >= 2 if multi_chunk else len(c["chunks"]) == 1
    starts = np.concatenate([ch["stream_off"] + ch["start"].astype(np.int64) for ch in c["chunks"]])
    assert np.array_equal(starts, [r["start"] for r in kept])  # (across arenas: the carry arithmetic)
    assert np.array_equal(np.concatenate([ch["rbytes"] for ch in c["chunks"]]),
                          [4 + struct.unpack_from("<I", bam.data, r["start"])[0] for r in kept])
    assert np.array_equal(np.concatenate([ch["hash"] for ch in c["chunks"]]), np.array([FB.name_hash(FB.qname(r)) for r in kept], np.uint64))
    want = FB.packed(bam, min_q)
    n, nw = len(kept), int(want.word_off[len(kept)])
    assert np.array_equal(np.concatenate([ch["len"] for ch in c["chunks"]]), want.len[:n])
    assert np.array_equal(np.concatenate([ch["codes"] for ch in c["chunks"]]), want.codes[:nw])
    assert np.array_equal(np.concatenate([ch["good"] for ch in c["chunks"]]), want.good[:nw])
    at, runs = 0, []
    for ch in c["chunks"]:
        assert np.array_equal(ch["word_off"], want.word_off[at:at + len(ch["hash"]) + 1] - want.word_off[at])
        for first, ref in ch["runs"].reshape(-1, 2).tolist():
            ref = ref - (1 << 32) if ref >= 1 << 31 else ref
            if not runs or runs[-1][1] != ref:
                runs.append((at + first, ref))
        at += len(ch["hash"])
    assert runs == bam.runs()
    return c


@pytest.mark.parametrize("arena", [None, "1048576"])
@pytest.mark.parametrize("name", SAMPLES)
def test_count_keeps_a_cache_that_describes_the_file_and_the_filter_pulls_from_it(samples, tmp_path, name, arena):
    d0, bam, sha, log, want = samples[name]
    d, env = d0, None
    if arena:  # the count again with arenas of 1 MiB: the records' addresses cross arenas
        d, env = str(tmp_path), {"RFX_BAM_ARENA": arena}
        os.symlink(f"{d0}/x.bam", f"{d}/x.bam")
        r = _count(d, "kept.Jhash", ["x.bam"], extra=["--bam", "kept.chr", "--keep-packed", "kp"], env=env)
        assert r.returncode == 0, r.stderr[-1500:]
    assert _payload_sha(f"{d}/kept.Jhash") == sha and open(f"{d}/kept.chr", "rb").read() == log == bam.chr_log()
    _check_cache(open(f"{d}/kp", "rb").read(), bam, 15, arena is not None)
    r = _filter(d, "--packed", ["kp", "p.chr", HL, "x.bam"], "p", env=env)
    assert r.returncode == 0 and UNUSABLE not in r.stderr, r.stderr[-1500:]
    got = _outputs(d, "p", "p.chr")
    assert got == want
    t = _trace(r)
    assert t["records"] == len(bam.kept()) and t["pairs"] == got[0].count(b"\n") // 4 and t["selected"] >= 2 * t["pairs"]
    assert 0 < t["blocks"] and t["of"] == len(B.split(bam.bam))
    if name == "Child":
        assert t["pairs"] == 26


@pytest.fixture(scope="module")
def sparse(tmp_path_factory):
    """The crafted file re-cut into blocks of 4096 bytes: (directory with x.bam, hl and the cache kp; Bam; FB.expected; the
    number of blocks that hold a record of a hit name)."""
    blob, hl, _ = FB.crafted()
    bam = R.Bam(B.write(R.Bam(blob).data, cut=4096))
    d = str(tmp_path_factory.mktemp("sparse"))
    open(f"{d}/x.bam", "wb").write(bam.bam)
    open(f"{d}/hl", "wb").write(hl)
    r = _count(d, "kept.Jhash", ["x.bam"], extra=["--bam", "kept.chr", "--keep-packed", "kp"])
    assert r.returncode == 0, r.stderr[-1500:]
    fs = oracle.FilterSet(hl)
    kept = [(r, s) for r, s in zip(bam.records, bam.starts) if not r["flag"] & 3328]
    hashes = [FB.name_hash(FB.qname(r)) for r, _ in kept]
    printed = [(0, FB.qname(r)) + FB.stranded_printed(r) for r, _ in kept]
    hit = {h for p, h in zip(printed, hashes) if p[2] and FB.scan(fs, p) >= FB.THRESH}
    isizes = [B.parts(b)[3] for b in B.split(bam.bam)]
    blocks = {k for (r, s), h in zip(kept, hashes) if h in hit for k in C.blocks_of(isizes, s, 4 + struct.unpack_from("<I", bam.data, s)[0])}
    return d, bam, FB.expected(bam, hl), len(blocks)


@pytest.mark.parametrize("arena", [None, "1048576"])
def test_sparse_fetch_inflates_only_the_blocks_of_the_hit_names(sparse, arena):
    d, bam, (e1, e2, log, idx), n_blocks = sparse
    want = _two_routes(d, "hl")
    assert want == [e1, e2, log] and len(idx) >= 20
    r = _filter(d, "--packed", ["kp", "p.chr", "hl", "x.bam"], "p" + (arena or ""), env={"RFX_BAM_ARENA": arena} if arena else None)
    assert r.returncode == 0 and UNUSABLE not in r.stderr, r.stderr[-1500:]
    assert _outputs(d, "p" + (arena or ""), "p.chr") == want
    t = _trace(r)
    assert t["pairs"] == len(idx) and t["of"] == len(B.split(bam.bam))
    if arena is None:
        assert t["batches"] == 1 and t["blocks"] == n_blocks and t["blocks"] <= t["of"] // 4
    else:  # a block shared by two batches is inflated in both
        assert t["batches"] >= 2 and n_blocks <= t["blocks"] < t["of"]


def test_a_hash_list_that_hits_nothing(samples, tmp_path):
    d, bam, _, log, _ = samples["Father"]
    rng = np.random.default_rng(8)
    kmers = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 25)) for _ in range(4)]
    text = b"|".join(FB.stranded_printed(r)[0] for r in bam.kept())
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    assert not any(km in text or km.translate(comp)[::-1] in text for km in kmers)  # k-mers the file does not hold
    open(f"{tmp_path}/hl", "wb").write(b"".join(km + b" 7\n" for km in kmers))
    r = _filter(d, "--packed", ["kp", "none.chr", f"{tmp_path}/hl", "x.bam"], "none")
    assert r.returncode == 0 and UNUSABLE not in r.stderr, r.stderr[-1500:]
    assert _outputs(d, "none", "none.chr") == [b"", b"", log]
    t = _trace(r)
    assert (t["hits"], t["names"], t["selected"], t["blocks"], t["batches"], t["pairs"]) == (0, 0, 0, 0, 0, 0)
    assert t["records"] == len(bam.kept())


def test_fallbacks_to_the_two_pass_route(samples, tmp_path):
    d, bam, _, _, want = samples["Child"]
    blob = open(f"{d}/kp", "rb").read()
    # a hit record's own hash entry altered: the record fetched for it has another name
    fs = oracle.FilterSet(open(HL, "rb").read())
    kept = bam.kept()
    first_hit = next(i for i, r in enumerate(kept)
                     if FB.stranded_printed(r)[0] and FB.scan(fs, (0, FB.qname(r)) + FB.stranded_printed(r)) >= FB.THRESH)
    c = C.read(blob)
    c["chunks"][0]["hash"][first_hit] ^= np.uint64(1)
    open(f"{d}/altered", "wb").write(C.write(c))
    open(f"{d}/cut", "wb").write(blob[:-C.HEADER.size])
    r = _count(d, "q0.Jhash", ["x.bam"], extra=["--bam", "q0.chr", "--keep-packed", "kp_q0", "--keep-minq", "0"])
    assert r.returncode == 0, r.stderr[-1500:]
    assert C.read(open(f"{d}/kp_q0", "rb").read())["min_q"] == 0
    cases = {"Mother's cache": os.path.join(samples["Mother"][0], "kp"), "cut before its final header": "cut",
             "made for MinQ 0": "kp_q0", "a hit record's hash altered": "altered"}
    for i, (what, cache) in enumerate(cases.items()):
        r = _filter(d, "--packed", [cache, f"fb{i}.chr", HL, "x.bam"], f"fb{i}")
        assert r.returncode == 0 and r.stderr.count(UNUSABLE) == 1, (what, r.stderr[-1500:])
        assert _outputs(d, f"fb{i}", f"fb{i}.chr") == want, what
        assert b"bam filter route:" in r.stderr and b"bam cache route:" not in r.stderr, what
    # (the unaltered cache written back by the Python writer is used as it is)
    open(f"{d}/rewritten", "wb").write(C.write(C.read(blob)))
    r = _filter(d, "--packed", ["rewritten", "rw.chr", HL, "x.bam"], "rw")
    assert r.returncode == 0 and UNUSABLE not in r.stderr and _outputs(d, "rw", "rw.chr") == want


def test_refusals(samples, tmp_path):
    d0, bam, _, _, _ = samples["Father"]
    d = str(tmp_path)
    os.symlink(f"{d0}/x.bam", f"{d}/x.bam")
    os.symlink(f"{d0}/x.bam", f"{d}/y.bam")
    r = _count(d, "x.Jhash", ["x.bam", "y.bam"], extra=["--bam", "x.chr", "--keep-packed", "kp"])
    assert r.returncode != 0 and b"--keep-packed" in r.stderr and b"ONE input" in r.stderr, r.stderr[-1500:]
    r = _count(d, "x.Jhash", ["x.bam"], extra=["--bam", "x.chr", "--spool", "sp"])
    assert r.returncode != 0 and b"--bam" in r.stderr and b"one device" in r.stderr, r.stderr[-1500:]
    r = _count(d, "x.Jhash", ["x.bam"], extra=["--bam", "x.chr", "--keep-packed", "kp"], env={"RUFUS_GPUS": "0,0"})
    assert r.returncode != 0 and b"one device" in r.stderr, r.stderr[-1500:]
    r = _filter(d0, "--packed", ["kp", f"{d}/g.chr", HL, "x.bam"], f"{d}/g", env={"RUFUS_GPUS": "0,0"})
    assert r.returncode != 0 and b"one device" in r.stderr, r.stderr[-1500:]
    r = _count(d, "x.Jhash", ["x.bam"], extra=["--bam", "x.chr", "--keep-packed", "no_such_directory/kp"])
    assert r.returncode != 0 and b"packed-read cache" in r.stderr, r.stderr[-1500:]
