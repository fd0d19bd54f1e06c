"""CPU-only: the FASTA rule the kernels of rufus_amd/csrc/rfx_fasta.hip run (rufus_amd/csrc/rfx_fasta_core.h, one source
for host and device) and the FASTA mode of the ingest class of `jellyfish count` (rufus_amd/csrc/host/rfx_ingest.hpp,
BgzfIngest) through tests/host/fasta_harness.cpp: a stand-alone program, built plain and with
-fsanitize=address,undefined and run directly.  The reference is tools.parse_sequences and the packer of
tests/fasta_ref.py.  The real library and executable are compared in tests/test_fasta_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

from rufus_amd import tools
from tests import bgzf_ref as B
from tests import fasta_ref as F
from tests.conftest import ROOT

HARNESS_SRC = os.path.join(ROOT, "tests", "host", "fasta_harness.cpp")
HOST_SRC = os.path.join(ROOT, "rufus_amd", "csrc", "rfx_host.cpp")
ARENA = 4096


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fasta") / ("harness_" + request.param))
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


def parse_core_line(line):
    """'T bytes fasta n N max M len .. off .. codes .. mask ..' -> (bytes, None | dict)"""
    w = line.split()
    assert w[0] == b"T"
    if w[2] == b"0":
        return int(w[1]), None
    at = {k: w.index(k) for k in (b"len", b"off", b"codes", b"mask")}
    return int(w[1]), {"n": int(w[4]), "max_len": int(w[6]),
                       "len": np.array([int(x) for x in w[at[b"len"] + 1:at[b"off"]]], np.uint32),
                       "word_off": np.array([int(x) for x in w[at[b"off"] + 1:at[b"codes"]]], np.uint32),
                       "codes": np.array([int(x, 16) for x in w[at[b"codes"] + 1:at[b"mask"]]], np.uint64),
                       "acgt": np.array([int(x, 16) for x in w[at[b"mask"] + 1:]], np.uint32)}


def same(got, text, what):
    if text[:1] != b">":
        assert got is None, what
        return
    want = F.pack(tools.parse_sequences(text))
    assert got is not None and got["n"] == len(want["len"]) and got["max_len"] == want["max_len"], what
    for key in ("len", "word_off", "codes", "acgt"):
        assert np.array_equal(got[key], want[key]), (what, key)


def test_core_joins_and_packs_like_the_reference_parser(harness, tmp_path):
    d = str(tmp_path)
    cases = F.cases() + [("empty", b""), ("not FASTA", b"ACGT\n>x\nAC\n"), ("a FASTQ record", b"@r\nACGT\n+\nIIII\n")]
    for i, (_, text) in enumerate(cases):
        open(f"{d}/t{i}", "wb").write(text)
    r = run(harness, d, ["core"] + [f"t{i}" for i in range(len(cases))])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (name, text), line in zip(cases, lines):
        n, got = parse_core_line(line)
        assert n == len(text), name
        same(got, text, name)


def test_core_on_every_prefix_of_a_small_text(harness, tmp_path):
    d = str(tmp_path)
    text = F.small_text()
    open(f"{d}/small", "wb").write(text)
    r = run(harness, d, ["core", "--trunc", "small"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(text) + 1
    for n, line in enumerate(lines):
        m, got = parse_core_line(line)
        assert m == n
        same(got, text[:n], f"prefix of {n} bytes")


# ---- the ingest driver over host stand-ins -------------------------------------------------------------------------------
def small_records(rng, n, lo=60, hi=500):
    return [F.record(b"s%d>>x>y" % i, F.bases(rng, int(rng.integers(lo, hi))), 60) for i in range(n)]


def ingest(harness, d, files, arena=ARENA, piece=1024):
    names = []
    for i, blob in enumerate(files):
        names.append(f"in{i}.gz")
        open(os.path.join(d, names[-1]), "wb").write(blob)
    return run(harness, d, ["ingest", str(arena), str(piece)] + names)


def outcome(r):
    assert r.returncode == 0, r.stderr[-2000:]
    reads, settles, oks = [], [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == b"R":
            reads.append((int(w[1]), int(w[2])))
        elif w[0] == b"settle":
            settles.append((int(w[1]), int(w[2])))
        else:
            assert w[0] == b"ok"
            oks.append(line.decode())
    return reads, settles, oks


def blocks_with_first_arena_end(text, end):
    """BGZF blocks of `text` such that the first arena of ARENA bytes ends exactly at byte `end` of the text: one block up to
    `end`, then one that no longer fits the arena's room, then blocks of 500 bytes."""
    assert ARENA - 1500 < end <= ARENA
    cuts = [0, end, end + 2000] + list(range(end + 2500, len(text), 500)) + [len(text)]
    return b"".join(B.block(text[a:b], 1) for a, b in zip(cuts, cuts[1:]) if b > a) + B.EOF


@pytest.mark.parametrize("where", ["on the '>'", "one byte behind", "inside the header", "on the newline in front", "inside a sequence line"])
def test_ingest_carries_the_last_record_at_the_five_cut_positions(harness, tmp_path, where):
    rng = np.random.default_rng(31)
    recs = small_records(rng, 60)
    text = b"".join(recs)[:-1]  # (the last line without its newline)
    h = max(p for p in np.cumsum([len(x) for x in recs]) if p <= ARENA - 8)  # a header's '>' near the first arena's end
    h = int(h)
    assert text[h:h + 1] == b">" and text[h - 1:h] == b"\n"
    end = {"on the '>'": h, "one byte behind": h + 1, "inside the header": h + 6, "on the newline in front": h - 1,
           "inside a sequence line": h - 30}[where]
    assert where != "inside the header" or b">" in text[h + 1:end]
    reads, settles, oks = outcome(ingest(harness, str(tmp_path), [blocks_with_first_arena_end(text, end)]))
    assert reads == F.read_crcs(F.pack(tools.parse_sequences(text)))
    # the first settle: the arena held text[:end]; carried = the bytes from its last header
    last = text.rindex(b"\n>", 0, end) + 1
    assert settles[0] == (end, end - last)
    assert last == h if end > h else last < h
    assert len(settles) >= 3 and settles[-1][1] == 0 and "fasta route" in oks[0] and f"{len(recs)} sequences" in oks[0]


def test_ingest_refuses_a_sequence_that_does_not_fit_an_arena(harness, tmp_path):
    rng = np.random.default_rng(37)
    msg = b"rufus_amd jellyfish count: a FASTA sequence does not fit a text arena of %d bytes (RFX_FASTA_ARENA)" % ARENA
    small = small_records(rng, 10)
    # one record fills the first arena: no header behind the first
    r = ingest(harness, str(tmp_path), [B.write(F.record(b"long", F.bases(rng, 2 * ARENA), 60) + b"".join(small), 1, cut=500)])
    assert r.returncode == 1 and msg in r.stderr, r.stderr[-500:]
    # a record that is carried first and then fills the next arena alone
    r = ingest(harness, str(tmp_path), [B.write(small[0] + F.record(b"carried", F.bases(rng, ARENA - 40), 60) + b"".join(small), 1, cut=500)])
    assert r.returncode == 1 and msg in r.stderr, r.stderr[-500:]
    # ... and one that just fits is counted
    text = small[0] + F.record(b"fits", F.bases(rng, ARENA // 2), 60) + b"".join(small)
    reads, _, _ = outcome(ingest(harness, str(tmp_path), [B.write(text, 1, cut=500)]))
    assert reads == F.read_crcs(F.pack(tools.parse_sequences(text)))


# ---- the FASTQ mode's end of file and the ring's wrap-around ----------------------------------------------------------------
# The smallest arena at which a run is one block and a whole block still fits; piece 1024, so a ring buffer is 64 KiB.
FQ_ARENA = 262144


def fastq_records(rng, lens):
    seqs = [F.bases(rng, int(L), b"ACGTN") for L in lens]
    return [b"@q%d some words\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs)]


def fastq_outcome(harness, d, text, blob, n_blocks, n_records, min_arenas):
    reads, _, oks = outcome(ingest(harness, d, [blob], arena=FQ_ARENA))
    assert reads == F.read_crcs(F.pack(tools.parse_sequences(text)))
    w = oks[0].split()  # ok bgzf route: B blocks in A appends, N arenas, R reads
    assert w[1:3] == ["bgzf", "route:"], oks[0]
    assert (int(w[3]), int(w[6]), int(w[10])) == (n_blocks, n_blocks, n_records), oks[0]  # (a run is one block)
    assert int(w[8]) >= min_arenas, oks[0]


@pytest.mark.parametrize("final_newline", [True, False])
def test_ingest_fastq_over_arenas_and_a_wrapped_ring(harness, tmp_path, final_newline):
    """Ten blocks and the EOF marker through the four buffers of the ring (it wraps twice); four blocks fill an arena, so two
    arenas are cut before the file's end, which comes with and without the last newline."""
    rng = np.random.default_rng(43)
    recs = fastq_records(rng, rng.integers(30, 260, 1900))
    text = b"".join(recs)
    assert len(text) > 9 * 60000
    text = text if final_newline else text[:-1]
    blob = B.write(text, 1, cut=60000)
    n_blocks = len(B.split(blob))
    assert n_blocks >= 10
    fastq_outcome(harness, str(tmp_path), text, blob, n_blocks, len(recs), 3)


def test_ingest_fastq_whose_last_record_is_cut_by_the_first_arena(harness, tmp_path):
    """The first arena takes ten blocks of 26000 bytes and ends inside the file's last record, whose rest does not fit the
    room that is left: the record's head is carried, its rest arrives behind it, and -- the file has no final newline -- the
    whole record is carried once more, to the arena that gets the newline."""
    rng = np.random.default_rng(47)
    end = 10 * 26000
    recs = fastq_records(rng, rng.integers(30, 260, 1200))
    recs = recs[:int(np.searchsorted(np.cumsum([len(x) for x in recs]), end - 3000))]
    size = sum(len(x) for x in recs)
    recs.append(fastq_records(rng, [4000])[0][:-1])  # the last record, without its newline
    text = b"".join(recs)
    assert size < end and len(text) - end > FQ_ARENA - end  # (it starts in the first arena; its rest is more than the room)
    cuts = list(range(0, end + 1, 26000)) + [len(text)]
    blob = b"".join(B.block(text[a:b], 1) for a, b in zip(cuts, cuts[1:])) + B.EOF
    fastq_outcome(harness, str(tmp_path), text, blob, 12, len(recs), 2)


def test_ingest_takes_a_fasta_beside_a_fastq(harness, tmp_path):
    rng = np.random.default_rng(41)
    fa = b"".join(small_records(rng, 40))
    seqs = [F.bases(rng, int(L), b"ACGTN") for L in rng.integers(30, 150, 80)]
    fq = b"".join(b"@q%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    for files, texts in (((fa, fq), (fa, fq)), ((fq, fa, fa), (fq, fa, fa))):
        reads, _, oks = outcome(ingest(harness, str(tmp_path), [B.write(t, 6, cut=700) for t in files]))
        want = []
        for t in texts:
            want += F.read_crcs(F.pack(tools.parse_sequences(t)))
        assert reads == want
        assert ["fasta route" in o for o in oks] == [t[:1] == b">" for t in texts]
