"""GPU: FASTA text in a text arena -> a packed read block (rfx_text_parse_fasta, rufus_amd/csrc/rfx_fasta.hip), the cut of
an arena at a FASTA record (rfx_text_settle_fasta) and `jellyfish count` on a bgzip'd FASTA.

The reference is capi.PackedReads of tools.parse_sequences(text) -- the host packer on the reference parser's sequences --
and the oracle's count; never the code under test.  The same texts run through the host side of the rule, under the
sanitizers, in tests/test_fasta_host.py.  No test here provokes a device fault: every refusal is decided before or without
an access outside the arena."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle
from rufus_amd import capi, tools
from tests import bgzf_ref as B
from tests import fasta_ref as F
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
CASES = F.cases()
ARENA = 1 << 20  # the smallest arena tests/test_bgzf_gpu.py opens


def same_block(blk, seqs, what):
    ref = capi.PackedReads.from_reads(seqs, flags=capi.PACK_COUNT)
    L = capi.lib()
    nw = int(ref.word_off[-1])
    assert blk.n == len(seqs) and int(L.rfx_reads_words(blk._h)) == nw, what
    assert int(L.rfx_reads_bases(blk._h)) == sum(map(len, seqs)), what
    assert blk.max_len == max(map(len, seqs)), what
    for l in range(32):
        assert int(L.rfx_reads_of_length(blk._h, l)) == sum(1 for s in seqs if len(s) == l), (what, l)
    got = blk.get(want_good=False)
    assert np.array_equal(got["word_off"], ref.word_off) and np.array_equal(got["len"], ref.len[:len(seqs)]), what
    assert np.array_equal(got["codes"][:nw], ref.codes[:nw]) and np.array_equal(got["acgt"][:nw], ref.acgt[:nw]), what


@pytest.mark.parametrize("case", range(len(CASES)), ids=[name for name, _ in CASES])
def test_parse_equals_the_host_packer(ctx, case):
    name, text = CASES[case]
    seqs = tools.parse_sequences(text)
    assert seqs and text[:1] == b">"
    arena = capi.TextArena(ctx, len(text) + 64)
    try:
        arena.append(text[:len(text) // 3])  # (three appends: the text need not arrive in one piece)
        arena.append(text[len(text) // 3:len(text) // 2])
        arena.append(text[len(text) // 2:])
        blk = arena.parse_fasta()
        assert blk is not None, name
        same_block(blk, seqs, name)
        blk.free()
        # the same text settled as a file's last arena: nothing is carried, nothing changes
        assert arena.settle_fasta(None) == 0 and arena.bytes == len(text)
        blk = arena.parse_fasta()
        same_block(blk, seqs, name)
        blk.free()
    finally:
        arena.close()


def test_count_of_a_parsed_chromosome_goes_through_the_tiler(ctx):
    text = F.long_text()
    seqs = tools.parse_sequences(text)
    assert [len(s) for s in seqs] == [200000]
    want = oracle.count(None, 25, 1 << 22, reads=seqs)
    arena = capi.TextArena(ctx, len(text) + 64)
    arena.append(text)
    blk = arena.parse_fasta()
    arena.close()
    assert blk.max_len == 200000
    t = capi.CountTable(ctx, 25, 1 << 22)
    try:
        t.add(blk)
        rec = t.finish()
        assert rec.payload() == want.payload()
        rec.free()
    finally:
        t.free()
        blk.free()


def test_settle_carries_the_last_record_across_arenas(ctx):
    text = F.big_text()
    assert len(text) >= 3 << 20 and text[-1:] != b"\n"
    seqs = tools.parse_sequences(text)
    arenas = [capi.TextArena(ctx, ARENA), capi.TextArena(ctx, ARENA)]
    places = ["on the '>'", "one byte behind", "inside the header", "on the newline in front", "inside a sequence line"]
    seen, got, pos, cur, carried = [], [], 0, 0, b""
    try:
        while True:
            # the arena holds `carried`; it is filled up to a chosen place near 600 KiB of new text
            aim = pos + 600_000
            if aim >= len(text):
                end, last_arena = len(text), True
            else:
                h = text.rindex(b"\n>", pos, aim) + 1  # a header's '>'
                place = places[len(seen) % len(places)]
                end = {places[0]: h, places[1]: h + 1, places[2]: h + 8, places[3]: h - 1, places[4]: h - 100}[place]
                assert place != places[2] or b">" in text[h + 1:end]
                seen.append(place)
                last_arena = False
            arenas[cur].append(text[pos:end])
            held = carried + text[pos:end]
            assert arenas[cur].bytes == len(held)
            if last_arena:
                assert arenas[cur].settle_fasta(None) == 0 and arenas[cur].bytes == len(held)  # the last line has no newline
                kept = held
            else:
                cut = held.rindex(b"\n>") + 1
                assert arenas[cur].settle_fasta(arenas[cur ^ 1]) == len(held) - cut
                assert arenas[cur].bytes == cut and arenas[cur ^ 1].bytes == len(held) - cut
                kept, carried = held[:cut], held[cut:]
            blk = arenas[cur].parse_fasta()
            part = tools.parse_sequences(kept)
            same_block(blk, part, f"arena {len(got)}")
            got += part
            blk.free()
            arenas[cur].reset()
            if last_arena:
                break
            pos, cur = end, cur ^ 1
        assert got == seqs and set(seen) == set(places)
        assert arenas[cur ^ 1].fetch() == b""
    finally:
        for a in arenas:
            a.close()


def test_refusals(ctx):
    rng = np.random.default_rng(43)
    a, b = capi.TextArena(ctx, ARENA), capi.TextArena(ctx, ARENA)
    try:
        # one record larger than the arena: what an arena can hold of it has no second header
        a.append(F.record(b"long", F.bases(rng, ARENA), 60)[:ARENA])
        with pytest.raises(capi.RufusError, match=r"\(-7\) rfx_fasta:.*%d bytes" % ARENA):
            a.settle_fasta(b)
        assert a.bytes == ARENA and b.bytes == 0
        a.reset()
        # `next` must be empty and another arena
        a.append(b">x\nACGT\n>y\nAC\n")
        b.append(b">z\n")
        for nxt in (b, a):
            with pytest.raises(capi.RufusError, match=r"\(-2\)"):
                a.settle_fasta(nxt)
        b.reset()
        assert a.settle_fasta(b) == 6 and a.fetch() == b">x\nACGT\n" and b.fetch() == b">y\nAC\n"
        a.reset(), b.reset()
        # an arena that starts with 'A'
        a.append(b"ACGT\n>x\nACGT\n")
        with pytest.raises(capi.RufusError, match=r"\(-8\)"):
            a.settle_fasta(b)
        assert a.parse_fasta() is None
        a.reset()
        assert a.parse_fasta() is None and a.settle_fasta(b) == 0  # an empty arena
        # FASTA has no qualities
        a.append(b">x\nACGT\n")
        for flags in (capi.PACK_FILTER, capi.PACK_COUNT | capi.PACK_FILTER, 0):
            with pytest.raises(capi.RufusError, match="RFX_E_INVAL"):
                a.parse_fasta(flags)
        a.reset()
        # a corrupt BGZF block in the arena (tests/bgzf_ref.py's CRC mismatch, which tests/test_bgzf_host.py runs on the host):
        # what rfx_text_parse answers
        good = B.block(b">r\nACGT\n" * 50)
        a.append_bgzf(good + B.refusals()[-1][2] + good)
        with pytest.raises(capi.RufusError, match=r"\(-8\) rfx_bgzf: block 1: CRC mismatch"):
            a.settle_fasta(b)
        with pytest.raises(capi.RufusError, match="rfx_bgzf: block 1: CRC mismatch"):
            a.parse_fasta()
        with pytest.raises(capi.RufusError, match="rfx_bgzf: block 1: CRC mismatch"):
            a.parse(capi.PACK_COUNT, 0)
        a.reset()
        # ... and the arena goes on to parse good blocks
        a.append_bgzf(good + B.EOF + good)
        blk = a.parse_fasta()
        same_block(blk, [b"ACGT"] * 100, "after the reset")
        blk.free()
    finally:
        a.close(), b.close()


# ---- the executable ---------------------------------------------------------------------------------------------------
def _payload(path):
    blob = open(path, "rb").read()
    return blob[9 + int(blob[:9]):]


def _run(d, args, env=None):
    return subprocess.run([f"{BIN}/jellyfish"] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", RFX_FASTA_ARENA=str(ARENA), RFX_INGEST_PIECE="4096", **(env or {})))


@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(47)
    seqs = [F.bases(rng, int(L), b"ACGTACGTACGTACGTacgtN") for L in rng.integers(20_000, 300_001, 24)]
    for i in range(1, 24, 3):  # repeats between the sequences: -L 2 leaves something to compare
        seqs[i] = seqs[i - 1][5_000:15_000] + seqs[i][10_000:]
    return b"".join(F.record(b"chr%d some text" % i, s, 60) for i, s in enumerate(seqs))


@pytest.fixture(scope="module")
def genome_counts(genome):
    return {k: oracle.count([genome], k, 100_000_000, lower=lower) for k, lower in ((25, 2), (15, 0))}


@pytest.mark.parametrize("k,extra", [(25, ["-L", "2"]), (15, [])])
@pytest.mark.parametrize("level", [1, 6])
def test_jellyfish_count_reads_a_bgzipped_fasta(genome, genome_counts, tmp_path, level, k, extra):
    d = str(tmp_path)
    open(f"{d}/ref.fa", "wb").write(genome)
    open(f"{d}/ref.fa.gz", "wb").write(B.write(genome, level))
    for out, src in (("a", "ref.fa.gz"), ("b", "ref.fa")):
        r = _run(d, ["count", "-m", str(k), "-C", "-s", "100M"] + extra + ["-o", f"{out}.jf", src])
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        trace = r.stderr.decode()
        assert ("fasta route" in trace) == (out == "a")
        if out == "a":
            w = trace[trace.index("fasta route: "):].split()
            assert int(w[7]) >= 3 and int(w[9]) == 24, trace  # arenas, sequences
        h = _run(d, ["histo", "-f", "-o", f"{out}.histo", f"{out}.jf"])
        assert h.returncode == 0, h.stderr.decode()[-2000:]
    assert _payload(f"{d}/a.jf") == _payload(f"{d}/b.jf")
    assert open(f"{d}/a.histo", "rb").read() == open(f"{d}/b.histo", "rb").read()
    want = genome_counts[k]
    assert _payload(f"{d}/a.jf") == want.payload() and len(want.keys) > 5_000


def test_jellyfish_count_takes_a_fasta_beside_a_fastq(genome, tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(53)
    fa = genome[:genome.index(b"\n>", 400_000) + 1]
    reads = [fa[at:at + 130].replace(b"\n", b"").replace(b">", b"") for at in rng.integers(100, len(fa) - 200, 4000)]
    fq = b"".join(b"@q%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads))
    for name, blob in (("ref.fa", fa), ("ref.fa.gz", B.write(fa, 6)), ("r.fastq", fq), ("r.fastq.gz", B.write(fq, 6))):
        open(f"{d}/{name}", "wb").write(blob)
    for out, srcs in (("a", ["ref.fa.gz", "r.fastq.gz"]), ("b", ["ref.fa", "r.fastq"]), ("c", ["r.fastq.gz", "ref.fa.gz"])):
        r = _run(d, ["count", "-m", "25", "-C", "-s", "100M", "-L", "2", "-o", f"{out}.jf"] + srcs)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert (b"fasta route" in r.stderr and b"bgzf route" in r.stderr) == (out != "b")
    want = oracle.count([fa, fq], 25, 100_000_000, lower=2)
    assert _payload(f"{d}/a.jf") == _payload(f"{d}/b.jf") == _payload(f"{d}/c.jf") == want.payload() and len(want.keys) > 5_000


def test_jellyfish_count_refuses_a_sequence_larger_than_the_arena(tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(59)
    text = F.record(b"small", F.bases(rng, 5000), 60) + F.record(b"long", F.bases(rng, ARENA + 5000), 60) + F.record(b"tail", b"ACGT", 60)
    open(f"{d}/ref.fa.gz", "wb").write(B.write(text, 1))
    r = _run(d, ["count", "-m", "25", "-C", "-s", "100M", "-o", "a.jf", "ref.fa.gz"])
    msg = b"rufus_amd jellyfish count: a FASTA sequence does not fit a text arena of %d bytes (RFX_FASTA_ARENA)" % ARENA
    assert r.returncode == 1 and msg in r.stderr, r.stderr.decode()[-2000:]
