"""GPU: BGZF inflated on the device (k_bgzf_inflate, rufus_amd/csrc/rfx_bgzf.hip) into the text arena of K1, the carry of
the record that straddles two arenas (rfx_text_settle), and `jellyfish count` on bgzip'd FASTQ.

The corpus and the corrupt set are those of tests/bgzf_ref.py.  The corrupt bytes go to the device only after
tests/test_bgzf_host.py has passed on the SAME bytes in the host harness under the sanitizers (the decoder core is one
source for both): run that file first -- the GPU job script does -- and do not re-run this one to look at a fault again."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from rufus_amd import capi
from tests import bgzf_ref as B
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
GUARD = bytes((i * 37 + 11) & 255 for i in range(4096))


@pytest.fixture(scope="module")
def big():
    return B.big_file()


@pytest.mark.parametrize("pieces", [1, 2, 7])
def test_corpus_inflates_between_guard_regions(ctx, big, pieces):
    data, blocks = big
    assert len(blocks) >= 300 and len(data) > 5 << 20
    at, seen = 0, set()
    for b in blocks:  # the blocks' text begins at every alignment mod 16
        seen.add(at % 16)
        at += B.parts(b)[3]
    assert seen == set(range(16))
    arena = capi.TextArena(ctx, len(data) + 2 * len(GUARD) + 64)
    arena.append(GUARD)
    cuts = [len(blocks) * i // pieces for i in range(pieces + 1)]
    for a, b in zip(cuts, cuts[1:]):
        arena.append_bgzf(b"".join(blocks[a:b]))
    arena.append(GUARD[::-1])
    assert arena.bytes == len(data) + 2 * len(GUARD)
    got = arena.fetch()
    assert got[:4096] == GUARD and got[-4096:] == GUARD[::-1]
    assert got[4096:-4096] == data
    # whole blocks only, and only what fits
    with pytest.raises(capi.RufusError, match=r"\(-8\)"):
        arena.append_bgzf(blocks[0][:-1])
    with pytest.raises(capi.RufusError, match=r"\(-7\)"):
        arena.append_bgzf(blocks[0] if B.parts(blocks[0])[3] > 64 else b"".join(blocks[:40]))
    assert arena.fetch() == got
    arena.close()


def _records(rng, n, ragged=True):  # the record sets of tests/test_text_gpu.py
    alpha = np.frombuffer(b"ACGTACGTACGTACGTacgtNnRYKM.-*\r", np.uint8)
    seqs, quals, names = [], [], []
    for i in range(n):
        L = int(rng.choice([0, 1, 5, 24, 25, 31, 32, 33, 63, 64, 65, 100, 150, 151, 250, 301])) if ragged else 150
        s = alpha[rng.integers(0, len(alpha), L)] if rng.random() < 0.3 else alpha[rng.integers(0, 16, L)]
        q = rng.integers(33, 75, L).astype(np.uint8)
        q[rng.random(L) < 0.05] = ord("#")
        q[rng.random(L) < 0.01] = 10 + 128
        q[q == 10] = 11
        seqs.append(s.tobytes())
        quals.append(q.tobytes())
        names.append(b"@r%d/1 some text + @ more" % i)
    return names, seqs, quals


def _fastq(names, seqs, quals):
    return [n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(names, seqs, quals)]


@pytest.mark.parametrize("seed,n,ragged", [(2, 9000, True), (3, 7000, False)])
@pytest.mark.parametrize("flags", [capi.PACK_COUNT, capi.PACK_FILTER])
def test_records_straddling_blocks_and_arenas_parse_like_the_host_packer(ctx, seed, n, ragged, flags):
    rng = np.random.default_rng(seed)
    names, seqs, quals = _records(rng, n, ragged)
    recs = _fastq(names, seqs, quals)
    text = b"".join(recs)
    blocks = B.split(B.write(text, level=1))  # a block per 65280 bytes: records straddle blocks
    cap = len(text) // 3 + 2 * 65536          # two arenas; the text needs three fills
    arenas = [capi.TextArena(ctx, cap), capi.TextArena(ctx, cap)]
    cur, done, fills = 0, 0, 0

    def check(arena):
        nonlocal done, fills
        blk = arena.parse(flags, 15)
        assert blk is not None
        m = blk.n
        ref = capi.PackedReads.from_reads(seqs[done:done + m], quals[done:done + m], 15, flags)
        got = blk.get(want_good=flags == capi.PACK_FILTER, want_acgt=flags == capi.PACK_COUNT)
        nw = int(ref.word_off[-1])
        assert np.array_equal(got["word_off"], ref.word_off) and np.array_equal(got["len"][:m], ref.len[:m])
        assert np.array_equal(got["codes"][:nw], ref.codes[:nw])
        key = "acgt" if flags == capi.PACK_COUNT else "good"
        assert np.array_equal(got[key][:nw], getattr(ref, key)[:nw])
        blk.free()
        arena.reset()
        done += m
        fills += 1

    longest = max(map(len, recs))
    for b in blocks:
        if B.parts(b)[3] > cap - arenas[cur].bytes:
            carried = arenas[cur].settle(arenas[cur ^ 1])
            assert carried < longest and arenas[cur ^ 1].bytes == carried
            check(arenas[cur])
            cur ^= 1
        arenas[cur].append_bgzf(b)
    assert arenas[cur].settle(None) == 0
    check(arenas[cur])
    assert done == n and fills >= 3
    for a in arenas:
        a.close()


def test_settle_edge_cases(ctx):
    rng = np.random.default_rng(5)
    recs = _fastq(*_records(rng, 40, ragged=False))
    text = b"".join(recs)
    a, b = capi.TextArena(ctx, 1 << 20), capi.TextArena(ctx, 1 << 20)
    # text that ends inside a record: nowhere to carry the tail to
    a.append_bgzf(B.write(text[:-10]))
    with pytest.raises(capi.RufusError, match=r"\(-8\).*inside a record"):
        a.settle(None)
    tail = len(recs[-1]) - 10
    assert a.settle(b) == tail and a.fetch() == text[:-len(recs[-1])] and b.fetch() == text[-len(recs[-1]):-10]
    with pytest.raises(capi.RufusError, match=r"\(-2\)"):  # `next` must be empty
        a.settle(b)
    a.reset(), b.reset()
    # fewer than four lines: everything is carried
    three = recs[0][:recs[0].rindex(b"\n", 0, -1) + 1] + b"IIII"  # three newlines and a piece of the fourth line
    a.append_bgzf(B.write(three, eof=False))
    assert a.settle(b) == len(three) and a.bytes == 0 and b.fetch() == three
    a.reset(), b.reset()
    # whole records, plain and BGZF appends mixed, an EOF marker in the middle: nothing to carry
    a.append(recs[0])
    a.append_bgzf(B.block(recs[1]) + B.EOF + B.block(recs[2] + recs[3]))
    a.append(recs[4])
    assert a.settle(None) == 0 and a.fetch() == b"".join(recs[:5])
    blk = a.parse(capi.PACK_COUNT, 0)
    assert blk is not None and blk.n == 5
    blk.free()
    a.reset()
    assert a.settle(None) == 0  # an empty arena
    a.close(), b.close()


def test_corrupt_blocks_are_refused_by_index_and_reason(ctx, big):
    """The bytes of tests/test_bgzf_host.py's corrupt set (which must have passed first), each between two good blocks in
    ONE append: the append is refused (the damage broke the container), or settle names block 1 and the core's reason,
    or -- damage in a field the decoder ignores -- the block inflates to its CRC.  One process, nothing retried."""
    good = B.block(b"@r\nACGT\n+\nIIII\n" * 50)
    text = b"@r\nACGT\n+\nIIII\n" * 50
    reasons = {1: "block type 3", 2: "LEN is not ~NLEN", 3: "HLIT > 286 or HDIST > 30", 4: "over-subscribed", 5: "incomplete",
               6: "repeat code 16", 7: "run past HLIT", 8: "no end-of-block", 9: "symbol 286 or 287", 10: "symbol 30 or 31",
               11: "before the block's first byte", 12: "beyond ISIZE", 13: "short of ISIZE", 14: "input exhausted",
               15: "does not end in the payload's last byte", 16: "CRC mismatch"}
    cases = [(name, blk, reasons[st], False) for name, st, blk in B.refusals()]
    cases += [(name, blk, "", may_pass) for name, blk, may_pass in B.seeded_damage()]
    a, b = capi.TextArena(ctx, 1 << 20), capi.TextArena(ctx, 1 << 20)
    refused_append = refused_block = passed = 0
    for name, blk, reason, may_pass in cases:
        try:
            a.append_bgzf(good + blk + good)
        except capi.RufusError as e:
            assert "(-8)" in str(e) and not reason, name
            refused_append += 1
            continue
        try:
            a.settle(b)
        except capi.RufusError as e:
            assert "(-8)" in str(e) and "rfx_bgzf: block 1: " in str(e) and reason in str(e), (name, str(e))
            with pytest.raises(capi.RufusError, match="rfx_bgzf: block 1"):
                a.fetch()
            with pytest.raises(capi.RufusError, match="rfx_bgzf: block 1"):
                a.parse(capi.PACK_COUNT, 0)
            refused_block += 1
        else:
            assert may_pass, name
            passed += 1
        a.reset(), b.reset()
    assert refused_block >= 100 and passed < 20 and refused_append + refused_block + passed == len(cases)
    # the same arena goes on to inflate the good corpus
    data, blocks = big
    a.close()
    a = capi.TextArena(ctx, len(data) + 64)
    a.append_bgzf(good + B.refusals()[-1][2] + good)
    with pytest.raises(capi.RufusError, match="rfx_bgzf: block 1: CRC mismatch"):
        a.settle(b)
    a.reset()
    a.append_bgzf(b"".join(blocks))
    assert a.fetch() == data
    a.close(), b.close()


# ---- the executable ---------------------------------------------------------------------------------------------------
def _count(d, name, env=None):
    return subprocess.run([f"{BIN}/jellyfish", "count", "--disk", "-m", "25", "-L", "2", "-s", "100M", "-t", "6", "-o", name + ".Jhash",
                           "-C", name + ".fastq.gz"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180,
                          env=dict(os.environ, RFX_CLI_TRACE="1", **(env or {})))


def _payload_sha(path):
    blob = open(path, "rb").read()
    return hashlib.sha256(blob[9 + int(blob[:9]):]).hexdigest()


@pytest.mark.parametrize("level,piece", [(1, None), (6, "70000"), (0, None)])
def test_jellyfish_count_reads_bgzipped_fastq(testrun, tmp_path, level, piece):
    d = str(tmp_path)
    text = testrun["Child"][0] + testrun["Child"][1]
    assert len(text) % B.BLOCK_PAYLOAD not in (0, B.BLOCK_PAYLOAD - 1)  # a short last block
    open(f"{d}/c.fastq.gz", "wb").write(B.write(text, level))
    r = _count(d, "c", {"RFX_INGEST_PIECE": piece} if piece else None)
    assert r.returncode == 0, r.stderr
    assert _payload_sha(f"{d}/c.Jhash") == testrun["expected"]["samples"]["Child"]["s100M"]["payload_sha256"]
    trace = r.stderr.decode()
    assert "bgzf route" in trace
    counts = trace[trace.index("bgzf route: "):].split()
    n_blocks, n_appends = int(counts[2]), int(counts[5])
    assert n_blocks == -(-len(text) // B.BLOCK_PAYLOAD) + 1
    if piece:
        assert n_appends > 3  # many appends


def test_jellyfish_count_refuses_what_it_cannot_count_compressed(testrun, tmp_path):
    d = str(tmp_path)
    text = testrun["Child"][0]
    at = text.index(b"\n@", len(text) // 2) + 1
    open(f"{d}/blank.fastq.gz", "wb").write(B.write(text[:at] + b"\n" + text[at:]))
    r = _count(d, "blank")
    assert r.returncode == 1 and b"compressed input must be strict 4-line FASTQ: inflate it and pipe it in" in r.stderr
    blob = bytearray(B.write(text))
    blocks = B.split(bytes(blob))
    off = sum(map(len, blocks[:2])) + 18 + len(B.parts(blocks[2])[1]) // 2  # inside the third block's payload
    blob[off] ^= 0x5A
    open(f"{d}/flip.fastq.gz", "wb").write(bytes(blob))
    r = _count(d, "flip")
    assert r.returncode != 0 and b"rfx_bgzf: block 2" in r.stderr, r.stderr
