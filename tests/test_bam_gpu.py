"""GPU: BAM records found (rfx_bam_settle: guess, walk, repair) and packed (rfx_bam_parse) on the device, through capi.

The reference is tests/bam_ref.py's reader (zlib and Python integers): the arrays of bam_parse must be capi.pack_reads' of
the SEQ strings the reader gives, for every tile size and without guesses; the adversarial files must show that repair ran
and still give the same arrays.  tests/test_bam_host.py runs the same record core under the sanitizers on the host: run
that file first -- the GPU job script does."""
import ctypes as C
import struct

import numpy as np
import pytest

from rufus_amd import capi
from tests import bam_ref as R
from tests import bgzf_ref as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files():
    """name -> (Bam, {exclude: (kept SEQ strings, packed reference, runs)}): read and packed once, shared, never changed."""
    out = {}
    for name, blob in (("Child", R.fixture("Child")), ("Mother", R.fixture("Mother")), ("Father", R.fixture("Father")),
                       ("synthetic", R.synthetic()), ("adversarial", R.adversarial(16384)), ("adversarial_512", R.adversarial(512))):
        bam = R.Bam(blob)
        refs = {}
        for ex in (0, 3328):
            seqs = bam.kept_seqs(ex)
            refs[ex] = (seqs, capi.PackedReads.from_reads(seqs, flags=capi.PACK_COUNT), bam.runs(ex))
        out[name] = (bam, refs)
    return out


def _check_block(blk, runs, ref):
    seqs, packed, want_runs = ref
    L = capi.lib()
    nw = int(packed.word_off[-1])
    assert blk.n == len(seqs)
    assert int(L.rfx_reads_words(blk._h)) == nw and int(L.rfx_reads_bases(blk._h)) == sum(map(len, seqs))
    for l in range(32):
        assert int(L.rfx_reads_of_length(blk._h, l)) == sum(1 for s in seqs if len(s) == l), l
    got = blk.get(want_good=False, want_acgt=True)
    assert np.array_equal(got["word_off"], packed.word_off) and np.array_equal(got["len"], packed.len[:len(seqs)])
    assert np.array_equal(got["codes"], packed.codes[:nw]) and np.array_equal(got["acgt"], packed.acgt[:nw])
    assert [tuple(x) for x in runs.tolist()] == want_runs


def _one_arena(ctx, bam, refs, excludes=(0, 3328)):
    hdr = capi.bam_header(bam.bam)
    assert hdr["n_ref"] == len(bam.refs)
    a = capi.TextArena(ctx, len(bam.data) + 65536)
    a.append_bgzf(bam.bam[hdr["first_block"]:])
    n, carried = a.bam_settle(None, hdr["skip"], hdr["n_ref"])
    assert (n, carried) == (len(bam.records), 0)
    stats = ctx.bam_stats()
    assert stats["records"] == n
    for ex in excludes:
        blk, runs = a.bam_parse(ex)
        _check_block(blk, runs, refs[ex])
        blk.free()
    a.close()
    return stats


@pytest.mark.parametrize("name", ["Child", "Mother", "Father", "synthetic"])
def test_parse_equals_the_host_packer(ctx, files, name):
    bam, refs = files[name]
    if name == "synthetic":
        lens = {r["l_seq"] for r in bam.records}
        assert set(R.EDGE_LENGTHS) <= lens and {r["start"] % 4 for r in bam.records} == {0, 1, 2, 3}
        assert {(r["start"] + 36 + len(r["name"]) + 1 + 4 * len(r["cigar"])) % 4 for r in bam.records} == {0, 1, 2, 3}
        assert {len(r["cigar"]) for r in bam.records} >= {0, 300} and {len(r["name"]) for r in bam.records} >= {0, 1, 253}
        assert {r["flag"] & 3840 for r in bam.records} >= {0, 256, 512, 1024, 2048, 3072, 3328}
        assert set("".join(r["seq"] for r in bam.records)) >= set(R.SEQ_LETTERS)
    stats = _one_arena(ctx, bam, refs)
    assert stats["tiles"] == -(-len(bam.data) // 16384)


@pytest.mark.parametrize("tile,no_guess", [(256, False), (512, False), (4096, False), (16384, False), (16384, True), (512, True)])
@pytest.mark.parametrize("name", ["Father", "synthetic"])
def test_tile_size_and_guessing_change_no_result(ctx, files, monkeypatch, name, tile, no_guess):
    bam, refs = files[name]
    monkeypatch.setenv("RFX_BAM_TILE", str(tile))
    if no_guess:
        monkeypatch.setenv("RFX_BAM_NO_GUESS", "1")
    stats = _one_arena(ctx, bam, refs, excludes=(3328,))
    assert stats["tiles"] == -(-len(bam.data) // tile)
    if no_guess:  # every tile behind the first had its sentinel replaced
        assert stats["changed"] == stats["tiles"] - 1 and stats["rounds"] >= 1


@pytest.mark.parametrize("name,tile", [("adversarial", 16384), ("adversarial_512", 512)])
def test_adversarial_files_are_repaired(ctx, files, monkeypatch, name, tile):
    bam, refs = files[name]
    monkeypatch.setenv("RFX_BAM_TILE", str(tile))
    assert max(e - s for s, e in zip(bam.starts, bam.starts[1:])) > 3 * tile
    stats = _one_arena(ctx, bam, refs)
    assert stats["changed"] >= 1 and stats["rounds"] >= 2, stats


@pytest.mark.parametrize("cap", [65536 + 40000, 200000, 1 << 20])
def test_two_arenas_carry_at_many_cuts(ctx, files, cap):
    """The file goes block by block through two arenas of `cap` bytes; the concatenated blocks are the one-arena result."""
    bam, refs = files["Father"]
    seqs, _, want_runs = refs[3328]
    hdr = capi.bam_header(bam.bam)
    arenas = [capi.TextArena(ctx, cap), capi.TextArena(ctx, cap)]
    cur, skip, done, fills, got_runs = 0, hdr["skip"], 0, 0, []
    kept_of = np.cumsum([0] + [not r["flag"] & 3328 for r in bam.records])

    def parse(a, n_rec, first_rec):
        nonlocal done, fills
        blk, runs = a.bam_parse(3328)
        m = int(kept_of[first_rec + n_rec] - kept_of[first_rec])
        part = seqs[done:done + m]
        _check_block(blk, runs, (part, capi.PackedReads.from_reads(part, flags=capi.PACK_COUNT),
                                 [tuple(x) for x in runs.tolist()]))
        for first, ref in runs.tolist():
            if not got_runs or got_runs[-1][1] != ref:
                got_runs.append((done + first, ref))
        blk.free()
        a.reset()
        done += m
        fills += 1

    rec, ends = 0, bam.starts + [len(bam.data)]
    for b in B.split(bam.bam[hdr["first_block"]:]):
        if B.parts(b)[3] > cap - arenas[cur].bytes:
            before = arenas[cur].bytes
            n, carried = arenas[cur].bam_settle(arenas[cur ^ 1], skip, hdr["n_ref"])
            assert carried == before - (ends[rec + n] - ends[rec]) - skip and arenas[cur ^ 1].bytes == carried
            parse(arenas[cur], n, rec)
            rec += n
            skip = 0
            cur ^= 1
        arenas[cur].append_bgzf(b)
    n, carried = arenas[cur].bam_settle(None, skip, hdr["n_ref"])
    assert carried == 0 and rec + n == len(bam.records)
    parse(arenas[cur], n, rec)
    assert done == len(seqs) and got_runs == want_runs and fills >= (2 if cap >= 1 << 20 else 4)
    for a in arenas:
        a.close()


def test_refusals(ctx):
    rng = np.random.default_rng(51)
    recs = [R.record(b"q%d" % i, 0, i % 5, i, [("M", 50)], R._seq(rng, 50, True)) for i in range(200)]
    good = R.Bam(R.write(R.REFS, recs))
    hdr = capi.bam_header(good.bam)
    a, b = capi.TextArena(ctx, 1 << 20), capi.TextArena(ctx, 1 << 20)
    # a file cut inside a record, nowhere to carry the tail to
    a.append_bgzf(B.write(good.data[:-10]))
    with pytest.raises(capi.RufusError, match=r"\(-8\).*inside a record"):
        a.bam_settle(None, good.first, 5)
    assert a.bam_settle(b, good.first, 5) == (199, len(good.data) - 10 - good.starts[-1])
    assert b.fetch() == good.data[good.starts[-1]:-10]
    with pytest.raises(capi.RufusError, match=r"\(-2\)"):  # `next` must be empty
        a.bam_settle(b, good.first, 5)
    a.reset(), b.reset()
    with pytest.raises(capi.RufusError, match="has not been settled"):
        a.bam_parse()
    # a chain record with block_size = 10
    bad = bytearray(good.data)
    bad[good.starts[100]:good.starts[100] + 4] = struct.pack("<I", 10)
    a.append_bgzf(B.write(bytes(bad)))
    with pytest.raises(capi.RufusError, match=r"\(-8\) rfx_bam: record at byte %d: block_size below 32" % good.starts[100]):
        a.bam_settle(b, good.first, 5)
    assert a.fetch() == bytes(bad) and b.bytes == 0  # nothing was changed
    a.reset()
    # a refID the header does not have
    a.append_bgzf(good.bam[hdr["first_block"]:])
    with pytest.raises(capi.RufusError, match=r"rfx_bam: record at byte %d: refID outside" % good.starts[3]):
        a.bam_settle(None, hdr["skip"], 3)
    a.reset()
    # a block that did not inflate
    blocks = B.split(good.bam)
    a.append_bgzf(blocks[0][:30] + bytes([blocks[0][30] ^ 0x5A]) + blocks[0][31:])
    with pytest.raises(capi.RufusError, match=r"\(-8\) rfx_bgzf: block 0"):
        a.bam_settle(None, hdr["skip"], 5)
    a.close(), b.close()
    # a record longer than the arena
    long = R.write(R.REFS, [R.record(b"long", 0, 0, 1, [], R._seq(rng, 200000))], level=1)
    small, nxt = capi.TextArena(ctx, 100000), capi.TextArena(ctx, 100000)
    h = capi.bam_header(long)
    small.append_bgzf(B.split(long)[0])
    assert small.bytes == B.BLOCK_PAYLOAD
    with pytest.raises(capi.RufusError, match=r"\(-7\).*first record does not end"):
        small.bam_settle(nxt, h["skip"], 5)
    small.close(), nxt.close()


def test_run_list_is_written_inside_its_bounds(ctx, files):
    """Guard words around the run list stay untouched, a list that is too short is refused, the arena is not written."""
    bam, refs = files["synthetic"]
    want = refs[3328][2]
    hdr = capi.bam_header(bam.bam)
    a = capi.TextArena(ctx, len(bam.data) + 65536)
    a.append_bgzf(bam.bam[hdr["first_block"]:])
    a.bam_settle(None, hdr["skip"], hdr["n_ref"])
    before = a.fetch()
    guard = 64
    buf = np.full(2 * len(want) + 2 * guard, 0xA5A5A5A5, np.uint32)
    n_runs = C.c_uint64(0)
    h = capi.lib().rfx_bam_parse(a._h, 3328, buf[guard:].ctypes.data_as(capi.u32p), len(want), C.byref(n_runs))
    assert h and n_runs.value == len(want)
    capi.ReadBlock.from_handle(ctx, h).free()
    assert (buf[:guard] == 0xA5A5A5A5).all() and (buf[-guard:] == 0xA5A5A5A5).all()
    assert buf[guard:-guard].reshape(-1, 2).astype(np.int32).tolist() == [list(x) for x in want]
    h = capi.lib().rfx_bam_parse(a._h, 3328, buf[guard:].ctypes.data_as(capi.u32p), len(want) - 1, C.byref(n_runs))
    assert not h and n_runs.value == len(want) and b"RFX_E_RANGE" in capi.lib().rfx_last_error()
    assert a.fetch() == before
    a.close()


def test_jellyfish_count_takes_a_bam(ctx, files):
    import oracle
    from rufus_amd import tools
    bam, refs = files["Father"]
    fastq = b"".join(b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for s in refs[3328][0])
    got = tools.jellyfish_count(ctx, [bam.bam], 25, 1 << 22, lower=2)
    assert got.records.payload() == oracle.count([fastq], 25, 1 << 22, lower=2).payload()
