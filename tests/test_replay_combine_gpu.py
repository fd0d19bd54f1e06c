"""k_msp_replay, the form that writes a wave's records in bin order (the default), against the hashing passes (no run map
store) and against the form that stores every record on its own (RFX_REPLAY_SCATTER=1): the same records per shard --
rfx_records_checksum + record count -- at the shapes where the forms part: more than 12 runs of a pass per lane (S >= 3),
reads of other lengths, a block of less than one chunk, bins that take more than two slabs' worth in one chunk."""
import numpy as np
import pytest

import oracle
from rufus_amd import capi, wgs

pytestmark = pytest.mark.gpu

K, SIZE, LOWER, MIN_Q = 25, 8 << 30, 2, 15


def _shard_tables(ctx, k, S, blocks, store=None):
    """One table per shard of S over `blocks`: [(checksum, n_records)] per shard, and the replay form of the last launch."""
    out, form = [], -1
    for sh in range(S):
        t = capi.CountTable(ctx, k, SIZE, mode=capi.COUNT_MSP)
        t.set_shard(sh, S)
        if store is not None:
            t.set_runmaps(store)
        for b in blocks:
            t.add(b)
        if store is not None:
            assert t.replayed() == len(blocks)
            form = capi.replay_variant(ctx)
        rec = t.finish(LOWER)
        out.append((tuple(rec.checksum()), len(rec)))
        rec.free()
        t.free()
    return out, form


def _three_ways(ctx, monkeypatch, k, S, blocks):
    """hashing passes == replay in bin order == replay with scattered stores, and each replay took the form it should"""
    monkeypatch.delenv("RFX_REPLAY_SCATTER", raising=False)
    monkeypatch.delenv("RFX_REPLAY_OLD", raising=False)
    ref, _ = _shard_tables(ctx, k, S, blocks)
    store = capi.RunMaps(ctx)
    got, form = _shard_tables(ctx, k, S, blocks, store)
    assert form == capi.REPLAY_COMBINE
    monkeypatch.setenv("RFX_REPLAY_SCATTER", "1")
    sca, form = _shard_tables(ctx, k, S, blocks, store)
    assert form == capi.REPLAY_SCATTER
    monkeypatch.delenv("RFX_REPLAY_SCATTER")
    store.free()
    assert got == ref, (k, S)
    assert sca == ref, (k, S)


@pytest.mark.parametrize("k,compact", [(25, True), (31, True), (27, False)])
def test_big_block_in_bin_order_cuts_the_records_of_the_hashing_passes(ctx, monkeypatch, k, compact):
    """The big-block path: 2 300 037 pairs (the read count no multiple of 512 or 64) and a small block behind it; S = 2, 3, 4.
    At S >= 3 the entries' half flags do not help, every entry is queued, lanes pass 12 runs: the later batches' scattered
    route runs beside the sorted one."""
    sy = capi.Synth.sample(30_000_000, 0, n_snv=50, seed=2718)
    big = wgs.make_sample(ctx, sy, 2_300_037, 2_300_037, MIN_Q, want_good=False, compact=compact)
    small = wgs.make_sample(ctx, sy, 200_000, 200_000, MIN_Q, want_good=False, compact=compact, first_pair=2_300_037)
    for S in (2, 3, 4):
        _three_ways(ctx, monkeypatch, k, S, big + small)
    for b in big + small:
        b.free()


@pytest.mark.parametrize("read_len,n_pairs", [(76, 1_200_011), (100, 1_200_011), (160, 6_007)])
def test_reads_of_other_lengths(ctx, monkeypatch, read_len, n_pairs):
    """Reads of 76 and 100 bases (3 and 4 code words) and of 160 (5: the longest a run map takes).  Of 160-base reads more
    than one in 32 cut into more runs than a map's 27 entries hold; a block keeps its map while those reads fit its list of
    n / 32 + 4096 -- hence the small block (forced onto the path of big ones) at that length."""
    if n_pairs < 100_000:
        monkeypatch.setenv("RFX_P2L_BINS", "32768")
    sy = capi.Synth.sample(30_000_000, 0, n_snv=50, seed=2718, read_len=read_len)
    blocks = wgs.make_sample(ctx, sy, n_pairs, n_pairs, MIN_Q, want_good=False, compact=True)
    _three_ways(ctx, monkeypatch, K, 2, blocks)
    for b in blocks:
        b.free()


@pytest.mark.parametrize("n_reads", [300, 513])
def test_a_block_of_less_than_a_chunk_per_workgroup(ctx, monkeypatch, n_reads):
    """300 reads: one chunk, not full, waves without a read; 513: a second chunk with one read."""
    monkeypatch.setenv("RFX_P2L_BINS", "32768")
    rng = np.random.default_rng(300 + n_reads)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, 20_000)]
    reads = [genome[p:p + 150].tobytes() for p in rng.integers(0, len(genome) - 150, n_reads)]
    ref = oracle.count(None, K, SIZE, lower=LOWER, reads=reads)
    blk = ctx.upload(capi.PackedReads.from_reads(reads))
    for scatter in (False, True):
        if scatter:
            monkeypatch.setenv("RFX_REPLAY_SCATTER", "1")
        ctx.prof(True)
        ctx.prof_reset()
        t = capi.CountTable(ctx, K, SIZE)
        t.set_passes(2)
        t.add(blk)
        rec = t.finish(LOWER)
        prof = ctx.prof_dict()
        ctx.prof(False)
        assert prof["k_msp_replay"][1] == 2
        assert capi.replay_variant(ctx) == (capi.REPLAY_SCATTER if scatter else capi.REPLAY_COMBINE)
        assert rec.payload() == ref.payload()
        rec.free()
        t.free()
    blk.free()


@pytest.mark.parametrize("copies", [0, 5000])
def test_small_and_skewed_input_matches_the_oracle(ctx, monkeypatch, copies):
    """30 000 plain reads of a 50 kb genome and 600 tandem-repeat reads (those go beside the replay, through the ordinary
    kernel); with `copies`, 5 000 reads that are one plain read over and over: its few coarse bins take more than two
    slabs' worth in one chunk, and the records beyond go through the reservation per record."""
    monkeypatch.setenv("RFX_P2L_BINS", "32768")
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    units = [bytes(acgt[rng.integers(0, 4, int(rng.integers(1, 7)))]) for _ in range(12)]
    repeats = [(u * 160)[:150] for u in units for _ in range(50)]
    genome = acgt[rng.integers(0, 4, 50_000)]
    plain = [genome[p:p + 150].tobytes() for p in rng.integers(0, len(genome) - 150, 30_000)]
    reads = plain[:15_000] + [plain[7]] * copies + plain[15_000:] + repeats
    ref = oracle.count(None, K, SIZE, lower=LOWER, reads=reads)
    blk = ctx.upload(capi.PackedReads.from_reads(reads))
    for scatter in (False, True):
        if scatter:
            monkeypatch.setenv("RFX_REPLAY_SCATTER", "1")
        ctx.prof(True)
        ctx.prof_reset()
        t = capi.CountTable(ctx, K, SIZE)
        t.set_passes(2)
        t.add(blk)
        rec = t.finish(LOWER)
        prof = ctx.prof_dict()
        ctx.prof(False)
        assert prof["k_msp_map"][1] == 1 and prof["k_msp_replay"][1] == 2 and prof["k_msp_part1"][1] == 2
        assert capi.replay_variant(ctx) == (capi.REPLAY_SCATTER if scatter else capi.REPLAY_COMBINE)
        assert rec.payload() == ref.payload()
        rec.free()
        t.free()
    blk.free()
