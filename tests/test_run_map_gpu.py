"""The run map that k_msp_part1<HMODE 4> leaves (rfx_runmaps_read) against tests/run_map_ref.py: every read's 32 bytes and
the block's overflow list, exactly, on reads chosen for where the kernel's paths part -- a phase is 8 bases, run ends are
closed every 4 phases (32 bases), a chunk is 512 reads."""
import functools

import numpy as np
import pytest

from rufus_amd import capi
from tests import run_map_ref as ref
from tests.binned_ref import SIZE, _planted_targets, mmer_len

pytestmark = pytest.mark.gpu

# the last batch of a read of L bases (L + 1 with the base that closes the last run) has 1, 2, 3 or 4 phases (40 and 105: 2)
LENGTHS = (24, 25, 31, 32, 33, 40, 56, 57, 64, 65, 88, 89, 105, 150, 159, 160)
assert {((L + 8) // 8 - 1) % 4 + 1 for L in LENGTHS} == {1, 2, 3, 4}


def _random(rng, L):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].copy()


def _with_n(rng, L, at):
    s = _random(rng, L)
    for a, b in at:
        s[a:b] = ord("N")
    return s


@functools.lru_cache(maxsize=None)
def zoo(k: int, n_reads: int) -> tuple:
    """n_reads reads as byte strings: the hand-made ones first, random 150-base reads up to n_reads."""
    rng = np.random.default_rng(100 * k + 7)
    out = []
    for L in LENGTHS:
        out += [_random(rng, L) for _ in range(16)]
        if L < 34:
            continue
        # N on either side of a batch boundary (base 32) and of a phase boundary (base 8)
        for at in ((31,), (32,), (33,), (7,), (8,), (31, 32, 33), (7, 8), (7, 33)):
            out.append(_with_n(rng, L, [(a, a + 1) for a in at]))
    for L in (150, 160):                                  # runs of N: gaps of more than 16 (and more than 32) positions
        for a, n in ((0, 20), (1, 31), (30, 17), (31, 34), (40, 40), (60, 64), (100, 60), (L - 1, 1), (L - 26, 2)):
            out.append(_with_n(rng, L, [(a, min(a + n, L))]))
        out.append(_with_n(rng, L, [(30, 31), (62, 63), (94, 95), (126, 127)]))
    out += [_with_n(rng, L, [(0, L)]) for L in (24, 33, 150)]    # all N
    # More than 27 entries.  Equal m-mers: the position in the hash's low bits breaks the tie, the minimizer changes at
    # every base.  And reads made of planted m-mers (mmer_unhash of the smallest hashes) one behind the other: each is
    # the minimizer while a window holds it, the k-mers between fall to what is left -- 20 to 35 entries, on both sides
    # of the map's capacity.
    for L in (89, 150, 160):
        out += [np.full(L, ord(c), np.uint8) for c in "ACGT"]
        out += [np.resize(np.frombuffer(p, np.uint8), L).copy() for p in (b"AC", b"GT", b"ACG", b"AATT", b"ACGTT")]
    m, targets = mmer_len(k), _planted_targets(k, 4096)
    letters = np.frombuffer(b"ACGT", np.uint8)
    for i in range(48):
        pick = rng.permutation(len(targets))[:160 // m + 1]
        if i % 3 == 0:
            pick = np.sort(pick)[::-1]                    # ever smaller hashes: a planted m-mer takes over as it comes
        s = np.concatenate([letters[[(int(targets[t]) >> (2 * (m - 1 - j))) & 3 for j in range(m)]] for t in pick])
        out.append(s[int(rng.integers(0, m)):][:(150, 159, 160)[i % 3]].copy())
    assert len(out) <= n_reads
    out += [_random(rng, 150) for _ in range(n_reads - len(out))]
    return tuple(x.tobytes() for x in out)


def _map_of(ctx, blk, k, canonical):
    t = capi.CountTable(ctx, k, SIZE, canonical=canonical, mode=capi.COUNT_MSP)
    store = capi.RunMaps(ctx)
    try:
        t.set_runmaps(store)
        t.prepare_maps([blk])
        assert store.blocks() == 1
        return store.read(blk)
    finally:
        t.free()
        store.free()


def _has_gap(rows):
    used = np.arange(27)[None, :] < np.minimum(rows[:, 31] >> 3, 27)[:, None]
    return bool((used & ((rows[:, :27] & 15) == 15)).any())


def _compare(got, want, what):
    (rows, ovf), (ref_rows, ref_ovf) = got, want
    assert rows.shape == ref_rows.shape
    bad = np.flatnonzero((rows != ref_rows).any(axis=1))
    assert len(bad) == 0, (what, f"{len(bad)} reads differ, the first: {bad[0]}", rows[bad[0]].tolist(), ref_rows[bad[0]].tolist())
    assert np.array_equal(ovf, ref_ovf), (what, ovf[:8], ref_ovf[:8])


@pytest.mark.parametrize("n_reads", [511, 512, 513])
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [25, 23, 27, 31])
def test_map_of_a_dense_block_is_the_reference(ctx, k, canonical, n_reads):
    reads = zoo(k, n_reads)
    blk = ctx.upload(capi.PackedReads.from_reads(list(reads)))
    try:
        packed = blk.get(want_good=False)
        assert np.array_equal(packed["len"], [len(s) for s in reads])
        want = ref.block_map(packed, k, canonical)
        counts = np.array([ref.entry_count(r) for r in want[0]])
        # the cases are there: full maps, reads without one, gaps, reads without a k-mer
        assert (counts == 27).any() or (counts == 26).any()
        assert 10 <= len(want[1]) < n_reads // 2 and (counts == 0).any() and _has_gap(want[0])
        _compare(_map_of(ctx, blk, k, canonical), want, (k, canonical, n_reads))
    finally:
        blk.free()


@pytest.mark.parametrize("k", [25, 31])
@pytest.mark.parametrize("L", LENGTHS)
def test_map_of_reads_of_one_length_is_the_reference(ctx, k, L):
    """A chunk runs as many phases as its longest read has: with one length the kernel's last batch is the reads' own."""
    rng = np.random.default_rng(1000 * k + L)
    reads = [_random(rng, L) for _ in range(150)]
    reads += [_with_n(rng, L, [(a, a + 1)]) for a in range(0, L, 3)] + [np.full(L, ord("A"), np.uint8)]
    blk = ctx.upload(capi.PackedReads.from_reads([x.tobytes() for x in reads]))
    try:
        want = ref.block_map(blk.get(want_good=False), k, True)
        assert L < k or (want[0][:, 31] >> 3).max() > 0
        _compare(_map_of(ctx, blk, k, True), want, (k, L))
    finally:
        blk.free()


@pytest.mark.parametrize("read_len,n_pairs", [(150, 256), (150, 257), (100, 1000), (57, 600), (40, 600)])
@pytest.mark.parametrize("k,canonical", [(25, True), (23, False), (27, True), (31, True)])
def test_map_of_a_compact_block_is_the_reference(ctx, k, canonical, read_len, n_pairs):
    """Reads of one length without offsets, the ACGT mask only for the reads that have an N."""
    sy = capi.Synth.sample(200_000, 0, n_snv=4, seed=77, read_len=read_len)
    blk = ctx.synth_reads(sy, 0, n_pairs, 15, want_good=False, compact=True)
    try:
        packed = blk.get(want_good=False)
        assert np.array_equal(packed["len"], np.full(2 * n_pairs, read_len, np.uint32))
        want = ref.block_map(packed, k, canonical)
        assert n_pairs < 500 or _has_gap(want[0])      # (some read has an N)
        _compare(_map_of(ctx, blk, k, canonical), want, (k, canonical, read_len, n_pairs))
    finally:
        blk.free()
