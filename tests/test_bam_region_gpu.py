"""GPU: the region test on the device (rfx_bam_set_region, k_bam_region) through capi.

One arena of raw records made by tests/bam_ref.py's writer (tests/bai_ref.py region_table: every CIGAR shape the test
branches on, the exact boundaries, 64-bit sums, the other references).  The keep set of bam_set_region + bam_parse must be
bai_ref.in_region AND the flag test, the block must be capi's host packer of exactly those SEQs, and bam_parse_filter,
bam_name_hashes, bam_locate, bam_mark_names and bam_gather must agree on that set.  Record counts 0, 1, 63, 64, 65 (the
ballot per 64 records), 257 (more than one workgroup) and 70 000 (the grid-stride loop cannot be seen below the grid's
size, but every lane's index arithmetic can).  tests/test_bai_host.py runs the same statements under the sanitizers on the
host.  Fails without the feature: rfx_bam_set_region does not exist."""
import numpy as np
import pytest

from rufus_amd import capi
from tests import bai_ref as X
from tests import bam_ref as R

pytestmark = pytest.mark.gpu
N_REF = len(X.TABLE_REFS)
COUNTS = (0, 1, 63, 64, 65, 257, 70_000)


@pytest.fixture(scope="module")
def table():
    """n -> (raw records, parsed records): made once, shared, never changed (a prefix of the longest table)."""
    recs = X.region_table(max(COUNTS))
    parsed = R.read_records(b"".join(recs), 0)
    return {n: (recs[:n], parsed[:n]) for n in COUNTS}


def _arena(ctx, recs):
    data = b"".join(recs)
    a = capi.TextArena(ctx, len(data) + 65536)
    if data:
        a.append(data)
    n, carried = a.bam_settle(None, 0, N_REF)
    assert (n, carried) == (len(recs), 0)
    return a


def _want(parsed, region, exclude):
    return [r for r in parsed if X.in_region(r, *region) and not r["flag"] & exclude]


def _check_block(blk, seqs):
    packed = capi.PackedReads.from_reads(seqs, flags=capi.PACK_COUNT)
    nw = int(packed.word_off[-1])
    assert blk.n == len(seqs)
    got = blk.get(want_good=False, want_acgt=True)
    assert np.array_equal(got["word_off"], packed.word_off) and np.array_equal(got["len"], packed.len[:len(seqs)])
    assert np.array_equal(got["codes"], packed.codes[:nw]) and np.array_equal(got["acgt"], packed.acgt[:nw])


def test_the_table_holds_what_the_test_is_about(table):
    _, parsed = table[257]
    tid, beg, end = X.TABLE_REGIONS[0]
    mine = [r for r in parsed if r["ref_id"] == tid]
    # each side of each boundary, on the reference's answers, before the device is asked
    assert sum(1 for r in mine if r["pos"] < beg and X.end_pos(r) <= beg) >= 25    # end in front of BEG: out
    assert sum(1 for r in mine if r["pos"] < beg and X.end_pos(r) > beg) >= 25     # ... behind it: in
    assert sum(1 for r in mine if beg <= r["pos"] < end) >= 25                     # start in front of END: in
    assert sum(1 for r in mine if r["pos"] >= end) >= 25                           # ... at or behind it: out
    assert any(X.end_pos(r) == beg for r in mine) and any(X.end_pos(r) == beg + 1 for r in mine)
    assert any(r["pos"] == end - 1 for r in mine) and any(r["pos"] == end for r in mine)
    n_ops = {len(r["cigar"]) for r in parsed}
    assert {0, 1, 2, 300, 9} <= n_ops
    assert any({op for op, _ in r["cigar"]} == set(R.CIGAR_OPS) for r in parsed)
    assert any(r["cigar"] and {op for op, _ in r["cigar"]} <= {"I", "S"} for r in parsed)
    assert any([op for op, _ in r["cigar"]] == ["S", "N"] and r["cigar"][1][1] >= 100_000 for r in parsed)
    assert any(r["flag"] & 4 and r["cigar"] and X.end_pos(r) == r["pos"] + 1 for r in parsed)
    assert {r["ref_id"] for r in parsed} == {-1, 0, 1, 2}
    assert {len(r["name"]) % 4 for r in parsed} == {0, 1, 2, 3} and {r["start"] % 4 for r in parsed} == {0, 1, 2, 3}
    assert any(X.end_pos(r) > 1 << 31 and r["pos"] < 1 << 31 for r in parsed)
    assert any(X.in_region(r, *X.TABLE_REGIONS[0]) and r["flag"] & 3328 for r in parsed)
    for region in X.TABLE_REGIONS:
        assert 0 < sum(X.in_region(r, *region) for r in parsed) < len(parsed)


@pytest.mark.parametrize("region", X.TABLE_REGIONS)
@pytest.mark.parametrize("n", COUNTS)
def test_keep_set_and_block(ctx, table, n, region):
    recs, parsed = table[n]
    a = _arena(ctx, recs)
    try:
        assert a.bam_set_region(*region) == sum(X.in_region(r, *region) for r in parsed)
        for exclude in (3328, 0):
            want = _want(parsed, region, exclude)
            blk, runs = a.bam_parse(exclude)
            try:
                _check_block(blk, [r["seq"].encode() for r in want])
                starts = [(i, r["ref_id"]) for i, r in enumerate(want) if i == 0 or want[i - 1]["ref_id"] != r["ref_id"]]
                assert [tuple(x) for x in runs.tolist()] == starts
            finally:
                blk.free()
    finally:
        a.close()


@pytest.mark.parametrize("n", (65, 257, 70_000))
def test_every_entry_point_agrees_on_the_kept_set(ctx, table, n):
    recs, parsed = table[n]
    region = X.TABLE_REGIONS[0]
    want = _want(parsed, region, 3328)
    a = _arena(ctx, recs)
    try:
        a.bam_set_region(*region)
        blk, _ = a.bam_parse_filter(10, 3328)
        assert blk.n == len(want)
        blk.free()
        start, nbytes = a.bam_locate(len(want))
        ends = [r["start"] for r in parsed[1:]] + [sum(map(len, recs))]
        size_of = {r["start"]: e - r["start"] for r, e in zip(parsed, ends)}
        assert start.tolist() == [r["start"] for r in want] and nbytes.tolist() == [size_of[r["start"]] for r in want]
        hashes = a.bam_name_hashes(len(want))
        assert len(hashes) == len(want)
        kept_starts = {r["start"] for r in want}
        ref = _arena(ctx, [rec for rec, r in zip(recs, parsed) if r["start"] in kept_starts])  # the same records alone, no region
        try:
            assert np.array_equal(ref.bam_name_hashes(len(want)), hashes)
        finally:
            ref.close()
        picked = hashes[::3]
        names = capi.NameSet(ctx, picked)
        try:
            mask, n_kept, n_marked = a.bam_mark_names(names)
            assert n_kept == len(want)
            bits = [(int(mask[i >> 6]) >> (i & 63)) & 1 for i in range(n_kept)]
            in_set = set(picked.tolist())
            assert bits == [int(h in in_set) for h in hashes.tolist()] and n_marked == sum(bits)
            blob = a.bam_gather(mask, n_kept)
            data = b"".join(recs)
            assert blob == b"".join(data[r["start"]:r["start"] + size_of[r["start"]]] for r, b in zip(want, bits) if b)
        finally:
            names.free()
        with pytest.raises(capi.RufusError):  # the count without the region is no longer the arena's
            a.bam_locate(sum(1 for r in parsed if not r["flag"] & 3328))
    finally:
        a.close()


def test_reset_and_a_new_settle_bring_the_old_behaviour_back(ctx, table):
    recs, parsed = table[257]
    everything = [r["seq"].encode() for r in parsed if not r["flag"] & 3328]
    a = _arena(ctx, recs)
    try:
        a.bam_set_region(*X.TABLE_REGIONS[0])
        blk, _ = a.bam_parse()
        assert blk.n < len(everything)
        blk.free()
        a.reset()
        a.append(b"".join(recs))
        assert a.bam_settle(None, 0, N_REF) == (len(recs), 0)
        blk, _ = a.bam_parse()
        try:
            _check_block(blk, everything)
        finally:
            blk.free()
        # a settle alone (no reset) drops the region as well: the record numbering it belonged to is gone
        a.bam_set_region(*X.TABLE_REGIONS[0])
        assert a.bam_settle(None, 0, N_REF) == (len(recs), 0)
        blk, _ = a.bam_parse()
        assert blk.n == len(everything)
        blk.free()
        # and a second region replaces the first
        a.bam_set_region(*X.TABLE_REGIONS[0])
        assert a.bam_set_region(*X.TABLE_REGIONS[1]) == sum(X.in_region(r, *X.TABLE_REGIONS[1]) for r in parsed)
        blk, _ = a.bam_parse()
        assert blk.n == len(_want(parsed, X.TABLE_REGIONS[1], 3328))
        blk.free()
    finally:
        a.close()


def test_an_unsettled_arena_is_refused(ctx, table):
    recs, _ = table[65]
    a = capi.TextArena(ctx, 1 << 20)
    try:
        a.append(b"".join(recs))
        with pytest.raises(capi.RufusError, match=r"\(-2\)"):
            a.bam_set_region(*X.TABLE_REGIONS[0])
        a.bam_settle(None, 0, N_REF)
        a.bam_set_region(*X.TABLE_REGIONS[0])
        a.reset()
        with pytest.raises(capi.RufusError, match=r"\(-2\)"):
            a.bam_set_region(*X.TABLE_REGIONS[0])
    finally:
        a.close()
