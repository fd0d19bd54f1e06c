"""GPU, C-ABI through capi: rfx_bam_gather_hits (k_bamh_pick, k_bamh_table), the device side of `RUFUS.Filter.single --bam`
-- the records of a settled arena whose count of hit windows reaches the threshold, with that count and their kept index.

The reference is plain Python: the oracle's single-end scan of every kept record's printed form (tests/filter_single_ref.py)
decides what is selected and with which count, slices of the inflated bytes are the records.  Record counts 0, 1, 63, 64,
65, 128, 129 (the ballot per 64 records, the last wave's idle lanes) and 700 (several workgroups); selections none, all, the
first, the last, the two sides of a wave's edge, every third.  Fails without the feature: the entry point does not exist."""
import ctypes as C

import numpy as np
import pytest

import oracle
from rufus_amd import capi
from tests import bai_ref as X
from tests import bam_ref as R
from tests import filter_bam_ref as FB
from tests import filter_single_ref as S

pytestmark = pytest.mark.gpu
K, MIN_Q = S.K, S.MIN_Q
COUNTS = (0, 1, 63, 64, 65, 128, 129, 700)
N_REF = len(R.REFS)


@pytest.fixture(scope="module")
def plant():
    return S.make_plant(400, 5)


def _arena(ctx, recs):
    """One settled arena of raw records."""
    data = b"".join(recs)
    a = capi.TextArena(ctx, len(data) + 65536)
    if data:
        a.append(data)
    assert a.bam_settle(None, 0, N_REF) == (len(recs), 0)
    return a


def _mset(ctx, hl):
    return capi.MutantSet(ctx, capi.hashlist_keys(hl, K, single_end=True), K)


def _hits(hl, parsed, single_end=True, min_q=MIN_Q):
    fs = oracle.FilterSet(hl, single_end=True)
    return [S.single_scan(fs, r, K, min_q, single_end=single_end) for r in parsed]


def _check(a, mset, recs, hits, thresh, last_base_skipped=False, min_q=MIN_Q):
    """bam_gather_hits of arena `a`, whose kept records are `recs` (raw bytes) with the oracle's counts `hits`."""
    blk, _ = a.bam_parse_filter(min_q)
    try:
        assert blk.n == len(recs)
        blob, got_hits, index = a.bam_gather_hits(mset, blk, thresh, last_base_skipped)
    finally:
        blk.free()
    want = [i for i, h in enumerate(hits) if h >= thresh]
    assert index.tolist() == want
    assert got_hits.tolist() == [hits[i] for i in want]
    assert blob == b"".join(recs[i] for i in want)
    return want


def _sets(n):
    return {"none": [], "all": list(range(n)), "first": [0][:n], "last": [n - 1] if n else [],
            "edge": [i for i in (63, 64) if i < n], "third": list(range(0, n, 3))}


@pytest.mark.parametrize("n", COUNTS)
def test_selection_bytes_counts_and_indices(ctx, plant, n):
    mset = _mset(ctx, plant[1])
    try:
        for key, planted in _sets(n).items():
            recs = S.planted_records(n, planted, plant[0])
            hits = _hits(plant[1], R.read_records(b"".join(recs), 0))
            assert [i for i, h in enumerate(hits) if h] == planted, key  # the file holds what it says, on the oracle's word
            assert not planted or {hits[i] for i in planted} <= {1, 3}
            a = _arena(ctx, recs)
            try:
                assert _check(a, mset, recs, hits, 1) == planted
                sel2 = _check(a, mset, recs, hits, 2)
                assert len(sel2) == len(planted) // 2 and set(sel2) <= set(planted)
                if n == 129:  # the reference's `>=`: a threshold of 0 (or below) selects every kept record, hits or not
                    assert _check(a, mset, recs, hits, 0) == list(range(n))
                    assert _check(a, mset, recs, hits, -3) == list(range(n))
            finally:
                a.close()
    finally:
        mset.free()


@pytest.fixture(scope="module")
def crafted():
    blob, hl, special = S.crafted_single()
    bam = R.Bam(blob)
    return bam, hl, special, FB.record_slices(bam)


def test_the_last_base_is_examined_unless_told_otherwise(ctx, crafted):
    bam, hl, special, slices = crafted
    kept = bam.kept()
    at = [i for i, r in enumerate(kept) if FB.qname(r) == special["last_base"]]
    assert len(at) == 1
    single, paired = _hits(hl, kept), _hits(hl, kept, single_end=False)
    assert single[at[0]] == 1 and paired[at[0]] == 0
    hdr = capi.bam_header(bam.bam)
    a = capi.TextArena(ctx, len(bam.data) + 65536)
    mset = _mset(ctx, hl)
    try:
        a.append_bgzf(bam.bam[hdr["first_block"]:])
        assert a.bam_settle(None, hdr["skip"], hdr["n_ref"]) == (len(bam.records), 0)
        assert at[0] in _check(a, mset, slices, single, 1, last_base_skipped=False)
        assert at[0] not in _check(a, mset, slices, paired, 1, last_base_skipped=True)
        _check(a, mset, slices, single, 2)
        _check(a, mset, slices, single, 100)  # (only the reads wholly inside the plant)
    finally:
        mset.free()
        a.close()


def test_a_set_beyond_the_lds_tables_and_the_child_hash_list(ctx):
    # >= 2100 k-mers: with their reverse complements more than 4096 keys, so the pair filter in its counting mode ran
    plant, hl = S.make_plant(2124 + K, 9)
    assert hl.count(b"\n") >= 2100
    mset = _mset(ctx, hl)
    try:
        assert int(capi.lib().rfx_set_size(mset._h)) > 4096
        recs = S.planted_records(300, range(0, 300, 4), plant)
        hits = _hits(hl, R.read_records(b"".join(recs), 0))
        a = _arena(ctx, recs)
        try:
            assert _check(a, mset, recs, hits, 1) == list(range(0, 300, 4))
            _check(a, mset, recs, hits, 2)
        finally:
            a.close()
    finally:
        mset.free()
    # the 50 k-mers of the Child fixture on the Child fixture
    bam = R.Bam(R.fixture("Child"))
    hl = open(R.GOLDEN + "/Child.k25_c5.HashList", "rb").read()
    assert hl.count(b"\n") == 50
    hits = _hits(hl, bam.kept())
    assert sum(h >= 1 for h in hits) >= 26
    hdr = capi.bam_header(bam.bam)
    a = capi.TextArena(ctx, len(bam.data) + 65536)
    mset = _mset(ctx, hl)
    try:
        a.append_bgzf(bam.bam[hdr["first_block"]:])
        a.bam_settle(None, hdr["skip"], hdr["n_ref"])
        for thresh in (1, 2):
            _check(a, mset, FB.record_slices(bam), hits, thresh)
    finally:
        mset.free()
        a.close()


def test_only_records_inside_the_region_can_be_selected(ctx):
    bam = R.Bam(R.synthetic())
    region = (1, 0, 500_000)
    ends = bam.starts[1:] + [len(bam.data)]
    kept = [(r, bam.data[s:e]) for r, s, e in zip(bam.records, bam.starts, ends) if not r["flag"] & 3328]
    inside = [(r, raw) for r, raw in kept if X.in_region(r, *region)]
    outside = [(r, raw) for r, raw in kept if not X.in_region(r, *region)]
    assert len(inside) >= 20 and len(outside) >= 20

    def windows(group):  # a few 25-mers of a few printed reads of the group that have qualities
        seqs = [FB.stranded_printed(r)[0] for r, _ in group if r["l_seq"] and r["qual"][0] != 0xFF]
        seqs = [s for s in seqs if len(s) >= 60 and set(s) <= set(b"ACGT")][:5]
        assert len(seqs) == 5
        return b"".join(s[i:i + K] + b" 9\n" for s in seqs for i in range(0, len(s) - K + 1, 7))

    hl = windows(inside) + windows(outside)
    hits_in = _hits(hl, [r for r, _ in inside], min_q=0)  # (MinQ 0: the file's qualities are random, 0 .. 41)
    assert sum(h >= 1 for h in _hits(hl, [r for r, _ in outside], min_q=0)) >= 5 and 5 <= sum(h >= 1 for h in hits_in) < len(inside)
    hdr = capi.bam_header(bam.bam)
    a = capi.TextArena(ctx, len(bam.data) + 65536)
    mset = _mset(ctx, hl)
    try:
        a.append_bgzf(bam.bam[hdr["first_block"]:])
        a.bam_settle(None, hdr["skip"], hdr["n_ref"])
        a.bam_set_region(*region)
        for thresh in (1, 0):  # (0: every kept record of the region and no other)
            _check(a, mset, [raw for _, raw in inside], hits_in, thresh, min_q=0)
    finally:
        mset.free()
        a.close()


def test_refusals(ctx, plant):
    n = 130
    planted = list(range(0, n, 5))
    recs = S.planted_records(n, planted, plant[0])
    hits = _hits(plant[1], R.read_records(b"".join(recs), 0))
    want = b"".join(recs[i] for i in planted)
    mset = _mset(ctx, plant[1])
    a = _arena(ctx, recs)
    other = capi.Context(0)
    try:
        blk, _ = a.bam_parse_filter(MIN_Q)
        out, h, ix = np.zeros(len(want), np.uint8), np.zeros(len(planted), np.uint32), np.zeros(len(planted), np.uint32)
        # a buffer one too small, either of them: both totals set, nothing written; then the retry
        for kw in ({"cap": len(want) - 1}, {"sel_cap": len(planted) - 1}):
            assert a.bam_gather_hits_into(mset, blk, 1, False, out, h, ix, **kw) == (capi.E_RANGE, len(want), len(planted))
            assert "rfx_bam_gather_hits" in capi.lib().rfx_last_error().decode()
            assert not out.any() and not h.any() and not ix.any()
        assert a.bam_gather_hits_into(mset, blk, 1, False, out, h, ix) == (0, len(want), len(planted))
        assert out.tobytes() == want and ix.tolist() == planted and h.tolist() == [hits[i] for i in planted]
        # the index is optional
        out[:] = 0
        assert a.bam_gather_hits_into(mset, blk, 1, False, out, h, None) == (0, len(want), len(planted)) and out.tobytes() == want
        # a block of another arena state: the region leaves fewer kept records than the block holds
        assert a.bam_set_region(0, 0, 50) < n
        with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_gather_hits"):
            a.bam_gather_hits(mset, blk, 1)
        blk.free()
        blk, _ = a.bam_parse_filter(MIN_Q)  # ... and the block of this state is taken
        _check(a, mset, [raw for raw, r in zip(recs, R.read_records(b"".join(recs), 0)) if X.in_region(r, 0, 0, 50)],
               [h_ for h_, r in zip(hits, R.read_records(b"".join(recs), 0)) if X.in_region(r, 0, 0, 50)], 1)
        # mismatched contexts: the set of another context
        mset2 = _mset(other, plant[1])
        try:
            with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_gather_hits"):
                a.bam_gather_hits(mset2, blk, 1)
        finally:
            mset2.free()
        # a NULL block: refused with both totals cleared
        nb, ns = C.c_uint64(7), C.c_uint64(7)
        rc = capi.lib().rfx_bam_gather_hits(a._h, 3328, mset._h, None, 1, 0, None, 0, C.byref(nb), None, None, 0, C.byref(ns))
        assert rc == -2 and (nb.value, ns.value) == (0, 0)
        # an arena that is not settled
        a.reset()
        a.append(b"".join(recs))
        with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_gather_hits.*settled"):
            a.bam_gather_hits(mset, blk, 1)
        blk.free()
        # no kept record: valid, empty
        a.bam_settle(None, 0, N_REF)
        a.bam_set_region(4, 0, 10)
        blk, _ = a.bam_parse_filter(MIN_Q)
        assert blk.n == 0
        got = a.bam_gather_hits(mset, blk, 0)
        assert got[0] == b"" and len(got[1]) == 0 and len(got[2]) == 0
        blk.free()
    finally:
        other.close()
        mset.free()
        a.close()


def test_tools_filter_bam_single_equals_the_statement(ctx, crafted):
    from rufus_amd import tools
    bam, hl, _, _ = crafted
    for thresh in (1, 2):
        text, log, idx, _ = S.expected_single(bam, hl, thresh=thresh)
        assert len(idx) >= 400
        for arena in (64 << 20, 1 << 20):
            assert tools.filter_bam_single(ctx, bam.bam, hl, K, MIN_Q, thresh, arena_bytes=arena) == (text, log)
    # a region, through the index and without it; a hash list that hits nothing: an empty file, the log all the same
    region = X.parse_region("chr2:1200-1500", [n for n, _ in bam.refs])
    want = S.expected_single(bam, hl, records=[r for r in bam.kept() if X.in_region(r, *region)])[:2]
    for index in (None, X.build(bam, "fine", "next")):
        assert tools.filter_bam_single(ctx, bam.bam, hl, K, MIN_Q, 1, arena_bytes=1 << 20, region="chr2:1200-1500", index=index) == want
    absent = b"".join(b"ACGT"[i % 4:i % 4 + 1] * 25 + b" 7\n" for i in range(4))
    assert tools.filter_bam_single(ctx, bam.bam, absent, K, MIN_Q, 1, arena_bytes=1 << 20) == (b"", bam.chr_log())
