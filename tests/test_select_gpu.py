"""GPU: reads selected by mask into a block of their own (rfx_select.hip), through the C-ABI.

(a) ``ReadBlock.select`` / ``origin`` equal the numpy statement (tests/select_ref.py, itself checked against the host packer
over text in tests/test_select_host.py) byte for byte, from dense and compact sources, with and without ``good`` / the ACGT
mask; (b) a selected block is an ordinary block: it counts like its text; (c) ``MutantSet.pull_many`` = ``filter_many`` +
``select`` per block, concatenated; (d) the reference's own test trio: the 26 pairs RUFUS.Filter pulls; (e) the trio driver's
``run(pull=True)``; (f) refusals."""
import numpy as np
import pytest

import oracle
from rufus_amd import capi, tools, wgs
from tests import select_ref as ref

pytestmark = pytest.mark.gpu
MIN_Q = 15
BOTH = capi.PACK_COUNT | capi.PACK_FILTER
ARRAYS = ("codes", "acgt", "good", "word_off", "len")


def _get(blk, want_good=True, want_acgt=True):
    return blk.get(want_good=want_good, want_acgt=want_acgt)


def _assert_same_block(blk, want: dict, origin, what, block_idx=None):
    """`blk` holds exactly the arrays of `want` (None: the block must lack that array) and the origin."""
    n = len(want["len"])
    L = capi.lib()
    assert blk.n == n and int(L.rfx_reads_count(blk._h)) == n, what
    assert int(L.rfx_reads_words(blk._h)) == int(want["word_off"][-1]), what
    assert int(L.rfx_reads_bases(blk._h)) == int(want["len"].astype(np.uint64).sum()), what
    got = _get(blk, want_good=want["good"] is not None, want_acgt=want["acgt"] is not None)
    for key in ARRAYS:
        if want[key] is None:
            with pytest.raises(capi.RufusError):            # the result lacks what the source lacks
                _get(blk, want_good=key == "good", want_acgt=key == "acgt")
        else:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)
    ob, orr = blk.origin()
    assert ob.dtype == np.uint32 and orr.dtype == np.uint32
    assert np.array_equal(orr, origin), what
    assert np.array_equal(ob, np.zeros(n, np.uint32) if block_idx is None else block_idx), what


# ---------------------------------------------------------------------------------------------------
# (a) against the numpy statement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.READ_COUNTS)
def test_select_from_a_dense_block(ctx, n):
    rng = np.random.default_rng(2000 + n)
    seqs, quals = ref.ragged_reads(rng, n)
    blk = ctx.upload(capi.PackedReads.from_reads(seqs, quals, MIN_Q, BOTH))
    try:
        whole = _get(blk)
        for name, mask in ref.masks_for(rng, n).items():
            for pairs in (False, True):
                want, origin = ref.select_packed(whole, n, mask, pairs)
                sel = blk.select(mask, pairs=pairs)
                try:
                    _assert_same_block(sel, want, origin, (n, name, pairs))
                finally:
                    sel.free()
    finally:
        blk.free()


@pytest.mark.parametrize("flags,missing", [(capi.PACK_COUNT, "good"), (capi.PACK_FILTER, "acgt")])
def test_select_keeps_what_the_source_has(ctx, flags, missing):
    rng = np.random.default_rng(7)
    n = 129
    seqs, quals = ref.ragged_reads(rng, n)
    blk = ctx.upload(capi.PackedReads.from_reads(seqs, quals, MIN_Q, flags))
    try:
        whole = _get(blk, want_good=missing != "good", want_acgt=missing != "acgt")
        assert whole[missing] is None
        mask = ref.masks_for(rng, n)["random+garbage"]
        want, origin = ref.select_packed(whole, n, mask, True)
        sel = blk.select(mask, pairs=True)
        try:
            _assert_same_block(sel, want, origin, missing)
        finally:
            sel.free()
    finally:
        blk.free()


@pytest.mark.parametrize("read_len,want_good", [(100, True), (150, False)])
def test_select_from_a_compact_block(ctx, read_len, want_good):
    """A compact source: reads of one length (4 and 5 words), the ACGT mask kept only for the reads with an N -- some
    reads carry a mask entry, most do not, and a selected read has flagged reads before and after it in its group of 64."""
    sy = capi.Synth.sample(200_000, 0, n_snv=4, seed=31, read_len=read_len)
    assert sy.n_1024 > 0
    n_pairs = 3000
    n = 2 * n_pairs
    seq, _ = sy.text(0, n_pairs)
    flagged = (seq == ord("N")).any(axis=1)
    assert 0 < flagged.mean() < 0.5
    rng = np.random.default_rng(read_len)
    mask = ref.masks_for(rng, n)["random"]
    mask &= rng.integers(0, 1 << 63, len(mask), dtype=np.uint64) & rng.integers(0, 1 << 63, len(mask), dtype=np.uint64)   # 1 in 8
    picked = ref.selected_reads(mask, n, False)
    assert any(flagged[r - r % 64:r].any() and flagged[r + 1:r - r % 64 + 64].any() for r in picked)
    assert flagged[picked].any() and not flagged[picked].all()
    blk = ctx.synth_reads(sy, 0, n_pairs, MIN_Q, want_good=want_good, compact=True)
    try:
        whole = _get(blk, want_good=want_good)                  # the dense arrays rfx_reads_get makes of the compact form
        assert np.array_equal(whole["len"], np.full(n, read_len, np.uint32))
        for pairs in (False, True):
            want, origin = ref.select_packed(whole, n, mask, pairs)
            sel = blk.select(mask, pairs=pairs)
            try:
                _assert_same_block(sel, want, origin, (read_len, pairs))
                assert tools.decode_reads(_get(sel, want_good=want_good)) == [seq[r].tobytes() for r in origin]
            finally:
                sel.free()
    finally:
        blk.free()


# ---------------------------------------------------------------------------------------------------
# (b) the result is an ordinary block
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,size", [(25, 1 << 26), (5, 1 << 10)])
def test_a_selected_block_counts_like_its_text(ctx, k, size):
    """A ragged selection with reads shorter than k and shorter than 32 bases: the count needs the block's exact
    short_cnt, n_bases and max_len.  The source is freed before the selected block is used."""
    rng = np.random.default_rng(k)
    n = 129
    seqs, quals = ref.ragged_reads(rng, n)
    mask = ref.masks_for(rng, n)["random"]
    picked = ref.selected_reads(mask, n, True)
    texts = [seqs[r] for r in picked]
    assert any(len(t) < k for t in texts) and any(len(t) < 32 for t in texts) and any(len(t) > 1024 for t in texts)
    src = ctx.upload(capi.PackedReads.from_reads(seqs, quals, MIN_Q, BOTH))
    sel = src.select(mask, pairs=True)
    src.free()
    t = capi.CountTable(ctx, k, size)
    try:
        t.add(sel)
        rec = t.finish()
        try:
            assert rec.payload() == oracle.count(None, k, size, reads=texts).payload()
        finally:
            rec.free()
    finally:
        t.free()
        sel.free()


# ---------------------------------------------------------------------------------------------------
# (c) filter + pull over several blocks
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pull_case(ctx):
    """Three blocks of one sample -- 1500 synthetic pairs (compact), no read at all, 129 ragged reads (dense) -- and a hash
    list of 2600 k-mers of the genome and the ragged reads, in neighbouring twos so that reads reach thresh = 2 (5200 set
    entries: the pair filter's range, whose thresh = 1 run is mask-only)."""
    k = 25
    sy = capi.Synth.sample(2_000_000, 0, n_snv=4, seed=11)
    rng = np.random.default_rng(3)
    seqs, quals = ref.ragged_reads(rng, 129)
    kmers = set()
    for at in rng.integers(0, sy.genome_len - k - 1, 1250):
        two = sy.genome(int(at), k + 1)
        if set(two) <= set(b"ACGT"):
            kmers |= {two[:k], two[1:]}
    for s in seqs:
        for at in range(0, len(s) - k - 1, 97):
            if set(s[at:at + k + 1]) <= set(b"ACGT"):
                kmers |= {s[at:at + k], s[at + 1:at + k + 1]}
    kmers = sorted(kmers)
    keys = capi.hashlist_keys(b"".join(km + b" 5\n" for km in kmers), k)
    assert len(keys) > 4096
    blocks = [ctx.synth_reads(sy, 0, 1500, MIN_Q, compact=True), ctx.upload(capi.PackedReads.from_reads([], [], MIN_Q, BOTH)),
              ctx.upload(capi.PackedReads.from_reads(seqs, quals, MIN_Q, BOTH))]
    mset = capi.MutantSet(ctx, keys, k)
    yield blocks, mset
    mset.free()
    for b in blocks:
        b.free()


@pytest.mark.parametrize("thresh", [1, 2])
@pytest.mark.parametrize("pairs", [True, False])
def test_pull_many_is_filter_many_plus_select(ctx, pull_case, thresh, pairs):
    blocks, mset = pull_case
    want_masks = [(m.copy(), nh) for m, nh in mset.filter_many(blocks, thresh)]     # (views of a buffer the next call reuses)
    parts, origins = [], []
    for b, (m, _) in zip(blocks, want_masks):
        sel = b.select(m, pairs=pairs)
        parts.append(_get(sel))
        origins.append(sel.origin()[1])
        sel.free()
    assert sum(nh for _, nh in want_masks) > 20 and len(origins[0]) > 20 and len(origins[1]) == 0
    want = {key: np.concatenate([p[key] for p in parts]) for key in ("codes", "acgt", "good", "len")}
    base = np.cumsum([0] + [int(p["word_off"][-1]) for p in parts])
    want["word_off"] = np.concatenate([p["word_off"][:-1] + np.uint32(b0) for p, b0 in zip(parts, base)]
                                      + [np.array([base[-1]], np.uint32)]).astype(np.uint32)
    pulled, got_masks = mset.pull_many(blocks, thresh, pairs=pairs)
    try:
        for b, (m, nh), (wm, wnh) in zip(blocks, got_masks, want_masks):
            nw = (b.n + 63) // 64
            assert np.array_equal(m[:nw], wm[:nw]) and nh == wnh
        _assert_same_block(pulled, want, np.concatenate(origins),
                           (thresh, pairs), block_idx=np.concatenate([np.full(len(o), i, np.uint32) for i, o in enumerate(origins)]))
    finally:
        pulled.free()
    quiet, none = mset.pull_many(blocks, thresh, pairs=pairs, want_masks=False)        # the masks stay on the device
    try:
        assert all(m is None for m, _ in none) and [nh for _, nh in none] == [nh for _, nh in want_masks]
        _assert_same_block(quiet, want, np.concatenate(origins), "no masks",
                           block_idx=np.concatenate([np.full(len(o), i, np.uint32) for i, o in enumerate(origins)]))
    finally:
        quiet.free()


def test_pull_many_of_no_block(ctx, pull_case):
    _, mset = pull_case
    blk, res = mset.pull_many([])
    try:
        assert blk.n == 0 and res == []
        got = _get(blk, want_acgt=False, want_good=False)
        assert got["word_off"].tolist() == [0] and len(got["codes"]) == 0
        assert all(len(a) == 0 for a in blk.origin())
    finally:
        blk.free()


# ---------------------------------------------------------------------------------------------------
# (d) the reference's test trio
# ---------------------------------------------------------------------------------------------------
def test_testrun_pulls_the_pairs_the_reference_writes(ctx, testrun):
    k = 25
    (h1, s1, _, q1), (h2, s2, _, q2) = (tools.parse_fastq4(m) for m in testrun["Child"])
    assert len(s1) == len(s2)
    seqs = [s for pair in zip(s1, s2) for s in pair]            # read 2p = mate 1, 2p + 1 = mate 2
    quals = [q for pair in zip(q1, q2) for q in pair]
    blk = ctx.upload(capi.PackedReads.from_reads(seqs, quals, MIN_Q, BOTH))
    mset = capi.MutantSet(ctx, capi.hashlist_keys(testrun["hashlist"].encode(), k), k)
    try:
        pulled, _ = mset.pull_many([blk], 1, last_base_skipped=True, pairs=True)
        try:
            _, orr = pulled.origin()
            names = testrun["expected"]["filter_paired_names"]
            assert len(names) == 26 and pulled.n == 52
            assert {h1[r // 2].decode() for r in orr} == set(names)
            assert tools.decode_reads(_get(pulled)) == [seqs[r] for r in orr]
        finally:
            pulled.free()
    finally:
        mset.free()
        blk.free()


# ---------------------------------------------------------------------------------------------------
# (e) the trio driver
# ---------------------------------------------------------------------------------------------------
def test_the_driver_hands_the_pulled_pairs_back(ctx):
    k, n_pairs, block_pairs = 25, 6000, 2000
    sys_ = [capi.Synth.sample(60_000, w, n_snv=8, seed=3) for w in range(3)]
    samples = [wgs.make_sample(ctx, sy, n_pairs, block_pairs, MIN_Q, want_good=(i == 0)) for i, sy in enumerate(sys_)]
    trio = wgs.WgsTrio(ctx, k, 8 << 30, 2, 5, 1200, 1)
    ctx.prof(True)
    try:
        ctx.prof_reset()
        plain = trio.run(samples)
        assert "pulled" not in plain
        assert not [name for name in ctx.prof_dict() if name.startswith("k_select")]
        ctx.prof_reset()
        res = trio.run(samples, pull=True)
        assert {"k_select_words", "k_select_table", "k_select_copy"} <= set(ctx.prof_dict())
        pulled = res["pulled"]
        try:
            assert sorted(set(res) - {"pulled"}) == sorted(plain)
            for key in ("n_mutant", "n_pulled_local", "n_pulled", "n_records"):
                assert res[key] == plain[key], key
            assert res["n_pulled"] > 0 and len(res["hit_masks"]) == len(samples[0]) == 3
            for key in ("mutant_keys", "mutant_counts"):
                assert np.array_equal(res[key], plain[key]), key
            for key in ("histos", "hit_masks"):
                assert len(res[key]) == len(plain[key]) and all(np.array_equal(a, b) for a, b in zip(res[key], plain[key])), key
            assert res["n_pulled_local"] == sum(wgs.pulled_pairs(m, b.n) for m, b in zip(res["hit_masks"], samples[0]))
            assert pulled["block"].n == 2 * res["n_pulled_local"]
            # = select of the subject's blocks by the hit masks
            at = 0
            got = _get(pulled["block"])
            seq, _ = sys_[0].text(0, n_pairs)
            texts = []
            for i, (b, m) in enumerate(zip(samples[0], res["hit_masks"])):
                sel = b.select(m, pairs=True)
                try:
                    part, orr = _get(sel), sel.origin()[1]
                finally:
                    sel.free()
                w0 = int(got["word_off"][at])
                for key in ("codes", "acgt", "good"):
                    assert got[key][w0:w0 + len(part[key])].tobytes() == part[key].tobytes(), (i, key)
                assert np.array_equal(got["len"][at:at + sel.n], part["len"])
                assert np.array_equal(got["word_off"][at:at + sel.n + 1] - np.uint32(w0), part["word_off"])
                assert np.array_equal(pulled["origin_block"][at:at + sel.n], np.full(sel.n, i, np.uint32))
                assert np.array_equal(pulled["origin_read"][at:at + sel.n], orr)
                texts += [seq[2 * i * block_pairs + int(r)].tobytes() for r in orr]
                at += sel.n
            assert at == pulled["block"].n
            assert tools.decode_reads(got) == texts              # rfx_synth_text of the pulled pairs
        finally:
            pulled["block"].free()
    finally:
        ctx.prof(False)
        trio.close()
        for s in samples:
            for b in s:
                b.free()


# ---------------------------------------------------------------------------------------------------
# (f) refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals(ctx, pull_case):
    blocks, mset = pull_case
    L = capi.lib()
    blk = blocks[2]
    mask = np.zeros((blk.n + 63) // 64, np.uint64)
    for mode in (-1, 2):
        assert not L.rfx_reads_select(ctx._h, blk._h, capi._p(mask, capi.u64p), mode)
        assert L.rfx_last_error().decode().startswith("rfx_reads_select: RFX_E_INVAL")
    assert not L.rfx_reads_select(ctx._h, blk._h, None, capi.SELECT_READS)
    assert L.rfx_last_error().decode().startswith("rfx_reads_select: RFX_E_INVAL")
    arr = (capi.C.c_void_p * 1)(blk._h)
    assert not L.rfx_filter_pull(mset._h, arr, 1, 1, 1, 7, None, None)
    assert L.rfx_last_error().decode().startswith("rfx_filter_pull: RFX_E_INVAL")
    with capi.Context(0) as other:
        assert not L.rfx_reads_select(other._h, blk._h, capi._p(mask, capi.u64p), capi.SELECT_READS)
        assert "RFX_E_INVAL" in L.rfx_last_error().decode()
        foreign = other.upload(capi.PackedReads.from_reads([b"ACGT" * 10], [b"I" * 40], MIN_Q, BOTH))
        try:
            arr = (capi.C.c_void_p * 1)(foreign._h)
            assert not L.rfx_filter_pull(mset._h, arr, 1, 1, 1, capi.SELECT_PAIRS, None, None)
            assert "RFX_E_INVAL" in L.rfx_last_error().decode()
        finally:
            foreign.free()
    count_only = ctx.upload(capi.PackedReads.from_reads([b"ACGT" * 10]))
    try:
        arr = (capi.C.c_void_p * 1)(count_only._h)
        assert not L.rfx_filter_pull(mset._h, arr, 1, 1, 1, capi.SELECT_PAIRS, None, None)      # no `good`
        assert "RFX_E_INVAL" in L.rfx_last_error().decode()
        assert L.rfx_reads_origin(count_only._h, None, None) == capi.E_INVAL                      # an uploaded block
        with pytest.raises(capi.RufusError):
            count_only.origin()
    finally:
        count_only.free()
