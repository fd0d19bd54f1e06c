"""The binned trio route read where it lies (rfx_binned_get / _checksum / _verify / _query), the hash list with counts
(rfx_candidates_get_counts), exclude databases (rfx_candidates_strike_records) and WgsTrio.run(verify="binned"), against
the oracle and against the sorted route.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import oracle
from rufus_amd import capi, tools, wgs
from tests.binned_ref import by_key, np_bin, np_revcomp

pytestmark = pytest.mark.gpu

SIZE, MIN_COV, MAX_DEPTH, MIN_Q, THRESH = 8 << 30, 5, 1200, 15, 1
UPPER = 1000
G, N_PAIRS = 250_000, 25_000


def sum_of_histo(h) -> int:
    return int(sum(int(x) * i for i, x in enumerate(h)))


@functools.lru_cache(maxsize=None)
def reads_of(genome: int, which: int, n_snv: int, seed: int, n_pairs: int, carrier: int = -1):
    sy = capi.Synth.sample(genome, which, n_snv=n_snv, seed=seed)
    if carrier >= 0:
        sy.carrier = carrier
    seq, _ = sy.text(0, n_pairs)
    return tuple(x.tobytes() for x in seq)


@functools.lru_cache(maxsize=None)
def oracle_of(genome: int, which: int, n_snv: int, seed: int, n_pairs: int, k: int, lower: int, upper: int, carrier: int = -1):
    """The oracle's records of a synthetic sample's text: made once, shared, never changed."""
    return oracle.count(None, k, SIZE, lower=lower, upper=upper, reads=reads_of(genome, which, n_snv, seed, n_pairs, carrier))


def table_of(ctx, blocks, k, shard=None):
    t = capi.CountTable(ctx, k, SIZE, True, mode=capi.COUNT_MSP)
    if shard is not None:
        t.set_shard(*shard)
    for b in blocks:
        t.add(b)
    return t


def binned_of(ctx, blocks, k, lower, upper=2**64 - 1, shard=None):
    t = table_of(ctx, blocks, k, shard)
    try:
        return t.finish_binned(lower, upper, want_histo=True)
    finally:
        t.free()


def free_all(*things):
    for x in things:
        for y in (x if isinstance(x, (list, tuple)) else [x]):
            y.free()


# ---- 1. a store against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [25, 31])
@pytest.mark.parametrize("lower", [1, 2])
def test_store_against_oracle(ctx, k, lower):
    sy = capi.Synth.sample(G, 0, n_snv=12, seed=777)
    ref = oracle_of(G, 0, 12, 777, N_PAIRS, k, lower, UPPER)
    blocks = wgs.make_sample(ctx, sy, N_PAIRS, 9000, MIN_Q, want_good=False)
    b = rec = None
    try:
        b, histo = binned_of(ctx, blocks, k, lower, UPPER)
        keys, counts, bins, at = b.get()
        assert len(keys) == len(b) == len(ref.keys)
        gk, gc = by_key(keys, counts)
        rk, rc = by_key(ref.keys, ref.counts)
        assert np.array_equal(gk, rk) and np.array_equal(gc, rc), "the store is not the oracle's multiset"
        assert b.checksum() == oracle.multiset_checksum(ref.keys, ref.counts)
        t2 = table_of(ctx, blocks, k)
        try:
            rec = t2.finish(lower, UPPER)
        finally:
            t2.free()
        assert b.checksum() == rec.checksum()
        v = b.verify(lower, UPPER)
        assert v == {"bad_bin": 0, "bad_count": 0, "not_canonical": 0, "duplicate": 0, "sum_counts": sum_of_histo(histo)}
        assert int(histo[-1]) == 0 and v["sum_counts"] == int(ref.counts.sum())
        assert np.array_equal(bins, np_bin(keys, k, b.bits)), "a survivor's bin is not the bin function of its key"
        assert np.all(np.diff(bins.astype(np.int64)) >= 0), "get() is not in bin order"
        assert len(np.unique(at)) == len(at)
        # lookup: keys the store holds, and canonical keys it does not
        rng = np.random.default_rng(k * 10 + lower)
        pick = rng.choice(len(keys), 1000, replace=False)
        rnd = rng.integers(0, 1 << (2 * k), 1200, dtype=np.uint64)
        rnd = np.minimum(rnd, np_revcomp(rnd, k))
        rnd = np.unique(rnd[~np.isin(rnd, keys)])[:1000]
        assert len(rnd) == 1000
        got = b.query(np.concatenate([keys[pick], rnd]))
        assert np.array_equal(got[:1000], counts[pick]) and not got[1000:].any()
    finally:
        free_all(blocks, [x for x in (b, rec) if x is not None])


# ---- 2. deep bins, chunk switches, shards ----------------------------------------------------------------------------
@pytest.mark.parametrize("stage_test", [False, True])
def test_deep_bins_chunk_switches_shards(ctx, monkeypatch, stage_test):
    """The shape of test_trio_binned_gpu.py::test_tiny_genome_deep_bins, one sample: bins the leaf halves several levels
    deep, a bin's survivors in several staging chunks.  RFX_LEAF_STAGE_TEST=1: the pool comes short and the finish reruns."""
    g, n_pairs, k, lower = 4000, 400_000, 25, 1
    if stage_test:
        monkeypatch.setenv("RFX_LEAF_STAGE_TEST", "1")
    sy = capi.Synth.sample(g, 0, n_snv=4, seed=31)
    ref = oracle_of(g, 0, 4, 31, n_pairs, k, lower, 2**64 - 1)
    blocks = wgs.make_sample(ctx, sy, n_pairs, 1 << 20, MIN_Q, want_good=False)
    stores = []
    try:
        whole, _ = binned_of(ctx, blocks, k, lower)
        stores.append(whole)
        one_pass = whole.checksum()
        assert one_pass == oracle.multiset_checksum(ref.keys, ref.counts)
        whole.free()
        got, sums = [], [0, 0]
        for shard in range(2):
            b, histo = binned_of(ctx, blocks, k, lower, shard=(shard, 2))
            stores.append(b)
            keys, counts, bins, _ = b.get()
            assert len(keys) > 0
            assert np.array_equal(bins, np_bin(keys, k, b.bits))
            v = b.verify(lower)
            # (30 000x of a 4 kb genome: the genome's own k-mers lie beyond the histogram's last bin, which holds them as
            # 10001 each -- the sum of the counts is checked against the survivors themselves)
            assert int(histo[-1]) > 0 and int(histo.sum()) == len(keys)
            assert v == {"bad_bin": 0, "bad_count": 0, "not_canonical": 0, "duplicate": 0,
                         "sum_counts": int(counts.sum(dtype=np.uint64))}
            sums = [(a + c) % (1 << 64) for a, c in zip(sums, b.checksum())]
            got.append((keys, counts))
            b.free()
        assert not np.intersect1d(got[0][0], got[1][0]).size, "the two shards share a k-mer"
        gk, gc = by_key(np.concatenate([got[0][0], got[1][0]]), np.concatenate([got[0][1], got[1][1]]))
        rk, rc = by_key(ref.keys, ref.counts)
        assert np.array_equal(gk, rk) and np.array_equal(gc, rc), "the shards' union is not the oracle's multiset"
        assert tuple(sums) == one_pass
    finally:
        free_all(blocks, stores)


# ---- 3. verify finds what it is for ----------------------------------------------------------------------------------
def test_verify_finds_what_it_is_for(ctx):
    k, lower = 25, 1
    sy = capi.Synth.sample(G, 0, n_snv=12, seed=777)
    blocks = wgs.make_sample(ctx, sy, N_PAIRS, 9000, MIN_Q, want_good=False)
    b = None
    try:
        b, histo = binned_of(ctx, blocks, k, lower, UPPER)
        clean = b.verify(lower, UPPER)
        assert b.verify(lower + 1, UPPER) == dict(clean, bad_count=int(histo[lower]))
        assert int(histo[lower]) > 0
        keys, counts, bins, at = b.get()
        d_keys, _ = b.dev_ptrs()
        same = np.flatnonzero(bins[1:] == bins[:-1])
        assert len(same), "no bin with two survivors: the case does not test what it should"
        i = int(same[0])
        # one survivor's key over its neighbour in the same bin: that bin now holds the key twice
        ctx.memcpy_dev(d_keys + 8 * int(at[i + 1]), d_keys + 8 * int(at[i]), 8)
        v1 = b.verify(lower, UPPER)
        assert v1["duplicate"] >= 1
        assert v1 == dict(clean, duplicate=v1["duplicate"])
        # and over a survivor of another bin: a key that does not lie where its minimizer says
        j = int(np.flatnonzero(bins != bins[i])[0])
        ctx.memcpy_dev(d_keys + 8 * int(at[j]), d_keys + 8 * int(at[i]), 8)
        v2 = b.verify(lower, UPPER)
        assert v2["bad_bin"] >= 1
        assert v2 == dict(v1, bad_bin=v2["bad_bin"])
        # a data check, not a fault: the store still reads
        k2, _, _, _ = b.get()
        assert k2[i + 1] == keys[i] and k2[j] == keys[i] and int((k2 != keys).sum()) == 2
    finally:
        free_all(blocks, [b] if b is not None else [])


# ---- the trio of tests 4 - 6 -------------------------------------------------------------------------------------------
TRIO_SEED, TRIO_SNV, SIB_PAIRS = 777, 12, 1000


@pytest.fixture(scope="module")
def trio_samples(ctx):
    sys_ = [capi.Synth.sample(G, w, n_snv=TRIO_SNV, seed=TRIO_SEED) for w in range(3)]
    samples = [wgs.make_sample(ctx, sy, N_PAIRS, 9000, MIN_Q, want_good=(w == 0)) for w, sy in enumerate(sys_)]
    yield samples
    free_all(*samples)


def run_trio(ctx, samples, passes, monkeypatch=None, sorted_route=False, **kw):
    trio = wgs.WgsTrio(ctx, 25, SIZE, 2, MIN_COV, MAX_DEPTH, THRESH, passes=passes)
    try:
        if sorted_route:
            monkeypatch.setenv("RFX_TRIO_SORTED", "1")
        res = trio.run(samples, **kw)
        if sorted_route:
            monkeypatch.delenv("RFX_TRIO_SORTED")
        assert trio.passes == passes
        return res, trio.binned_counts
    finally:
        trio.close()


def test_hash_list_with_counts(ctx, monkeypatch, trio_samples):
    new, n_binned = run_trio(ctx, trio_samples, 2)
    assert n_binned == 2 * 3, "the binned route was not taken"
    old, n_binned = run_trio(ctx, trio_samples, 2, monkeypatch, sorted_route=True)
    assert n_binned == 0
    assert new["mutant_counts"].dtype == np.uint32 and old["mutant_counts"].dtype == np.uint32
    assert np.array_equal(new["mutant_keys"], old["mutant_keys"])
    assert np.array_equal(new["mutant_counts"], old["mutant_counts"])
    orc = [oracle_of(G, w, TRIO_SNV, TRIO_SEED, N_PAIRS, 25, 2, 2**64 - 1) for w in range(3)]
    want = oracle.hash_list(orc[0], orc[1:], MIN_COV, MAX_DEPTH)
    assert want and tools.hash_list_of_run(new, 25) == want
    assert tools.hash_list_of_run(old, 25) == want


def test_exclude(ctx, monkeypatch, trio_samples):
    """A fourth sample of the same genome -- a sibling that carries the SNVs too, at 1.2x -- as the exclude database: the SNV
    k-mers it saw (133 of the trio's 278 mutant k-mers, by the oracle) fall to it alone, the others stay."""
    sib = capi.Synth.sample(G, 3, n_snv=TRIO_SNV, seed=TRIO_SEED)
    sib.carrier = 1
    blocks = wgs.make_sample(ctx, sib, SIB_PAIRS, 9000, MIN_Q, want_good=False)
    held = []
    try:
        t = table_of(ctx, blocks, 25)
        try:
            rec = t.finish(1)
        finally:
            t.free()
        held.append(rec)
        loaded = capi.Records.load(ctx, 25, rec.lsize, capi.jf_matrix(rec.lsize, 25), rec.payload())
        held.append(loaded)
        plain, _ = run_trio(ctx, trio_samples, 2)
        for ex in (rec, loaded):
            new, n_binned = run_trio(ctx, trio_samples, 2, exclude=[ex])
            assert n_binned == 2 * 3, "the binned route was not taken"
            old, n_binned = run_trio(ctx, trio_samples, 2, monkeypatch, sorted_route=True, exclude=[ex])
            assert n_binned == 0
            assert np.array_equal(new["mutant_keys"], old["mutant_keys"])
            assert np.array_equal(new["mutant_counts"], old["mutant_counts"])
            assert new["n_pulled"] == old["n_pulled"]
            assert 0 < len(new["mutant_keys"]) < len(plain["mutant_keys"]), "no k-mer fell to the exclude alone"
            assert np.isin(new["mutant_keys"], plain["mutant_keys"]).all()
        kept, _ = run_trio(ctx, trio_samples, 1, keep_shard_records=True, exclude=[rec])
        recs = kept["shard_records"][0]
        held += recs
        uk, uc = capi.unique_to_subject(ctx, recs[0], recs[1:] + [rec], MIN_COV, MAX_DEPTH)
        assert np.array_equal(new["mutant_keys"], uk) and np.array_equal(new["mutant_counts"], uc)
        assert np.array_equal(kept["mutant_keys"], uk) and np.array_equal(kept["mutant_counts"], uc)
        # in the oracle's words: the hash list with the exclude among the others
        orc = [oracle_of(G, w, TRIO_SNV, TRIO_SEED, N_PAIRS, 25, 2, 2**64 - 1) for w in range(3)]
        orc_sib = oracle_of(G, 3, TRIO_SNV, TRIO_SEED, SIB_PAIRS, 25, 1, 2**64 - 1, 1)
        assert tools.hash_list_of_run(new, 25) == oracle.hash_list(orc[0], orc[1:] + [orc_sib], MIN_COV, MAX_DEPTH)
    finally:
        free_all(blocks, held)


def test_exclude_of_another_k_is_refused(ctx, trio_samples):
    t27 = table_of(ctx, trio_samples[1], 27)
    try:
        rec27 = t27.finish(2)
    finally:
        t27.free()
    b, _ = binned_of(ctx, trio_samples[0], 25, 2)
    cand = capi.binned_strike(ctx, b, None, MIN_COV, MAX_DEPTH)
    try:
        n0 = len(cand.keys())
        with pytest.raises(capi.RufusError) as e:
            cand.strike_records(rec27)
        assert f"({capi.E_FORMAT})" in str(e.value)
        assert len(cand.keys()) == n0 > 0
    finally:
        free_all(cand, b, rec27)


def test_verify_binned(ctx, trio_samples):
    S = 2
    plain, _ = run_trio(ctx, trio_samples, S)
    keys = plain["mutant_keys"]
    assert len(keys)
    a, n_a = run_trio(ctx, trio_samples, S, verify="binned", probe_keys=keys)
    b, n_b = run_trio(ctx, trio_samples, S + 1, verify="binned", probe_keys=keys)
    assert n_a == S * 3 and n_b == (S + 1) * 3, "the binned route was left"
    old, n_old = run_trio(ctx, trio_samples, S, verify=True, probe_keys=keys)
    assert n_old == 0
    for r in (a, b):
        v = r["verify"]
        assert v["checksum"] == old["verify"]["checksum"]
        assert v["sum_counts"] == old["verify"]["sum_counts"]
        assert v["probe_found"] == [len(keys), 0, 0] and v["probe_count_out_of_range"] == 0
        assert all(v[x] == 0 for x in ("bad_order", "bad_pos", "bad_count", "bad_bin", "duplicate", "not_canonical"))
        assert np.array_equal(r["mutant_keys"], keys) and np.array_equal(r["mutant_counts"], plain["mutant_counts"])
        assert r["n_records"] == plain["n_records"] and r["n_pulled"] == plain["n_pulled"]
    assert set(old["verify"]) == {"bad_order", "bad_pos", "bad_count", "sum_counts", "probe_found", "probe_count_out_of_range",
                                  "checksum"}, "verify=True changed what it reports"


def test_self_check_binned(ctx, trio_samples):
    sys_ = [capi.Synth.sample(G, w, n_snv=TRIO_SNV, seed=TRIO_SEED) for w in range(3)]
    trio = wgs.WgsTrio(ctx, 25, SIZE, 2, MIN_COV, MAX_DEPTH, THRESH, passes=2)
    try:
        res = trio.run(trio_samples)
        out = wgs.self_check_binned(ctx, trio, trio_samples, sys_, res, N_PAIRS)
    finally:
        trio.close()
    assert out["mutant_in_subject"] == len(res["mutant_keys"]) and out["mutant_in_controls"] == 0
    assert out["passes_compared"] == [2, 3]
