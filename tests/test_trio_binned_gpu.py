"""The trio driver's binned route (rufus_amd/wgs.py run(): survivors stay grouped by fine minimizer bin, the controls are
struck off bin against bin) against the sorted route (RFX_TRIO_SORTED=1: rfx_count_finish + rfx_records_subtract) on
what tests/test_scale_gpu.py does not force: bins the leaf halves several levels deep, the recount of a bin, a staging
pool that comes short, survivors of one bin in several chunks, samples whose bin counts differ, no / one control, a
control without reads in a shard, a small input that the sorted route would not refine."""
import numpy as np
import pytest

from rufus_amd import capi, wgs

pytestmark = pytest.mark.gpu

SIZE, MIN_COV, MIN_Q, THRESH = 8 << 30, 5, 15, 1


def _both_routes(ctx, monkeypatch, sys_, n_pairs, k=25, lower=2, max_depth=1200, passes=1, block_pairs=1 << 20, env=()):
    """run() on both routes; asserts that each took the route it was meant to and that they agree; returns the result."""
    samples = [wgs.make_sample(ctx, sy, n, block_pairs, MIN_Q, want_good=(i == 0)) for i, (sy, n) in enumerate(zip(sys_, n_pairs))]
    trio = wgs.WgsTrio(ctx, k, SIZE, lower, MIN_COV, max_depth, THRESH, passes=passes)
    try:
        for name, val in env:
            monkeypatch.setenv(name, val)
        new = trio.run(samples)
        assert trio.binned_counts == trio.passes * len(samples), "the binned route was not taken"
        monkeypatch.setenv("RFX_TRIO_SORTED", "1")
        old = trio.run(samples)
        assert trio.binned_counts == 0, "RFX_TRIO_SORTED=1 did not force the sorted route"
        monkeypatch.delenv("RFX_TRIO_SORTED")
        for name, _ in env:
            monkeypatch.delenv(name)
    finally:
        trio.close()
        for s in samples:
            for b in s:
                b.free()
    assert np.array_equal(new["mutant_keys"], old["mutant_keys"])
    assert new["n_records"] == old["n_records"] and new["n_pulled"] == old["n_pulled"]
    assert len(new["histos"]) == len(old["histos"]) and all(np.array_equal(a, b) for a, b in zip(new["histos"], old["histos"]))
    assert len(new["hit_masks"]) == len(old["hit_masks"])
    assert all(np.array_equal(a, b) for a, b in zip(new["hit_masks"], old["hit_masks"]))
    return new


@pytest.mark.parametrize("lower,force_mixed", [(2, False), (2, True), (1, False)])
def test_tiny_genome_deep_bins(ctx, monkeypatch, lower, force_mixed):
    """4 kb of genome under 8 x 10^5 reads per sample: a few hundred minimizers carry everything, so a bin holds the
    thousands of distinct error k-mers around its stretch of genome and the leaf halves it several times by hash bits
    (12 k distinct k-mers per bin on average against the 3072 / 6144 a pass can take).  RFX_LEAF_FORCE_MIXED=1: every third
    bin is counted a second time without the record cache.  lower = 1: every distinct k-mer survives, a bin's survivors
    are several staging chunks (4352 / 8704 entries each for a small input) -- chunk switches inside a bin."""
    sys_ = [capi.Synth.sample(4000, w, n_snv=4, seed=31) for w in range(3)]
    res = _both_routes(ctx, monkeypatch, sys_, [400_000] * 3, lower=lower, max_depth=1_000_000, passes=2,
                       env=(("RFX_LEAF_FORCE_MIXED", "1"),) if force_mixed else ())
    assert res["n_mutant"] > 0 and res["n_pulled"] > 0


def test_staging_pool_comes_short(ctx, monkeypatch):
    """RFX_LEAF_STAGE_TEST=1: the pool holds no chunk beyond the workgroups' first ones, the leaf raises its flag and the
    finish is run again with the chunks the counter asks for."""
    sys_ = [capi.Synth.sample(250_000, w, n_snv=12, seed=777) for w in range(3)]
    res = _both_routes(ctx, monkeypatch, sys_, [25_000] * 3, passes=2, block_pairs=9000, env=(("RFX_LEAF_STAGE_TEST", "1"),))
    assert res["n_mutant"] > 0


def test_tumor_normal_bin_counts_differ(ctx, monkeypatch):
    """Tumor 60x / normal 30x of 5 Mb, k = 31 (wide records): each table chooses its bin count from its own k-mer count, so
    a bin of the normal is two bins of the tumor."""
    G = 5_000_000
    sys_ = [capi.Synth.sample(G, w, n_snv=40, seed=2024) for w in range(2)]
    n_pairs = [1_000_000, 500_000]
    bits = []
    for sy, n in zip(sys_, n_pairs):
        blocks = wgs.make_sample(ctx, sy, n, 1 << 20, MIN_Q, want_good=False)
        t = capi.CountTable(ctx, 31, SIZE, True, mode=capi.COUNT_MSP)
        try:
            for b in blocks:
                t.add(b)
            bn = t.finish_binned(2)
            bits.append(bn.bits)
            bn.free()
        finally:
            t.free()
            for b in blocks:
                b.free()
    assert bits[0] > bits[1], f"the samples chose the same bin count ({bits}): the case does not test what it should"
    res = _both_routes(ctx, monkeypatch, sys_, n_pairs, k=31)
    assert res["n_mutant"] > 0


@pytest.mark.parametrize("n_samples", [1, 2])
def test_no_control_and_one_control(ctx, monkeypatch, n_samples):
    sys_ = [capi.Synth.sample(250_000, w, n_snv=12, seed=5) for w in range(n_samples)]
    res = _both_routes(ctx, monkeypatch, sys_, [25_000] * n_samples, passes=3, block_pairs=7001)
    assert res["n_mutant"] > 0


@pytest.mark.parametrize("control_pairs", [0, 1])
def test_control_empty_in_a_shard(ctx, monkeypatch, control_pairs):
    """A control of one pair (its ~250 k-mers leave most of eight shard passes without a record) or of no read at all
    between the subject and a full control."""
    sys_ = [capi.Synth.sample(250_000, w, n_snv=12, seed=9) for w in range(3)]
    res = _both_routes(ctx, monkeypatch, sys_, [25_000, control_pairs, 25_000], passes=8)
    assert res["n_mutant"] > 0


def test_small_input_one_pass(ctx, monkeypatch):
    """3000 pairs in one block and one pass: the sorted route counts the block's bins as they are (no refinement); the
    binned route always takes the refined leaf, here with nothing to refine."""
    sys_ = [capi.Synth.sample(60_000, w, n_snv=8, seed=3) for w in range(3)]
    _both_routes(ctx, monkeypatch, sys_, [3000] * 3)
