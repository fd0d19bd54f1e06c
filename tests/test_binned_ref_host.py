"""tests/binned_ref.py, the host reference of tests/test_strike_gpu.py, checked on its own: the planted k-mers lie where they
are said to lie, and the set difference is the one oracle.hash_list prints."""
import numpy as np
import pytest

import oracle
from tests import binned_ref as ref


def keys_of(reads, k):
    return np.array([oracle.jf_encode(r.decode()) for r in reads], np.uint64)


def test_planted_minimizer_is_the_hash_inverted():
    assert ref.planted_minimizer(25) == 0x1E464115 and ref.planted_minimizer(31) == 0x5BD1E995
    for k in (25, 27, 31):
        c, m = ref.planted_minimizer(k), ref.mmer_len(k)
        assert c < 1 << (2 * m) and c <= int(ref.np_revcomp(np.array([c], np.uint64), m)[0])
        assert int(ref.mmer_hash(np.array([c], np.uint64))[0]) < 1 << 12
    h = np.random.default_rng(5).integers(0, 1 << 32, 1000, dtype=np.uint64)
    assert np.array_equal(ref.mmer_hash(ref.mmer_unhash(h)), h)


@pytest.mark.parametrize("k", [25, 27, 31])
def test_planted_kmers_share_a_bin_at_every_bit_count(k):
    """k = 27: the first k whose window is k - 15 (m stays 16 from there on)."""
    reads = ref.kmers_in_one_bin(k, 3000, seed=k)
    assert len(set(reads)) == 3000 and all(len(r) == k for r in reads)
    keys = keys_of(reads, k)
    assert np.array_equal(keys, np.minimum(keys, ref.np_revcomp(keys, k))), "a planted k-mer is not canonical"
    planted = ref.planted_minimizer(k)
    for bits in range(8, 29):
        bins = ref.np_bin(keys, k, bits)
        assert (bins == bins[0]).all() and int(bins[0]) == ref.mmer_bin(planted, bits), f"{bits} bits"
    # one read, one k-mer: the oracle counts each of them once
    ek, ec = ref.expected_store(reads, k, 1)
    assert np.array_equal(np.sort(ek), np.sort(keys)) and (ec == 1).all()


@pytest.mark.parametrize("k", [25, 31])
@pytest.mark.parametrize("coarse,fine", [(16, 17), (14, 18)])
def test_planted_pair_splits_between_coarse_and_fine(k, coarse, fine):
    a, b = ref.planted_pair(k, coarse, fine)
    assert a == ref.planted_minimizer(k) and a != b
    ka, kb = (keys_of(ref.kmers_in_one_bin(k, 200, 7, m), k) for m in (a, b))
    assert not np.intersect1d(ka, kb).size
    both = np.concatenate([ka, kb])
    assert len(np.unique(ref.np_bin(both, k, coarse))) == 1
    fa, fb = ref.np_bin(ka, k, fine), ref.np_bin(kb, k, fine)
    assert len(np.unique(fa)) == 1 and len(np.unique(fb)) == 1 and fa[0] != fb[0]


def test_expected_candidates_is_the_oracles_hash_list(small_trio):
    k, lower, min_cov, max_depth = 25, 2, 5, 1200
    reads = {n: [row.tobytes() for m in (0, 1) for row in small_trio[n].s[m]] for n in ("child", "mother", "father")}
    orc = {n: oracle.count(None, k, ref.SIZE, lower=lower, reads=r) for n, r in reads.items()}
    want = oracle.hash_list(orc["child"], [orc["mother"], orc["father"]], min_cov, max_depth)
    stores = {n: ref.expected_store(r, k, lower) for n, r in reads.items()}
    keys, counts = ref.expected_candidates(stores["child"], [stores["mother"], stores["father"]], min_cov, max_depth)
    assert len(keys) > 0 and np.all(np.diff(keys.astype(np.int64)) > 0)
    lines = [ln.split() for ln in want.splitlines()]
    wk, wc = ref.by_key(np.array([oracle.jf_encode(a) for a, _ in lines], np.uint64), np.array([int(c) for _, c in lines], np.uint64))
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc)
    # and the range bites on both sides: a narrower one drops exactly the records outside it
    k2, c2 = ref.expected_candidates(stores["child"], [stores["mother"], stores["father"]], min_cov + 2, int(counts.max()) - 1)
    inside = (counts >= min_cov + 2) & (counts <= counts.max() - 1)
    assert 0 < len(k2) < len(keys) and np.array_equal(k2, keys[inside]) and np.array_equal(c2, counts[inside])
