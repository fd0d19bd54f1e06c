"""CPU-only: bench.py --dump-outputs -- what the last timed step computed, as exact float64 arrays within 64 MB."""
import os

import numpy as np

import bench
from rufus_amd import tools


class _Block:
    def __init__(self, n):
        self.n = n


def _mask(bits):
    """A packed per-read hit mask as the filter leaves it: uint64 words, bits past the block's reads set (padding)."""
    pad = np.ones((-len(bits)) % 64 + 64, bool)
    return np.packbits(np.concatenate([bits, pad]), bitorder="little").view(np.uint64)


def test_step_outputs_are_exact():
    rng = np.random.default_rng(3)
    blocks = [_Block(1000), _Block(77), _Block(4096)]
    masks = [_mask(rng.random(b.n) < 0.05) for b in blocks]
    keys = rng.integers(0, 1 << 62, 50, dtype=np.uint64)
    res = {"mutant_keys": keys, "histos": [np.arange(10002, dtype=np.uint64)] * 3, "n_records": [5, 6, 7],
           "hit_masks": masks}
    out = bench.step_outputs(res, {"_samples": [blocks]})
    want, base = [], 0
    for m, b in zip(masks, blocks):
        want.append(base + np.flatnonzero(tools._mask_bits(m, b.n)))
        base += b.n
    assert np.array_equal(out["hit_reads"], np.concatenate(want))
    hi, lo = out["mutant_keys"][:, 0], out["mutant_keys"][:, 1]
    assert np.array_equal((hi << np.uint64(32)) | lo, keys)
    # s1: the pulled pairs of the subject
    s1 = {k: v for k, v in res.items() if k != "hit_masks"}
    out = bench.step_outputs({**s1, "pulled": np.array([0, 1, 0, 1, 1], bool)}, {})
    assert "hit_reads" not in out and np.array_equal(out["pulled_pairs"], [1, 3, 4])


def test_dump_is_float64_exact_and_bounded(tmp_path, monkeypatch):
    keys = np.array([(1 << 62) - 1, 12345, 1 << 40], dtype=np.uint64)
    out = bench.step_outputs({"mutant_keys": keys, "histos": [np.zeros(4, np.uint64)], "n_records": [9],
                              "pulled": np.array([True, False])}, {})
    assert bench.dump_outputs(str(tmp_path / "a"), out) == {}
    k = np.load(tmp_path / "a" / "mutant_keys.npy")
    assert k.dtype == np.float64
    assert np.array_equal((k[:, 0].astype(np.uint64) << np.uint64(32)) | k[:, 1].astype(np.uint64), keys)
    assert sorted(os.listdir(tmp_path / "a")) == ["histograms.npy", "mutant_keys.npy", "pulled_pairs.npy",
                                                  "records_per_sample.npy"]
    # past the budget: a fixed sample of rows, the same on every run, and the whole dump within the budget
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    big = {"a": np.arange(100_000), "b": np.arange(10), "c": np.arange(20_000).reshape(-1, 2)}
    for d in ("x", "y"):
        sampled = bench.dump_outputs(str(tmp_path / d), big)
        assert set(sampled) == {"a", "c"}
    total = 0
    for n in big:
        x, y = np.load(tmp_path / "x" / f"{n}.npy"), np.load(tmp_path / "y" / f"{n}.npy")
        assert np.array_equal(x, y) and x.dtype == np.float64
        total += x.nbytes
    assert total <= 4096
    assert np.array_equal(np.load(tmp_path / "x" / "b.npy"), np.arange(10))
