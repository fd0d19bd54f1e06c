"""GPU: long sequences are counted through tiles of <= 150 bases cut on the device (rfx_tile.hip).

(a) ``ReadBlock.tile`` equals the host packer over the tile substrings, byte for byte; (b) the counts of a block of long
sequences are the oracle's, on every count path, tiled or not, in one pass or in shard passes from run maps; (c) the default
route runs ``k_reads_tile`` and ``RFX_NO_TILE=1`` does not; (d) the tiled twin lives and dies with its source block; (e) the
drop-in ``jellyfish count`` writes the same database either way.

Run as a module (``python -m tests.test_tile_gpu``) this file is the CHILD of (b) / (c): it counts the same sequences in a
process of its own -- the parent starts it with RFX_NO_TILE=1 -- and prints what it got as JSON."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from rufus_amd import capi, tools
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "rufus_amd", "bin")
SIZE = 1 << 26
ALPHABET = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTacgtNRY\r", dtype=np.uint8)   # mostly ACGT
CLEAN = np.frombuffer(b"ACGT" * 250 + b"acgtacgtNRY\r", dtype=np.uint8)     # 0.4 % non-ACGT: most windows count
COUNT_KS = (15, 25, 31, 32)     # P2L, MSP, MSP (records with a plane), global table


def _random_seq(rng, n, alphabet=ALPHABET):
    return alphabet[rng.integers(0, len(alphabet), n)].copy()


# ---------------------------------------------------------------------------------------------------
# (a) the tiler against the host packer
# ---------------------------------------------------------------------------------------------------
def _tiles(length, k, L):
    n, step = capi.tile_plan(length, k, L)
    if length <= L:
        return [(0, length)]
    return [(t * step, min(L, length - t * step)) for t in range(n)]


def _assert_tiled_equals_packed(blk, seqs, k, L, what):
    subs, starts = [], []
    for s in seqs:
        for start, tl in _tiles(len(s), k, L):
            subs.append(bytes(s[start:start + tl]))
            starts.append(start)
    want = capi.PackedReads.from_reads(subs)
    tiled = blk.tile(k, L)
    try:
        got = tiled.get(want_good=False)
        nw = int(want.word_off[-1])
        assert tiled.n == len(subs), what
        assert tiled.bases == sum(len(s) for s in subs), what
        assert np.array_equal(got["len"], want.len[:len(subs)]), what
        assert np.array_equal(got["word_off"], want.word_off), what
        assert len(got["codes"]) == nw, what
        assert got["codes"].tobytes() == want.codes[:nw].tobytes(), what
        assert got["acgt"].tobytes() == want.acgt[:nw].tobytes(), what
    finally:
        tiled.free()
    return starts


def test_tiling_matches_the_host_packer_byte_for_byte(ctx):
    rng = np.random.default_rng(20261019)
    residues = set()
    for k in (5, 25, 32):
        for L in (k, 33, 64, 127 + k, 150, 160):
            step = L - k + 1
            seqs = []
            for n in (0, k - 1, k, L, L + 1, step * 3 + k - 1, step * 3 + k, 1000, 4099):
                s = _random_seq(rng, n)
                # runs of N across tile boundaries: over the start of tile t and over the end of tile t - 1
                for t in (1, 2, 5, max(1, (n // step) - 1)):
                    for edge, width in ((t * step, 3), (t * step + k - 1, 2), (t * step, 40 if t == 5 else 1)):
                        lo, hi = max(0, edge - width), min(n, edge + width)
                        if lo < hi and t * step < n:
                            s[lo:hi] = ord("N")
                seqs.append(s)
            blk = ctx.upload(capi.PackedReads.from_reads([bytes(s) for s in seqs]))
            try:
                starts = _assert_tiled_equals_packed(blk, seqs, k, L, (k, L))
            finally:
                blk.free()
            residues |= {s % 32 for s in starts}
            if L == 127 + k:
                assert {s % 32 for s in starts} == {0}          # step 128: every tile starts word-aligned (shift 0)
    assert residues == set(range(32))


@pytest.mark.parametrize("with_n", [False, True])
def test_tiling_a_compact_block(ctx, with_n):
    """A compact source block (reads of one length, the ACGT mask kept only for reads with an N): without N no read has
    a mask and the tiles' masks are all ones up to their length."""
    sy = capi.Synth.sample(200_000, 0, n_snv=4, seed=31, read_len=250)
    sy.n_1024 = 8 if with_n else 0
    n_pairs = 700
    seq, _ = sy.text(0, n_pairs)
    seqs = [row for row in seq]
    assert any(ord("N") in r.tobytes() for r in seqs) == with_n
    blk = ctx.synth_reads(sy, 0, n_pairs, want_good=False, compact=True)
    try:
        own = blk.get(want_good=False)
        whole = capi.PackedReads.from_reads([r.tobytes() for r in seqs])
        assert own["codes"].tobytes() == whole.codes[:len(own["codes"])].tobytes()      # the block IS these reads
        assert own["acgt"].tobytes() == whole.acgt[:len(own["acgt"])].tobytes()
        for k, L in ((25, 33), (25, 64), (5, 150), (32, 160)):
            _assert_tiled_equals_packed(blk, seqs, k, L, (with_n, k, L))
    finally:
        blk.free()


# ---------------------------------------------------------------------------------------------------
# (b), (c) counts of long sequences: default route, RFX_NO_TILE=1 in a child process, shard passes from run maps
# ---------------------------------------------------------------------------------------------------
def _long_seqs():
    """Three sequences of 40 000, 70 001 and 3 bases with repeats (counts above 1) and non-ACGT stretches."""
    rng = np.random.default_rng(77)
    a, b = _random_seq(rng, 40_000, CLEAN), _random_seq(rng, 70_001, CLEAN)
    b[10_000:25_000] = a[5_000:20_000]          # a shared stretch
    b[50_000:58_000] = b[30_000:38_000]         # a repeat inside one sequence
    for s, spots in ((a, ((100, 1), (149, 3), (12_345, 30), (30_000, 200))), (b, ((0, 2), (125, 2), (60_000, 500), (69_990, 11)))):
        for at, n in spots:
            s[at:at + n] = ord("N")
    return [a.tobytes(), b.tobytes(), b"ACN"]


def _count(ctx, seqs, k):
    """(payload sha256, histogram sha256, kernels seen) of one count of `seqs` as ONE block."""
    blk = ctx.upload(capi.PackedReads.from_reads(seqs))
    ctx.prof(True)
    ctx.prof_reset()
    t = capi.CountTable(ctx, k, SIZE)
    try:
        t.add(blk)
        rec, h = t.finish(want_histo=True)
        names = sorted(ctx.prof_dict())
        out = (hashlib.sha256(rec.payload()).hexdigest(), hashlib.sha256(h.tobytes()).hexdigest(), names)
        rec.free()
    finally:
        t.free()
        blk.free()
        ctx.prof(False)
    return out


def _child_main():
    seqs = _long_seqs()
    out = {}
    with capi.Context(0) as c:
        for k in COUNT_KS:
            out[str(k)] = _count(c, seqs, k)
    print("TILE_CHILD " + json.dumps(out))


@pytest.fixture(scope="module")
def long_seqs():
    return _long_seqs()


@pytest.fixture(scope="module")
def oracle_counts(long_seqs):
    return {k: oracle.count(None, k, SIZE, reads=long_seqs) for k in COUNT_KS}


@pytest.fixture(scope="module")
def untiled_child():
    """The same counts with RFX_NO_TILE=1, in a process of its own (the knob is read at every add; a child keeps this
    process's environment out of it)."""
    env = dict(os.environ, RFX_NO_TILE="1")
    p = subprocess.run([sys.executable, "-m", "tests.test_tile_gpu"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    line, = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("TILE_CHILD ")]
    return json.loads(line[len("TILE_CHILD "):])


@pytest.mark.parametrize("k", COUNT_KS)
def test_counts_of_long_sequences_are_unchanged(ctx, long_seqs, oracle_counts, untiled_child, k):
    ref = oracle_counts[k]
    want = (hashlib.sha256(ref.payload()).hexdigest(),
            hashlib.sha256(oracle.histo(ref.counts, full=True)[0].tobytes()).hexdigest())
    assert len(ref.keys) > 60_000 and int(ref.counts.max()) > 1
    payload, histo, names = _count(ctx, long_seqs, k)
    assert (payload, histo) == want
    assert "k_reads_tile" in names                                   # (c) the door is used ...
    c_payload, c_histo, c_names = untiled_child[str(k)]
    assert (c_payload, c_histo) == want
    assert "k_reads_tile" not in c_names and len(c_names) > 0        # ... and RFX_NO_TILE=1 keeps it shut


@pytest.mark.parametrize("k", [25, 31])
def test_shard_passes_of_long_sequences_replay_run_maps(ctx, long_seqs, oracle_counts, k, monkeypatch):
    """Two minimizer shards over one store of run maps: the second pass cuts its records from the tiled twin + its map
    (k_msp_replay) instead of hashing -- untiled, a block of long sequences is refused a map.  (Run maps are for blocks
    whose bins are fine enough, 2^29 windows or more than 8192 bins: RFX_P2L_BINS gives this small block 16384.)"""
    from rufus_amd import dist as rdist
    monkeypatch.setenv("RFX_P2L_BINS", "16384")
    ref = oracle_counts[k]
    blk = ctx.upload(capi.PackedReads.from_reads(long_seqs))
    store = capi.RunMaps(ctx)
    shards, hsum, replayed = [], np.zeros(capi.HISTO_BINS, dtype=np.uint64), []
    try:
        for sh in range(2):
            t = capi.CountTable(ctx, k, SIZE, mode=capi.COUNT_MSP)
            t.set_shard(sh, 2)
            t.set_runmaps(store)
            t.prepare_maps([blk])
            assert store.blocks() == 1               # the twin's map, asked for with the source
            t.add(blk)
            rec, h = t.finish(want_histo=True)
            shards.append(tuple(x.astype(np.uint64) for x in rec.get()))
            hsum += h
            replayed.append(t.replayed())
            rec.free()
            t.free()
        assert replayed[1] > 0
        store.drop(blk)
        assert store.blocks() == 0
    finally:
        store.free()
        blk.free()
    keys, counts, pos = rdist.merge_shards(shards)
    assert np.array_equal(keys, ref.keys) and np.array_equal(counts, ref.counts) and np.array_equal(pos, ref.pos)
    assert np.array_equal(hsum, oracle.histo(ref.counts, full=True)[0])


# ---------------------------------------------------------------------------------------------------
# (d) lifetime of the twin
# ---------------------------------------------------------------------------------------------------
def test_the_twin_lives_and_dies_with_its_source_block(ctx, long_seqs, oracle_counts):
    ctx.sync()
    used0 = ctx.mem_stats()["used"]
    # add, free the source, then finish: the free settles what the table still needs of the twin
    blk = ctx.upload(capi.PackedReads.from_reads(long_seqs))
    t = capi.CountTable(ctx, 25, SIZE)
    t.add(blk)
    blk.free()
    rec = t.finish()
    assert rec.payload() == oracle_counts[25].payload()
    rec.free()
    t.free()
    ctx.sync()
    assert ctx.mem_stats()["used"] == used0
    # a second table with another k on the same block: its twin replaces the first one's
    blk = ctx.upload(capi.PackedReads.from_reads(long_seqs))
    t25, t31 = capi.CountTable(ctx, 25, SIZE), capi.CountTable(ctx, 31, SIZE)
    t25.add(blk)
    t31.add(blk)
    r25, r31 = t25.finish(), t31.finish()
    assert r25.payload() == oracle_counts[25].payload()
    assert r31.payload() == oracle_counts[31].payload()
    for x in (r25, r31, t25, t31, blk):
        x.free()
    ctx.sync()
    assert ctx.mem_stats()["used"] == used0


# ---------------------------------------------------------------------------------------------------
# (e) through the executable
# ---------------------------------------------------------------------------------------------------
def test_jellyfish_count_of_a_multi_line_fasta(ctx, tmp_path):
    rng = np.random.default_rng(5)
    a, b = _random_seq(rng, 120_000, CLEAN), _random_seq(rng, 80_000, CLEAN)
    a[100_000:120_000] = a[:20_000]
    b[20_000:50_000] = a[40_000:70_000]
    b[70_000:70_300] = ord("N")
    fa = b""
    for name, s in ((b"chrA", a.tobytes().replace(b"\r", b"N")), (b"chrB some text", b.tobytes().replace(b"\r", b"N"))):
        fa += b">" + name + b"\n" + b"".join(s[i:i + 70] + b"\n" for i in range(0, len(s), 70))
    d = str(tmp_path)
    open(f"{d}/ref.fa", "wb").write(fa)
    jf = tools.jellyfish_count(ctx, [fa], 25, 100_000_000, lower=2)
    want = hashlib.sha256(jf.records.payload()).hexdigest()
    assert len(jf.records) > 40_000          # (the repeats: -L 2 leaves something to compare)
    jf.records.free()
    got = {}
    for name, extra in (("tiled", {}), ("untiled", {"RFX_NO_TILE": "1"}), ("passes", {"RFX_COUNT_DEFER": "1", "RFX_COUNT_PASSES": "2"})):
        p = subprocess.run([f"{BIN}/jellyfish", "count", "-m", "25", "-C", "-s", "100M", "-L", "2", "-o", f"{name}.jf", "ref.fa"],
                           cwd=d, env=dict(os.environ, RFX_CLI_TRACE="1", **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        blob = open(f"{d}/{name}.jf", "rb").read()
        got[name] = hashlib.sha256(blob[9 + int(blob[:9]):]).hexdigest()
        assert (b"through the tiler" in p.stderr) == (name != "untiled"), p.stderr.decode()[-2000:]
    assert got == {"tiled": want, "untiled": want, "passes": want}


if __name__ == "__main__":
    _child_main()
