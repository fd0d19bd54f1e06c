"""k_msp_leaf's three variants -- compiled for k = 25 and k = 31 with one segment, and the one that takes k, the segment
tables and the recount knob as arguments -- against the oracle, byte for byte (payload, histogram, checksum), at the
shapes where the kernel's paths part; capi.leaf_variant says which of them a count launched."""
import functools

import numpy as np
import pytest

import oracle
from rufus_amd import capi
from tests import run_map_ref as ref
from tests.binned_ref import _planted_targets, mmer_len, window_of

pytestmark = pytest.mark.gpu

SIZE = 1 << 34      # (a table size every k of the file takes: 2k - 30 <= 34 < min(2k, 40))
FULL = 2**64 - 1
LETTERS = np.frombuffer(b"ACGT", np.uint8)


@functools.lru_cache(maxsize=None)
def _reads():
    """4000 reads of <= 151 bases over 40 kb of random genome, a tenth with an N, a third reversed, a few homopolymers;
    depth ~14, so lower = 2 cuts and the record cache sees copies."""
    rng = np.random.default_rng(20251)
    genome = LETTERS[rng.integers(0, 4, 40_000)]
    seqs = []
    for _ in range(4000):
        n = int(rng.choice([0, 10, 24, 25, 26, 31, 60, 100, 150, 151, 151, 151]))
        s0 = int(rng.integers(0, len(genome) - n))
        r = genome[s0:s0 + n].copy()
        if rng.random() < 0.1 and len(r):
            r[rng.integers(0, len(r))] = ord("N")
        if rng.random() < 0.02:
            r[:] = ord("ACGT"[int(rng.integers(0, 4))])
        if rng.random() < 0.3:
            r = r[::-1].copy()
        seqs.append(bytes(r))
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def _expected(which, k, canonical, lower=2, upper=FULL):
    """(payload, histogram, checksum) of the oracle's count: computed once per case, shared, never changed."""
    seqs = {"reads": _reads, "edges25": lambda: _edge_reads(25), "edges31": lambda: _edge_reads(31), "dense": _dense_reads,
            "repeated": _repeated_reads}[which]()
    r = oracle.count(None, k, SIZE, lower=lower, upper=upper, canonical=canonical, reads=list(seqs))
    return r.payload(), oracle.histo(r.counts, full=True)[0], r.checksum()


def _count(ctx, seqs, k, canonical, lower=2, upper=FULL, blocks=1):
    """(payload, histogram, checksum, leaf_variant) of the MSP count of `seqs`, added as `blocks` read blocks."""
    t = capi.CountTable(ctx, k, SIZE, canonical, mode=capi.COUNT_MSP)
    cuts = [len(seqs) * i // blocks for i in range(blocks + 1)]
    for a, b in zip(cuts, cuts[1:]):
        blk = ctx.upload(capi.PackedReads.from_reads(list(seqs[a:b])))
        t.add(blk)
        blk.free()
    rec, h = t.finish(lower, upper, want_histo=True)
    out = (rec.payload(), np.array(h), rec.checksum(), capi.leaf_variant(ctx))
    rec.free()
    t.free()
    return out


def _same(got, want, what):
    assert got[0] == want[0], f"{what}: payload differs"
    assert np.array_equal(got[1], want[1]), f"{what}: histogram differs"
    assert got[2] == want[2], f"{what}: checksum differs"


def _took(v, kc):
    assert v == {"kc": kc, "one": kc > 0}, f"the launch took {v}, meant: kc = {kc}"


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [24, 25, 26, 31])
def test_k_and_orientation(ctx, k, canonical):
    """25 and 31 take the kernels compiled for them; 24 and 26, beside them on the same reads, the generic one."""
    got = _count(ctx, _reads(), k, canonical)
    _took(got[3], k if k in (25, 31) else 0)
    _same(got, _expected("reads", k, canonical), (k, canonical))


@pytest.mark.parametrize("k", [25, 31])
def test_forced_generic_gives_the_same_bytes(ctx, monkeypatch, k):
    """RFX_LEAF_GENERIC=1: the same reads through the generic kernel; its bytes equal the specialised run's."""
    spec = _count(ctx, _reads(), k, True)
    _took(spec[3], k)
    monkeypatch.setenv("RFX_LEAF_GENERIC", "1")
    gen = _count(ctx, _reads(), k, True)
    _took(gen[3], 0)
    _same(gen, spec, ("generic against specialised", k))
    _same(spec, _expected("reads", k, True), ("specialised", k))


@pytest.mark.parametrize("geo", ["0", "1"])
@pytest.mark.parametrize("k", [25, 31])
def test_both_leaf_geometries(ctx, monkeypatch, k, geo):
    """RFX_MSP_GEO=0: one 1024-thread workgroup per CU; 1: two of 768."""
    monkeypatch.setenv("RFX_MSP_GEO", geo)
    got = _count(ctx, _reads(), k, True)
    _took(got[3], k)
    _same(got, _expected("reads", k, True), (k, "geo", geo))


def test_several_segments_take_the_generic_kernel(ctx, monkeypatch):
    """Three read blocks, a launch per segment (RFX_PART3_PER_SEG=1): the leaf reads three segments, which only the
    generic kernel can."""
    monkeypatch.setenv("RFX_PART3_PER_SEG", "1")
    got = _count(ctx, _reads(), 25, True, blocks=3)
    _took(got[3], 0)
    _same(got, _expected("reads", 25, True), "three segments")


def test_forced_recount_takes_the_generic_kernel(ctx, monkeypatch):
    """RFX_LEAF_FORCE_MIXED=1: every third bin is counted again without the record cache -- a route the specialised
    kernels do not carry."""
    monkeypatch.setenv("RFX_LEAF_FORCE_MIXED", "1")
    got = _count(ctx, _reads(), 25, True)
    _took(got[3], 0)
    _same(got, _expected("reads", 25, True), "forced recount")


# ---- runs at the record's edges ---------------------------------------------------------------------------------------------
# A read of L bases that holds a planted m-mer (the smallest hashes there are: the minimizer of every k-mer that contains it)
# at offset o, with L - k <= o <= k - m, is ONE super-k-mer of L bases: every one of its L - k + 1 k-mers contains the m-mer.

def _planted_read(rng, k, L, o, which=0):
    m = mmer_len(k)
    t = int(_planted_targets(k, 4096)[which])
    r = LETTERS[rng.integers(0, 4, L)]
    r[o:o + m] = LETTERS[[(t >> (2 * (m - 1 - j))) & 3 for j in range(m)]]
    return r


def _edge_shapes(k):
    """(L, o) of the planted reads: a single k-mer, 28 and 29 bases (the word / plane boundary), the longest run -- and at
    k = 31 minimizers that end inside the first 28 bases (side 0) and beyond them (side 1)."""
    m, cap = mmer_len(k), ref.run_cap(k)
    lens = sorted({k, max(k, 28), max(k, 29), k + 1, k + cap - 2, k + cap - 1})
    out = []
    for L in lens:
        lo, hi = L - k, k - m
        out += [(L, o) for o in sorted({lo, (lo + hi) // 2, hi, min(max(lo, 28 - m), hi), min(max(lo, 29 - m), hi)})]
    return out


@functools.lru_cache(maxsize=None)
def _edge_reads(k):
    rng = np.random.default_rng(77 + k)
    out = []
    for L, o in _edge_shapes(k):
        for rep in range(6):
            r = _planted_read(rng, k, L, o, which=rep % 3)
            out += [bytes(r)] * (1 + rep % 3)                  # copies: the record cache's multiplicity
            if rep == 5:
                out.append(bytes(r[::-1].copy()))
    out += list(_reads()[:600])
    return tuple(out)


def _runs_of(seqs, k, canonical):
    """(run length in bases, side) of every super-k-mer of the reads, by tests/run_map_ref.py's brute-force minimizer."""
    width = max(len(s) for s in seqs)
    codes, valid = np.zeros((len(seqs), width), np.uint8), np.zeros((len(seqs), width), bool)
    lut = np.full(256, 4, np.uint8)
    lut[LETTERS] = np.arange(4, dtype=np.uint8)
    for i, s in enumerate(seqs):
        c = lut[np.frombuffer(s, np.uint8)]
        valid[i, :len(s)] = c < 4
        codes[i, :len(s)] = c & 3
    m, seen = mmer_len(k), set()
    for runs in ref.read_runs(codes, valid, k, canonical):
        for rs, e, minh in runs:
            L = e - rs + k
            first = rs - (k - 1)                              # the run's first base
            end = rs - ((rs - (int(minh) & 31)) & 31)         # the minimizer m-mer ends inside the run's first k-mer
            mpos = end - (m - 1) - first
            assert 0 <= mpos <= k - m
            seen.add((L, int(k >= 29 and L > 28 and mpos + m > 28)))
    return seen


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [25, 31])
def test_run_lengths_at_the_records_edges(ctx, k, canonical):
    seqs = _edge_reads(k)
    seen = _runs_of(seqs, k, canonical)
    longest = k + ref.run_cap(k) - 1
    assert longest == (35 if k == 25 else 43) and window_of(k) >= ref.run_cap(k)
    if k == 25:
        need = {(25, 0), (28, 0), (29, 0), (35, 0)}
    else:
        need = {(31, 0), (31, 1), (32, 0), (32, 1), (42, 0), (42, 1), (43, 0), (43, 1)}
    assert need <= seen, f"the input lacks runs of (bases, side) {sorted(need - seen)}"
    got = _count(ctx, seqs, k, canonical, lower=1)
    _took(got[3], k)
    _same(got, _expected(f"edges{k}", k, canonical, 1), ("edges", k, canonical))


# ---- a bin that must split ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dense_reads():
    """900 reads of 35 random bases around ONE planted 15-mer (k = 25): 9900 k-mers with the same minimizer, so in the same
    fine bin whatever the bin count -- more distinct keys than a pass of either geometry takes (3072 / 6144)."""
    rng = np.random.default_rng(4242)
    out = [bytes(_planted_read(rng, 25, 35, 10)) for _ in range(900)]
    return tuple(out + list(_reads()[:300]))


@pytest.mark.parametrize("geo", ["0", "1"])
def test_a_bin_that_must_split(ctx, monkeypatch, geo):
    seqs = _dense_reads()
    planted = set()
    t = int(_planted_targets(25, 4096)[0])
    text = bytes(LETTERS[[(t >> (2 * (14 - j))) & 3 for j in range(15)]])
    for s in seqs[:900]:
        assert s[10:25] == text
        planted |= {min(s[q:q + 25], s[q:q + 25][::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))) for q in range(11)}
    assert _runs_of(seqs[:900], 25, True) == {(35, 0)}, "a planted read is not one run under one minimizer"
    assert len(planted) > 6144
    monkeypatch.setenv("RFX_MSP_GEO", geo)
    got = _count(ctx, seqs, 25, True, lower=1)
    _took(got[3], 25)
    _same(got, _expected("dense", 25, True, 1), ("dense bin", geo))


# ---- bounds ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _repeated_reads():
    """The first 1500 reads once, the first 300 of them 45 times more: counts on both sides of upper = 40."""
    base = _reads()
    return tuple(list(base[:1500]) + list(base[:300]) * 45)


@pytest.mark.parametrize("k", [25, 31])
def test_every_key_survives_and_the_upper_bound_cuts(ctx, k):
    want_all, want_cut = _expected("repeated", k, True, 1, FULL), _expected("repeated", k, True, 1, 40)
    assert len(want_cut[0]) < len(want_all[0]), "upper = 40 cuts nothing on this input"
    for upper, want in ((FULL, want_all), (40, want_cut)):
        got = _count(ctx, _repeated_reads(), k, True, lower=1, upper=upper)
        _took(got[3], k)
        _same(got, want, ("bounds", k, upper))
