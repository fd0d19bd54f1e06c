"""k_strike_wave (rufus_amd/csrc/rfx_msp.hip): the wave-per-unit strike that takes the plain units, and its hand-over of the
others to k_strike_bins -- through rfx_binned_strike on stores built from hand-made reads, exactly against a set difference
computed on the host (tests/binned_ref.py).  Every case runs on both routes (the default, and RFX_STRIKE_WG=1: every unit
through k_strike_bins) against the same expected lists, and asserts from rfx_binned_strike_stats that it took the route it
is there for: `deferred` is the number of units k_strike_wave left to k_strike_bins (all of them under RFX_STRIKE_WG=1).

A unit is plain -- k_strike_wave's -- when it has at most cap_c control and cap_s subject survivors and either side lies
in at most two stretches of its pool (one bin crossing a chunk boundary, or two bins of the finer side)."""
import functools

import numpy as np
import pytest

from rufus_amd import capi
from tests import binned_ref as ref
from tests.binned_ref import np_bin
from tests.test_strike_gpu import (BITS_OF_DELTA, NATURAL_BITS, U32, check_planted_bin, check_store, planted_minimizers,
                                   planted_samples, ref_store, rig, shuffled, trio_samples)  # noqa: F401  (rig: a fixture)

pytestmark = pytest.mark.gpu

K = 25
SW_SET, SW_PER = 1024, 12                                # rfx_msp.hip
CAP_C, CAP_S = min(3 * SW_SET // 4, 64 * SW_PER), 64 * SW_PER  # SW_CAP_C, SW_CAP_S: 768, 768
SW_SEGS = 2


@pytest.fixture(params=["wave", "wg"])
def route(request, monkeypatch):
    if request.param == "wg":
        monkeypatch.setenv("RFX_STRIKE_WG", "1")
    else:
        monkeypatch.delenv("RFX_STRIKE_WG", raising=False)
    return request.param


def check_route(ctx, route, want_deferred):
    """want_deferred: the exact number of units k_strike_wave must have left to k_strike_bins, or a predicate on
    (units, deferred)."""
    st = capi.binned_strike_stats(ctx)
    assert st["units"] > 0
    if route == "wg":
        assert st["deferred"] == st["units"], "RFX_STRIKE_WG=1 did not send every unit through k_strike_bins"
    elif callable(want_deferred):
        assert want_deferred(st["units"], st["deferred"]), f"route taken: {st}"
    else:
        assert st["deferred"] == want_deferred, f"route taken: {st}, the case asks for {want_deferred} deferred"
    return st


def sb_hash(keys: np.ndarray) -> np.ndarray:
    """rfx_msp.hip sb_hash: (key * 0x9E3779B97F4A7C15) >> 40, as 32 bits."""
    with np.errstate(over="ignore"):
        return ((np.asarray(keys, np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)).astype(np.uint32)


def np_encode(reads) -> np.ndarray:
    """2-bit keys (A C G T = 0 1 2 3, first base highest) of reads of equal length <= 32."""
    a = np.frombuffer(b"".join(reads), np.uint8).reshape(len(reads), -1)
    code = np.zeros(256, np.uint64)
    code[list(b"ACGT")] = [0, 1, 2, 3]
    key = np.zeros(len(reads), np.uint64)
    for col in a.T:
        key = (key << np.uint64(2)) | code[col]
    return key


def unit_sizes(store_ref, k, bits):
    """{unit: number of survivors} at `bits` bits."""
    u, n = np.unique(np_bin(store_ref[0], k, bits), return_counts=True)
    return dict(zip(u.tolist(), n.tolist()))


def not_plain_by_size(s_ref, c_ref, k, ubits, cap_c, cap_s):
    """Units (bins at ubits) that hold subject survivors and more of either side than the wave kernel is given room for."""
    ns, nc = unit_sizes(s_ref, k, ubits), unit_sizes(c_ref, k, ubits) if c_ref is not None else {}
    return sorted(u for u, n in ns.items() if n > cap_s or nc.get(u, 0) > cap_c)


def stretches(store, k, ubits):
    """{unit: stretches the walk of the unit passes}, from rfx_binned_get's flat indices: a stretch is a run of consecutive
    pool entries of ONE bin of the store (a bin that crosses a chunk boundary is two; two bins of a unit are two even
    where they touch)."""
    keys, _, bins, at = store.get()
    if not len(keys):
        return {}
    o = np.lexsort((at, bins))
    b, a = bins[o].astype(np.int64), at[o].astype(np.int64)
    first = np.ones(len(b), bool)
    first[1:] = (b[1:] != b[:-1]) | (a[1:] != a[:-1] + 1)
    u, n = np.unique(b[first] >> (store.bits - ubits), return_counts=True)
    return dict(zip(u.tolist(), n.tolist()))


def not_plain(S, C, s_ref, c_ref, k, ubits, cap_c=CAP_C, cap_s=CAP_S):
    """The units k_strike_wave must defer: those with subject survivors and a side beyond its capacity or in more than
    SW_SEGS stretches."""
    ss, cs = stretches(S, k, ubits), stretches(C, k, ubits) if C is not None else {}
    many = {u for u, n in ss.items() if n > SW_SEGS or cs.get(u, 0) > SW_SEGS}
    return sorted(many | set(not_plain_by_size(s_ref, c_ref, k, ubits, cap_c, cap_s)))


# ---- a. at the capacity edge -------------------------------------------------------------------------------------------
EDGE_CASES = [(None, CAP_S, CAP_C, 0), (None, CAP_S, CAP_C + 1, 1), (None, CAP_S + 1, CAP_C, 1), (None, CAP_S - 1, CAP_C - 1, 0),
              ((8, 8), 8, 8, 0), ((8, 8), 8, 9, 1), ((8, 8), 9, 8, 1), ((8, 16), 16, 8, 0), ((8, 16), 17, 8, 1)]


@pytest.mark.parametrize("caps,n_s,n_c,deferred", EDGE_CASES)
def test_capacity_edge(rig, route, monkeypatch, caps, n_s, n_c, deferred):
    """One planted unit with exactly the capacity on a side (the wave kernel takes it) and one more (deferred): at the
    compiled capacities and at capacities lowered by RFX_STRIKE_WAVE_CAP."""
    lower, lo, hi = 1, 1, 1
    if caps:
        monkeypatch.setenv("RFX_STRIKE_WAVE_CAP", "%d,%d" % caps)
    s_reads, c_reads = planted_samples(K, n_s, n_c)
    s_ref, c_ref = ref_store(s_reads, K, lower), ref_store(c_reads, K, lower)
    check_planted_bin(s_ref, K, NATURAL_BITS, n_s)
    check_planted_bin(c_ref, K, NATURAL_BITS, n_c)
    S, s_histo = rig.store(s_reads, K, lower)
    C, c_histo = rig.store(c_reads, K, lower)
    check_store(S, s_histo, s_ref, K, lower)
    check_store(C, c_histo, c_ref, K, lower)
    assert S.bits == C.bits == NATURAL_BITS
    cap_c, cap_s = (min(caps[0], CAP_C), min(caps[1], CAP_S)) if caps else (CAP_C, CAP_S)
    assert len(not_plain(S, C, s_ref, c_ref, K, NATURAL_BITS, cap_c, cap_s)) == deferred
    wk, wc = rig.strike(S, [C], s_ref, [c_ref], lo, hi)
    check_route(rig.ctx, route, deferred)  # (units: the bins between the store's first and last, here the planted one)
    assert 0 < len(wk) < n_s and (wc == 1).all()


@functools.lru_cache(maxsize=None)
def mixed_samples():
    """Random reads over all the bins and a planted unit beyond the compiled capacities on the control's side."""
    rr = ref.random_reads(500, 150, 31337)
    planted_s, planted_c = planted_samples(K, 600, CAP_C + 200)
    return shuffled(rr[:300] + planted_s, 5), shuffled(rr[150:450] + planted_c, 6), shuffled(rr[100:200] + rr[450:500], 7)


@pytest.mark.parametrize("caps", [None, (150, 150), (140, 1000), (1000, 140)])
def test_some_units_deferred(rig, route, monkeypatch, caps):
    """A store of which some units are plain and some are not: the list is the union of what the two kernels find, and the
    number deferred is the number of units beyond a capacity, counted on the host."""
    lower, lo, hi = 1, 1, 2
    if caps:
        monkeypatch.setenv("RFX_STRIKE_WAVE_CAP", "%d,%d" % caps)
    cap_c, cap_s = (min(caps[0], CAP_C), min(caps[1], CAP_S)) if caps else (CAP_C, CAP_S)
    reads = mixed_samples()
    refs = [ref_store(r, K, lower) for r in reads]
    S, s_histo = rig.store(reads[0], K, lower)
    C1, c1_histo = rig.store(reads[1], K, lower)
    C2, _ = rig.store(reads[2], K, lower)
    check_store(S, s_histo, refs[0], K, lower)
    check_store(C1, c1_histo, refs[1], K, lower)
    big = not_plain(S, C1, refs[0], refs[1], K, NATURAL_BITS, cap_c, cap_s)
    n_units = len(unit_sizes(refs[0], K, NATURAL_BITS))
    assert 0 < len(big) < n_units, "the case wants units on both routes"
    wk, _ = rig.strike(S, [C1, C2], refs[0], refs[1:], lo, hi)
    check_route(rig.ctx, route, len(big))
    assert len(wk) > 0
    on_big = np.isin(np_bin(wk, K, NATURAL_BITS), np.array(big, np.uint32))
    assert on_big.any() and not on_big.all(), "the list does not come from both kernels"


# ---- b. set probing ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def colliding_samples():
    """Control: planted k-mers of one bin whose sb_hash lands in the set's last four slots -- many more than four, so the
    probe wraps past the last slot.  Subject: half of them, the near-misses (same slots, not in the control) and others."""
    pool = ref.kmers_in_one_bin(K, 21000, 77)
    keys = np_encode(pool)
    h = sb_hash(keys) & np.uint32(SW_SET - 1)
    tail = np.flatnonzero(h >= SW_SET - 4)
    assert len(tail) >= 40
    ctl, miss = tail[:len(tail) * 2 // 3], tail[len(tail) * 2 // 3:]
    other = np.flatnonzero(h < SW_SET - 4)[:200]
    control = [pool[i] for i in ctl] + [pool[i] for i in other[:100]]
    subject = [pool[i] for i in ctl[::2]] + [pool[i] for i in miss] + [pool[i] for i in other[50:200]]
    return shuffled(subject, 11), shuffled(control, 12), len(ctl), len(miss)


def test_set_probing(rig, route):
    lower, lo, hi = 1, 1, U32
    s_reads, c_reads, n_ctl, n_miss = colliding_samples()
    s_ref, c_ref = ref_store(s_reads, K, lower), ref_store(c_reads, K, lower)
    hc = sb_hash(c_ref[0]) & np.uint32(SW_SET - 1)
    assert int((hc >= SW_SET - 4).sum()) == n_ctl > 8, "the control's keys do not wrap past the last slot"
    hs = sb_hash(s_ref[0]) & np.uint32(SW_SET - 1)
    near = (hs >= SW_SET - 4) & ~np.isin(s_ref[0], c_ref[0])
    assert int(near.sum()) == n_miss > 4 and int(((hs >= SW_SET - 4) & np.isin(s_ref[0], c_ref[0])).sum()) > 4
    S, s_histo = rig.store(s_reads, K, lower)
    C, c_histo = rig.store(c_reads, K, lower)
    check_store(S, s_histo, s_ref, K, lower)
    check_store(C, c_histo, c_ref, K, lower)
    wk, _ = rig.strike(S, [C], s_ref, [c_ref], lo, hi)
    check_route(rig.ctx, route, 0)
    assert np.isin(s_ref[0][near], wk).all() and len(wk) == int((~np.isin(s_ref[0], c_ref[0])).sum())


# ---- c. the lane clear -------------------------------------------------------------------------------------------------
def test_lane_clear(rig, route, monkeypatch):
    """A wave takes unit after unit with one set, and its lanes empty only the slots they filled.  A k-mer has one bin in
    every sample, so a key left behind by an earlier unit can never equal a key of a later one: what a missing clear does is
    fill the set up.  One workgroup (RFX_STRIKE_WAVE_GRID=1) takes all 256 units here, 64 to a wave, ~150 control keys
    each -- nine times the set -- and the list must still be exact: a control key that found no room would let its k-mer
    through."""
    lower, lo, hi = 1, 1, 3
    monkeypatch.setenv("RFX_STRIKE_WAVE_GRID", "1")
    reads = trio_samples(K)
    refs = [ref_store(r, K, lower) for r in reads]
    sizes = unit_sizes(refs[1], K, NATURAL_BITS)
    assert len(sizes) == 1 << NATURAL_BITS and min(sizes.values()) > 50
    assert sum(sorted(sizes.values())[:64]) > 4 * SW_SET, "a wave's units do not overfill a set that is never emptied"
    S, s_histo = rig.store(reads[0], K, lower)
    C1, c1_histo = rig.store(reads[1], K, lower)
    C2, _ = rig.store(reads[2], K, lower)
    check_store(S, s_histo, refs[0], K, lower)
    check_store(C1, c1_histo, refs[1], K, lower)
    wk, _ = rig.strike(S, [C1, C2], refs[0], refs[1:], lo, hi)
    check_route(rig.ctx, route, lambda units, deferred: 4 * 16 < units <= 1 << NATURAL_BITS and deferred == 0)
    assert len(wk) > 0


# ---- d. segments -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,n_s,n_c", [("subject", 10000, 700), ("control", 700, 5000), ("both", 10000, 5000)])
def test_segments(rig, route, side, n_s, n_c):
    """A bin whose survivors cross staging-chunk boundaries (4352 entries to a chunk of a small input's pool) on the
    subject's side, on the control's and on both.  The leaf splits a bin only between its passes, so a bin that crosses is
    far beyond the wave kernel's capacities: it is deferred, and k_strike_bins walks its stretches.  (Two stretches within the
    capacities are what a unit of two fine bins is: test_unequal_depth.)"""
    lower, lo, hi = 1, 1, 1
    s_reads, c_reads = planted_samples(K, n_s, n_c)
    s_ref, c_ref = ref_store(s_reads, K, lower), ref_store(c_reads, K, lower)
    check_planted_bin(s_ref, K, NATURAL_BITS, n_s)
    check_planted_bin(c_ref, K, NATURAL_BITS, n_c)
    S, s_histo = rig.store(s_reads, K, lower)
    C, c_histo = rig.store(c_reads, K, lower)
    check_store(S, s_histo, s_ref, K, lower)
    check_store(C, c_histo, c_ref, K, lower)
    ss, cs = max(stretches(S, K, NATURAL_BITS).values()), max(stretches(C, K, NATURAL_BITS).values())
    assert (ss > 1) == (side != "control") and (cs > 1) == (side != "subject"), f"stretches: subject {ss}, control {cs}"
    wk, _ = rig.strike(S, [C], s_ref, [c_ref], lo, hi)
    check_route(rig.ctx, route, 1)
    assert 0 < len(wk) < n_s


# ---- e. unequal depth --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_bits,c_bits", [(13, 12), (12, 13), (13, 9), (13, 17)])
def test_unequal_depth(rig, route, s_bits, c_bits):
    """The subject finer than the control and coarser.  One bit apart a unit is two bins of the finer side: two stretches,
    the wave kernel's (but for the units that also cross a chunk boundary); four bits apart it is sixteen, and every unit
    with more than two of them filled goes to k_strike_bins.  Some units' fine bins are partly empty."""
    lower, lo, hi = 1, 1, 3
    reads = trio_samples(K)
    refs = [ref_store(r, K, lower) for r in reads]
    S, s_histo = rig.store(reads[0], K, lower, bits=s_bits)
    C1, c1_histo = rig.store(reads[1], K, lower, bits=c_bits)
    C2, _ = rig.store(reads[2], K, lower, bits=c_bits)
    check_store(S, s_histo, refs[0], K, lower)
    check_store(C1, c1_histo, refs[1], K, lower)
    ubits, fbits = min(s_bits, c_bits), max(s_bits, c_bits)
    fine_ref = refs[0] if s_bits > c_bits else refs[1]
    fine_bins = np.unique(np_bin(fine_ref[0], K, fbits))
    per_unit = np.unique(fine_bins >> np.uint32(fbits - ubits), return_counts=True)[1]
    assert (per_unit < (1 << (fbits - ubits))).any() and (per_unit > 1).any(), "no unit's fine bins are partly empty"
    ss, cs = stretches(S, K, ubits), stretches(C1, K, ubits)
    many = not_plain(S, C1, refs[0], refs[1], K, ubits)
    assert not not_plain_by_size(refs[0], refs[1], K, ubits, CAP_C, CAP_S)
    wk, _ = rig.strike(S, [C1, C2], refs[0], refs[1:], lo, hi)
    st = check_route(rig.ctx, route, len(many))
    assert len(ss) <= st["units"] <= 1 << ubits
    if route == "wave":
        if abs(s_bits - c_bits) == 1:
            assert st["deferred"] < len(ss) // 4, "one bit apart nearly every unit is the wave kernel's"
        else:
            assert st["deferred"] > 0
    assert len(wk) > 0


# ---- f. degenerate -----------------------------------------------------------------------------------------------------
def test_no_control_and_empty_control(rig, route):
    lower, lo, hi = 1, 1, 3
    s_reads = trio_samples(K)[0]
    s_ref = ref_store(s_reads, K, lower)
    short = tuple(r[:K - 1] for r in s_reads[:50])  # reads, but no k-mer: a store without survivors
    e_ref = ref_store(short, K, lower)
    in_range = int(((s_ref[1] >= lo) & (s_ref[1] <= hi)).sum())
    assert 0 < in_range < len(s_ref[0]) and len(e_ref[0]) == 0
    S, _ = rig.store(s_reads, K, lower)
    wk, _ = rig.strike(S, [], s_ref, [], lo, hi)  # the range alone
    check_route(rig.ctx, route, 0)
    assert len(wk) == in_range
    S, _ = rig.store(s_reads, K, lower)
    E, _ = rig.store(short, K, lower, empty=True)
    assert E.bits == 0 and len(E) == 0
    wk, _ = rig.strike(S, [E], s_ref, [e_ref], lo, hi)
    check_route(rig.ctx, route, 0)
    assert len(wk) == in_range


def test_empty_bins_opposite_full_ones(rig, route):
    """The subject's only bin is empty in the control and the control's only bin is empty in the subject."""
    lower, lo, hi = 1, 1, U32
    m0 = ref.planted_minimizer(K)
    m1 = next(int(m) for m in ref._planted_targets(K, 4096)[1:] if ref.mmer_bin(int(m), NATURAL_BITS) != ref.mmer_bin(m0, NATURAL_BITS))
    s_reads, c_reads = ref.kmers_in_one_bin(K, 300, 21, m0), ref.kmers_in_one_bin(K, 300, 22, m1)
    assert ref.mmer_bin(m0, NATURAL_BITS) != ref.mmer_bin(m1, NATURAL_BITS)
    s_ref, c_ref = ref_store(s_reads, K, lower), ref_store(c_reads, K, lower)
    check_planted_bin(s_ref, K, NATURAL_BITS, 300)
    check_planted_bin(c_ref, K, NATURAL_BITS, 300)
    S, _ = rig.store(s_reads, K, lower)
    C, _ = rig.store(c_reads, K, lower)
    wk, _ = rig.strike(S, [C], s_ref, [c_ref], lo, hi)
    check_route(rig.ctx, route, 0)
    assert len(wk) == 300
    S, _ = rig.store(s_reads, K, lower)
    C, _ = rig.store(c_reads, K, lower)
    wk, _ = rig.strike(C, [S], c_ref, [s_ref], lo, hi)
    check_route(rig.ctx, route, 0)
    assert len(wk) == 300


@pytest.mark.parametrize("lo,hi,some", [(5, 7, False), (1, 1, True), (2, 2, True)])
def test_count_ranges(rig, route, lo, hi, some):
    """Every count of the subject outside [lo, hi] (nothing listed), and lo == hi."""
    lower = 1
    s_reads, c_reads = planted_samples(K, 400, 300)  # counts 1 and, every eighth, 2
    s_ref, c_ref = ref_store(s_reads, K, lower), ref_store(c_reads, K, lower)
    assert set(np.unique(s_ref[1]).tolist()) == {1, 2}
    S, _ = rig.store(s_reads, K, lower)
    C, _ = rig.store(c_reads, K, lower)
    wk, wc = rig.strike(S, [C], s_ref, [c_ref], lo, hi)
    check_route(rig.ctx, route, 0)
    assert (len(wk) > 0) == some and (wc == lo).all()


def test_shard_pass_store(rig, route):
    """Stores of the second of two shard passes: the units do not begin at 0."""
    lower, lo, hi = 1, 1, 3
    reads = trio_samples(K)
    refs = [ref_store(r, K, lower) for r in reads]
    S, C1, C2 = (rig.store(r, K, lower, shard=(1, 2))[0] for r in reads)
    keys, _, bins, _ = S.get()
    assert len(keys) and int(bins.min()) >= 1 << (NATURAL_BITS - 1), "the shard's bins begin at 0"
    own = np.isin(refs[0][0], keys)
    assert 0 < int(own.sum()) < len(own)
    wk, _ = rig.strike(S, [C1, C2], (refs[0][0][own], refs[0][1][own]), refs[1:], lo, hi)
    st = check_route(rig.ctx, route, 0)
    assert len(np.unique(bins)) <= st["units"] <= 1 << (NATURAL_BITS - 1) and len(wk) > 0
