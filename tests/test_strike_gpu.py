"""k_strike_bins and k_strike_cands (rufus_amd/csrc/rfx_msp.hip) through the C API -- rfx_count_finish_binned,
rfx_binned_strike, rfx_candidates_strike -- on stores of chosen shape, built from hand-made reads, against a set difference
computed on the host from the oracle's counts (tests/binned_ref.py).  Every comparison is exact, and every case asserts the
shape it is there for: the bit counts of both sides, the size of the planted bin, the spread over sub-bins, the length of
the candidate list."""
import functools

import numpy as np
import pytest

import oracle
from rufus_amd import capi
from tests import binned_ref as ref
from tests.binned_ref import by_key, np_bin

pytestmark = pytest.mark.gpu

U32, U64 = 0xFFFFFFFF, 2**64 - 1
NATURAL_BITS = 8          # what a small input is counted at: 256 bins per read block (rfx_api.hip msp_geometry), nothing to refine
CAND_CAP_FLOOR = 1 << 16  # rfx_api.hip rfx_binned_strike: cap = max(1 << 16, subject->n / 256)
HISTO_BINS = 10002        # counts 0 .. 10000, and 10001 for everything beyond


# ---- stores ----------------------------------------------------------------------------------------------------------
class Rig:
    """Builds stores and strikes them; frees what it made when the test is over."""

    def __init__(self, ctx, monkeypatch):
        self.ctx, self.monkeypatch, self.held = ctx, monkeypatch, []

    def store(self, reads, k, lower, upper=U64, bits=None, shard=None, empty=False):
        """reads -> PackedReads -> upload -> CountTable(COUNT_MSP) -> add -> finish_binned.  bits: RFX_MSP_REFINE_BITS around
        the finish (msp_prepare_leaf takes the larger of this and what the input asks for)."""
        blk = self.ctx.upload(capi.PackedReads.from_reads(list(reads)))
        t = capi.CountTable(self.ctx, k, ref.SIZE, True, mode=capi.COUNT_MSP)
        try:
            if shard is not None:
                t.set_shard(*shard)
            t.add(blk)
            if bits is not None:
                self.monkeypatch.setenv("RFX_MSP_REFINE_BITS", str(bits))
            try:
                b, histo = t.finish_binned(lower, upper, want_histo=True)
            finally:
                if bits is not None:
                    self.monkeypatch.delenv("RFX_MSP_REFINE_BITS")
            self.held.append(b)
        finally:
            t.free()
            blk.free()
        want_bits = 0 if empty else NATURAL_BITS if bits is None else bits
        assert b.bits == want_bits, f"the store has {b.bits} bits, the case asks for {want_bits}"
        return b, histo

    def strike(self, subject, controls, s_ref, c_refs, lo, hi):
        """binned_strike with the first control (or none), Candidates.strike with the others; the list after the first and
        after the last against the reference."""
        cand = capi.binned_strike(self.ctx, subject, controls[0] if controls else None, lo, hi)
        self.held.append(cand)
        fk, fc = ref.expected_candidates(s_ref, c_refs[:1], lo, hi)
        assert len(cand) == len(fk), "length of the list after the first control"
        gk, gc = by_key(*cand.keys_counts())
        assert np.array_equal(gk, fk) and np.array_equal(gc, fc), "candidates after the first control"
        for c in controls[1:]:
            cand.strike(c)
        assert len(cand) == len(fk), "a later control changed the list's length"
        wk, wc = ref.expected_candidates(s_ref, c_refs, lo, hi)
        gk, gc = by_key(*cand.keys_counts())
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc), "candidates after the last control"
        return wk, wc

    def close(self):
        for x in self.held:
            x.free()


@pytest.fixture
def rig(ctx, monkeypatch):
    b = Rig(ctx, monkeypatch)
    yield b
    b.close()


@functools.lru_cache(maxsize=None)
def ref_store(reads: tuple, k: int, lower: int, upper: int = U64):
    """The oracle's store of a sample: made once, shared, never changed."""
    keys, counts = ref.expected_store(reads, k, lower, upper)
    keys.setflags(write=False)
    counts.setflags(write=False)
    return keys, counts


def check_store(b, histo, want, k, lower, upper=U64):
    """get() against the oracle as a key-sorted multiset, the histogram, verify()."""
    wk, wc = by_key(*want)
    keys, counts, bins, _ = b.get()
    assert len(b) == len(keys) == len(wk)
    gk, gc = by_key(keys, counts)
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc), "the store is not the oracle's multiset"
    assert np.array_equal(histo, np.bincount(np.minimum(wc, np.uint64(10001)).astype(np.int64), minlength=HISTO_BINS))
    assert b.verify(lower, upper) == {"bad_bin": 0, "bad_count": 0, "not_canonical": 0, "duplicate": 0, "sum_counts": int(wc.sum())}
    if len(keys):
        assert np.array_equal(bins, np_bin(keys, k, b.bits)), "a survivor's bin is not the bin function of its key"


def shuffled(reads, seed):
    reads = list(reads)
    return tuple(reads[i] for i in np.random.default_rng(seed).permutation(len(reads)))


# ---- a. count edges ----------------------------------------------------------------------------------------------------
EDGE_K, EDGE_LOWER, EDGE_UPPER = 25, 2, 300
SUBJECT_COUNTS = (1, 2, 4, 5, 100, 101, 300, 301)
CONTROL_COUNTS = (0, 1, 2, 300, 301)  # absent; below the control's lower; its lower; its upper; beyond its upper
BIG_COUNTS = ((10001, 0), (10001, 2), (10002, 0), (65535, 2), (65536, 0), (65536, 301), (70000, 0), (70000, 1))


@functools.lru_cache(maxsize=None)
def edge_samples():
    """(subject reads, subject reads with the big counts, control reads, {k-mer text: (subject count, control count)}): one
    k-mer per pair of counts, reads of exactly k bases."""
    pool = iter(ref.random_reads(200, EDGE_K, 2501))
    subject, big, control, plan = [], [], [], {}
    for sc in SUBJECT_COUNTS:
        for cc in CONTROL_COUNTS:
            r = next(pool)
            plan[r] = (sc, cc)
            subject += [r] * sc
            control += [r] * cc
    for cc in (1, 2, 5, 300, 301):  # and k-mers of the control alone
        control += [next(pool)] * cc
    for sc, cc in BIG_COUNTS:
        r = next(pool)
        plan[r] = (sc, cc)
        big += [r] * sc
        control += [r] * cc
    return shuffled(subject, 1), shuffled(subject + big, 2), shuffled(control, 3), plan


@pytest.mark.parametrize("which,upper,lo,hi", [("plain", EDGE_UPPER, 5, 100), ("big", U64, 5, 100), ("big", U64, 5, U32),
                                               ("big", U64, 10002, 65536)])
def test_count_edges(rig, which, upper, lo, hi):
    """Counts on both edges of lower / upper of the count and of min_count / max_count of the strike; a control that saw a
    k-mer once (below its lower) or 301 times (beyond its upper) does not hold it and does not strike it."""
    k = EDGE_K
    subject, big, control, plan = edge_samples()
    s_reads = subject if which == "plain" else big
    s_ref, c_ref = ref_store(s_reads, k, EDGE_LOWER, upper), ref_store(control, k, EDGE_LOWER, EDGE_UPPER)
    S, s_histo = rig.store(s_reads, k, EDGE_LOWER, upper)
    C, c_histo = rig.store(control, k, EDGE_LOWER, EDGE_UPPER)
    check_store(S, s_histo, s_ref, k, EDGE_LOWER, upper)
    check_store(C, c_histo, c_ref, k, EDGE_LOWER, EDGE_UPPER)
    # the plan in the oracle's words: what the stores hold and what must come out
    key_of = {r: oracle.jf_canonical(oracle.jf_encode(r.decode()), k) for r in plan}
    s_has, c_has = dict(zip(s_ref[0].tolist(), s_ref[1].tolist())), dict(zip(c_ref[0].tolist(), c_ref[1].tolist()))
    for r, (sc, cc) in plan.items():
        if which == "plain" and sc > 301:
            continue
        assert s_has.get(key_of[r], 0) == (sc if EDGE_LOWER <= sc <= upper else 0)
        assert c_has.get(key_of[r], 0) == (cc if EDGE_LOWER <= cc <= EDGE_UPPER else 0)
    if which == "big":
        assert int(s_histo[10001]) == sum(1 for sc, _ in BIG_COUNTS if sc > 10000) and int(s_histo[10000]) == 0
        assert int(s_ref[1].max()) == 70000
    # the control's own lookup agrees: a k-mer it saw once or 301 times reads 0
    probe = np.array(sorted(key_of.values()), np.uint64)
    assert np.array_equal(C.query(probe), np.array([c_has.get(int(x), 0) for x in probe], np.uint32))
    wk, wc = rig.strike(S, [C], s_ref, [c_ref], lo, hi)
    want = sorted((key_of[r], sc) for r, (sc, cc) in plan.items()
                  if (which == "big" or sc <= 301) and max(lo, EDGE_LOWER) <= sc <= min(hi, upper) and cc in (0, 1, 301))
    assert want and list(zip(wk.tolist(), wc.tolist())) == want, "the reference is not what the plan says"
    assert lo in wc and (hi in wc or hi == U32), "no survivor sits on an edge of the strike's range"
    assert (s_ref[1] == lo - 1).any() and ((s_ref[1] > hi).any() or hi == U32), "no record of the subject lies just outside it"


# ---- b. bit relations ------------------------------------------------------------------------------------------------
SPLITS = ((12, 13), (13, 14), (16, 17))  # planted minimizers beside the first: one bin with it at 12 / 13 / 16 bits, another from there on
BITS_OF_DELTA = {+4: (13, 9), +1: (13, 12), 0: (13, 13), -1: (13, 14), -4: (13, 17)}  # S.bits - C.bits: (S.bits, C.bits)


def planted_minimizers(k: int):
    return (ref.planted_minimizer(k),) + tuple(ref.planted_pair(k, coarse, fine)[1] for coarse, fine in SPLITS)


@functools.lru_cache(maxsize=None)
def trio_samples(k: int):
    """Subject and two controls: 300 random 150-base reads each, about half of them shared, a few of the subject's given
    three and five times, and 60 k-mers around each planted minimizer, shared in part."""
    rr = ref.random_reads(600, 150, 100 + k)
    subject, c1, c2 = rr[:300] + rr[:20] * 2 + rr[20:30] * 4, rr[150:450], rr[75:225] + rr[450:600]
    for i, m in enumerate(planted_minimizers(k)):
        p = ref.kmers_in_one_bin(k, 60, 11 + i, m)
        subject, c1, c2 = subject + p[:40], c1 + p[20:50], c2 + p[10:25] + p[50:60]
    return shuffled(subject, 1), shuffled(c1, 2), shuffled(c2, 3)


def assert_spread(struck, subject, k, coarse, fine):
    """The case is not vacuous: some unit (bin at `coarse` bits) holds k-mers of the subject in two or more of its sub-bins
    (bins at `fine` bits), two planted minimizers share a unit and not a sub-bin, and some k-mer that a control strikes lies
    in a sub-bin other than its unit's first."""
    if coarse == fine:
        return
    first, *others = planted_minimizers(k)
    assert any(ref.mmer_bin(m, coarse) == ref.mmer_bin(first, coarse) and ref.mmer_bin(m, fine) != ref.mmer_bin(first, fine)
               for m in others), "no two planted minimizers part between these bit counts"
    sub = {}
    for u, f in zip(np_bin(subject, k, coarse).tolist(), np_bin(subject, k, fine).tolist()):
        sub.setdefault(u, set()).add(f)
    assert max(len(v) for v in sub.values()) >= 2, "no unit holds subject k-mers in two sub-bins"
    assert len(struck) and (np_bin(struck, k, fine) & np.uint32((1 << (fine - coarse)) - 1)).any(), \
        "every struck k-mer lies in its unit's first sub-bin"


@pytest.mark.parametrize("delta", sorted(BITS_OF_DELTA))
@pytest.mark.parametrize("k", [25, 31])
def test_bit_relations(rig, k, delta):
    """Subject finer than the control, equal, and coarser (a shallow child against deep parents): k_strike_bins takes the
    unit from the coarser side and walks 2^d bins of the other; k_strike_cands does the same for the second control, once
    at the first control's bits and once on the other side of the subject's."""
    lower, lo, hi = 1, 1, 3
    s_bits, c_bits = BITS_OF_DELTA[delta]
    # (every bit count asked for lies above what these inputs are counted at by themselves -- test_empty_sides counts them
    # so -- or the forced value would not be the one that holds)
    assert NATURAL_BITS < min(s_bits, c_bits, s_bits + delta)
    reads = trio_samples(k)
    refs = [ref_store(r, k, lower) for r in reads]
    assert int(refs[0][1].max()) > hi, "no count of the subject lies beyond the strike's range"
    for c2_bits in sorted({c_bits, s_bits + delta}):
        S, s_histo = rig.store(reads[0], k, lower, bits=s_bits)
        C1, c1_histo = rig.store(reads[1], k, lower, bits=c_bits)
        C2, c2_histo = rig.store(reads[2], k, lower, bits=c2_bits)
        for b, h, r in ((S, s_histo, refs[0]), (C1, c1_histo, refs[1]), (C2, c2_histo, refs[2])):
            check_store(b, h, r, k, lower)
        in_range = refs[0][0][(refs[0][1] >= lo) & (refs[0][1] <= hi)]
        by_c1 = in_range[np.isin(in_range, refs[1][0])]
        left = in_range[~np.isin(in_range, refs[1][0])]
        by_c2 = left[np.isin(left, refs[2][0])]
        assert_spread(by_c1, refs[0][0], k, min(s_bits, c_bits), max(s_bits, c_bits))
        assert_spread(by_c2, left, k, min(s_bits, c2_bits), max(s_bits, c2_bits))
        wk, _ = rig.strike(S, [C1, C2], refs[0], refs[1:], lo, hi)
        assert 0 < len(wk) < len(left) < len(in_range)
        for x in (S, C1, C2):
            x.free()


# ---- c. tile and trip edges --------------------------------------------------------------------------------------------
TILE = 1024  # rfx_msp.hip SB_TILE: control survivors of a unit per pass over the subject's; SB_BLK = 128 subject entries per trip
POOL = 21000


def planted_samples(k: int, n_s: int, n_c: int):
    """Control: n_c planted k-mers.  Subject: n_s planted k-mers, half of them (as far as the control has that many) the
    control's; every eighth twice, which the strike's range [1, 1] drops."""
    pool = ref.kmers_in_one_bin(k, POOL, 77)
    shared = min(n_s // 2, n_c)
    own = pool[n_c - shared:n_c] + pool[6000:6000 + n_s - shared]
    subject = tuple(r for i, r in enumerate(own) for _ in range(2 if i % 8 == 7 else 1))
    return shuffled(subject, n_s), shuffled(pool[:n_c], n_c)


def check_planted_bin(store_ref, k, bits, n):
    bins = np_bin(store_ref[0], k, bits)
    assert len(bins) == n and (bins == bins[0]).all(), "the planted bin does not hold what the case asks for"


TILE_CASES = [(3000, n_c, dc) for dc in (0, 3) for n_c in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 5000)]
TILE_CASES += [(n_s, TILE, 0) for n_s in (127, 128, 129)] + [(10000, 5000, 0), (10000, 2 * TILE + 1, 3)]


@pytest.mark.parametrize("n_s,n_c,dc", TILE_CASES)
def test_tile_and_trip_edges(rig, n_s, n_c, dc):
    """One unit whose control side fills the LDS set exactly, nearly, just beyond (the step from one pass without a
    write-back to several with one), twice and many times; a subject bin of one trip of the workgroup, nearly, just beyond;
    a control 3 bits finer, whose planted k-mers are still one bin, so that n_c must be summed over all 2^3 sub-bins."""
    k, lower, lo, hi = 25, 1, 1, 1
    s_reads, c_reads = planted_samples(k, n_s, n_c)
    s_ref, c_ref = ref_store(s_reads, k, lower), ref_store(c_reads, k, lower)
    s_bits, c_bits = NATURAL_BITS, NATURAL_BITS + dc
    check_planted_bin(s_ref, k, s_bits, n_s)
    check_planted_bin(c_ref, k, s_bits, n_c)
    check_planted_bin(c_ref, k, c_bits, n_c)
    if dc:
        assert ref.mmer_bin(ref.planted_minimizer(k), c_bits) & ((1 << dc) - 1), "the planted bin is its unit's first sub-bin"
    S, s_histo = rig.store(s_reads, k, lower)
    C, c_histo = rig.store(c_reads, k, lower, bits=c_bits if dc else None)
    check_store(S, s_histo, s_ref, k, lower)
    check_store(C, c_histo, c_ref, k, lower)
    if n_s == 10000:  # 4352 entries to a staging chunk of a small input: the bin is not one stretch of the store
        at = S.get()[3]
        assert int(at.max() - at.min()) + 1 > n_s, "the subject's bin lies in one stretch"
    wk, wc = rig.strike(S, [C], s_ref, [c_ref], lo, hi)
    shared = min(n_s // 2, n_c)
    assert int(np.isin(s_ref[0], c_ref[0]).sum()) == shared and int((s_ref[1] == 2).sum()) == n_s // 8
    assert 0 < len(wk) < n_s - shared and (wc == 1).all()


# ---- d. a list that comes short, after a write-back -----------------------------------------------------------------------
def test_list_comes_short_after_a_write_back(rig):
    """More candidates than the list is first given room for: rfx_binned_strike runs k_strike_bins a second time, over a
    store whose planted unit (five tiles of control) has had the counts of its fallen candidates put to 0 by the first."""
    k, lower = 25, 1
    rr = ref.random_reads(700, 150, 4242)
    planted_s, planted_c = planted_samples(k, 3000, 5000)
    s_reads, c_reads = rr + planted_s, planted_c + rr[:5]
    s_ref, c_ref = ref_store(s_reads, k, lower), ref_store(c_reads, k, lower)
    planted_bin = ref.mmer_bin(ref.planted_minimizer(k), NATURAL_BITS)
    assert int((np_bin(c_ref[0], k, NATURAL_BITS) == planted_bin).sum()) > 4 * TILE, "the planted unit is not several tiles"
    in_unit = s_ref[0][np_bin(s_ref[0], k, NATURAL_BITS) == planted_bin]
    assert len(in_unit) >= 3000 and 1000 < int(np.isin(in_unit, c_ref[0]).sum()) < len(in_unit)
    wk, _ = ref.expected_candidates(s_ref, [c_ref], 1, U32)
    assert len(wk) > CAND_CAP_FLOOR and len(s_ref[0]) // 256 < CAND_CAP_FLOOR, "the list does not come short"
    S, s_histo = rig.store(s_reads, k, lower)
    C, c_histo = rig.store(c_reads, k, lower)
    check_store(S, s_histo, s_ref, k, lower)
    check_store(C, c_histo, c_ref, k, lower)
    rig.strike(S, [C], s_ref, [c_ref], 1, U32)


# ---- e. shards with differing bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [+4, -4])
def test_shards_with_differing_bits(rig, delta):
    k, lower, lo, hi, n_shards = 25, 1, 1, 3, 3
    s_bits, c_bits = BITS_OF_DELTA[delta]
    reads = trio_samples(k)
    refs = [ref_store(r, k, lower) for r in reads]
    got_k, got_c, stores = [], [], [[], [], []]
    for s in range(n_shards):
        S, C1, C2 = (rig.store(r, k, lower, bits=b, shard=(s, n_shards))[0]
                     for r, b in zip(reads, (s_bits, c_bits, c_bits)))
        for i, b in enumerate((S, C1, C2)):
            keys, counts, bins, _ = b.get()
            assert len(keys) and np.array_equal(bins, np_bin(keys, k, b.bits))
            stores[i].append((keys, counts))
        own = np.isin(refs[0][0], stores[0][-1][0])  # the reference, cut to what this shard's subject holds
        shard_ref = (refs[0][0][own], refs[0][1][own])
        wk, wc = rig.strike(S, [C1, C2], shard_ref, refs[1:], lo, hi)
        got_k.append(wk)
        got_c.append(wc)
        for x in (S, C1, C2):
            x.free()
    for i in range(3):
        uk, uc = by_key(np.concatenate([x[0] for x in stores[i]]), np.concatenate([x[1] for x in stores[i]]))
        rk, rc = by_key(*refs[i])
        assert np.array_equal(uk, rk) and np.array_equal(uc, rc), "the shards' stores are not a partition of the oracle's"
    assert all(len(x) for x in got_k)
    all_k = np.concatenate(got_k)
    assert len(np.unique(all_k)) == len(all_k), "two shards list the same k-mer"
    uk, uc = by_key(all_k, np.concatenate(got_c))
    wk, wc = ref.expected_candidates(refs[0], refs[1:], lo, hi)
    assert np.array_equal(uk, wk) and np.array_equal(uc, wc)


# ---- f. empty sides ----------------------------------------------------------------------------------------------------
def test_empty_sides(rig):
    k, lower, lo, hi = 25, 1, 1, 3
    s_reads = trio_samples(k)[0]
    s_ref = ref_store(s_reads, k, lower)
    short = tuple(r[:k - 1] for r in s_reads[:50])      # reads, but no k-mer: an empty store, no bin_at
    apart = ref.random_reads(100, 150, 999)             # no key in common
    e_ref, a_ref = ref_store(short, k, lower), ref_store(apart, k, lower)
    assert len(e_ref[0]) == 0 and len(a_ref[0]) > 0 and not np.isin(a_ref[0], s_ref[0]).any()
    in_range = int(((s_ref[1] >= lo) & (s_ref[1] <= hi)).sum())
    assert 0 < in_range < len(s_ref[0])

    def stores():
        S, s_histo = rig.store(s_reads, k, lower)
        check_store(S, s_histo, s_ref, k, lower)
        E, e_histo = rig.store(short, k, lower, empty=True)
        check_store(E, e_histo, e_ref, k, lower)
        assert len(E) == 0 and not E.query(s_ref[0][:100]).any()
        return S, E

    # an empty control first, an empty control later, a control that holds other k-mers: the range alone
    S, E = stores()
    A, a_histo = rig.store(apart, k, lower)
    check_store(A, a_histo, a_ref, k, lower)
    wk, _ = rig.strike(S, [E, A, E], s_ref, [e_ref, a_ref, e_ref], lo, hi)
    assert len(wk) == in_range
    S, E = stores()
    wk, _ = rig.strike(S, [A, E], s_ref, [a_ref, e_ref], lo, hi)
    assert len(wk) == in_range
    # a control equal to the subject: nothing survives
    S, E = stores()
    S2, _ = rig.store(s_reads, k, lower)
    wk, _ = rig.strike(S, [S2], s_ref, [s_ref], lo, hi)
    assert len(wk) == 0
    # the same as a later control
    S, E = stores()
    wk, _ = rig.strike(S, [A, S2], s_ref, [a_ref, s_ref], lo, hi)
    assert len(wk) == 0
    # an empty subject
    wk, _ = rig.strike(E, [S2, A], e_ref, [s_ref, a_ref], lo, hi)
    assert len(wk) == 0
    wk, _ = rig.strike(E, [], e_ref, [], lo, hi)
    assert len(wk) == 0
