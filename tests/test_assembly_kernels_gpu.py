"""GPU: the assembly-side kernels of rufus_amd/csrc/rfx_overlap.hip, each against a host reference of the same
operation (tests/overlap_ref.py), kernel by kernel and input by input:
  * k_overlap_score (rfx_overlap_score) and k_overlap_pool (rfx_ovl_pool_*) against align3_fast, over one case table
    built for the places where a parallel reduction can leave the reference's sequential scan: several 256-thread
    passes over the offsets, ties between offsets and between phases, score / length exactly on min_pct, empty and
    one-base strings, the grid caps, the pool's in-place patching, moving and regrowth;
  * k_annotate (rfx_annotate) against annotate_ref.
Nothing here needs oracle/_ref."""
import functools

import numpy as np
import pytest

from rufus_amd import capi
from tests.overlap_ref import align3_fast, annotate_ref

pytestmark = pytest.mark.gpu

SAM, CONTIG, REGION = capi.OVL_SAM, capi.OVL_CONTIG, capi.OVL_REGION
# (variant, min_pct, min_ovl): the four of tests/test_overlap_gpu.py, then min_ovl = 0 (one-base overlaps), min_pct = 0
# (every offset accepted: the hardest tie-break, and a score of 0 against CONTIG's start of -1) and min_pct = 1
SETTINGS = [(SAM, .95, 20), (CONTIG, .98, 50), (REGION, .98, 50), (CONTIG, .9, 5), (CONTIG, .95, 10), (SAM, .95, 10),
            (SAM, .5, 0), (CONTIG, 0.0, 0), (CONTIG, 1.0, 1)]
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _rules(variant):
    """(strict3, init) of a variant: Overlap.cpp starts LocalBestScore at -1 and accepts phase 3 with '>'."""
    return (True, -1) if variant == CONTIG else (False, 0)


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def _rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _mutate(rng, s, n_sub, n_n):
    """n_sub bases replaced by a DIFFERENT base and n_n by 'N', all at distinct places."""
    s = bytearray(s)
    at = rng.choice(len(s), n_sub + n_n, replace=False)
    for p in at[:n_sub]:
        s[p] = b"ACGT"[(b"ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
    for p in at[n_sub:]:
        s[p] = ord("N")
    return bytes(s)


F4_CASES = [(20, 1, .95, 10), (40, 2, .95, 10), (100, 5, .95, 10), (50, 1, .98, 20), (100, 2, .98, 20), (10, 1, .9, 5),
            (20, 2, .9, 5), (4, 1, .75, 1)]


@functools.lru_cache(maxsize=None)
def case_table():
    """[(family, tag, a, b)]: the pairs every scoring test shares."""
    rng = np.random.default_rng(4242)
    base = _rand(rng, 3000)
    t = []
    # F1: B is a substring of the same text, `shift` after A's start: the overlap the assemblers look for, at lengths
    # from one pass of the 256 threads (150 / 150: ~ 300 offsets) to several and a ragged last one (700 / 300: ~ 1000)
    s0 = 1000
    for alen, blen in ((150, 150), (150, 60), (60, 150), (700, 300), (300, 700), (257, 256), (256, 257), (33, 1000)):
        for shift in (-alen + 30, -40, -1, 0, 1, 40, max(alen, blen) - 30):
            for n_sub, n_n in ((0, 0), (2, 0), (1, 2), (12, 0)):
                b = _mutate(rng, base[s0 + shift:s0 + shift + blen], n_sub, n_n)
                t.append(("F1", (alen, blen, shift, n_sub, n_n), base[s0:s0 + alen], b))
    # F2: periodic strings, B one base later: many offsets share a score, the earliest in the loop order must win
    for unit in (b"A", b"AC", b"ACG", b"ACGT", b"AAN"):
        for la, lb in ((90, 60), (60, 90), (64, 64)):
            t.append(("F2", (unit, la, lb), (unit * 100)[:la], (unit * 100)[1:1 + lb]))
    # F3: P + R1 + P against P + R2 + P.  A's last |P| = B's first |P| (phase 2) and B's last |P| = A's first |P| (phase
    # 3) score |P| each; phase 2 comes first and must be the one reported.  R2 differs from R1 at every base and is
    # 2 |P| + 10 long, so the one phase-1 offset has 2 |P| of 4 |P| + 10 and is refused wherever min_pct >= .5.
    for plen in (20, 50, 100):
        p, r1 = _rand(rng, plen), _rand(rng, 2 * plen + 10)
        r2 = r1.translate(bytes.maketrans(b"ACGT", b"CGTA"))
        t.append(("F3", plen, p + r1 + p, p + r2 + p))
    # F4: an overlap of n bases with exactly n * (1 - min_pct) mismatches, between two otherwise unrelated strings
    for n, mis, pct, movl in F4_CASES:
        p = _rand(rng, n)
        a, b = _mutate(rng, p, mis, 0) + _rand(rng, 70), _rand(rng, 70) + p
        t.append(("F4", (n, mis, pct, movl, "fwd"), a, b))
        t.append(("F4", (n, mis, pct, movl, "swapped"), b, a))
    # F5: degenerate
    q = base[200:350]
    for b in (b"", b"A", b"N" * 150, q, q[:-1], q[1:], b"moved"):
        t.append(("F5", b[:8], q, b))
    for a, b in ((b"", b""), (b"", b"ACGT"), (b"A", b"A"), (b"N", b"N")):
        t.append(("F5", (a, b), a, b))
    return t


@functools.lru_cache(maxsize=None)
def want(a: bytes, b: bytes, si: int):
    """(the five numbers, winning phase) of the reference for one pair under SETTINGS[si]."""
    variant, pct, movl = SETTINGS[si]
    return align3_fast(a, b, pct, movl, *_rules(variant), with_phase=True)


def groups():
    """The table by query, so that one call carries many candidates: [(a, [b, ...])]."""
    g = {}
    for _, _, a, b in case_table():
        g.setdefault(a, []).append(b)
    return list(g.items())


def _rows(a, bs, si):
    return np.array([want(a, b, si)[0] for b in bs], np.int32).reshape(len(bs), 5)


def test_case_table_reaches_every_outcome():
    """The reference's own answers over table x settings: the table keeps its teeth only while every outcome stays
    well represented."""
    n = {"none": 0, "p1": 0, "p2": 0, "p3": 0, "perfect": 0}
    f3_phase2 = 0
    for fam, tag, a, b in case_table():
        for si, (variant, pct, movl) in enumerate(SETTINGS):
            (s1, o1, perfect, sf, of), phase = want(a, b, si)
            n["perfect" if perfect else ("none", "p1", "p2", "p3")[phase]] += 1
            # F3 (min_pct = 0 accepts the phase-1 offset with its 2 |P| matches: nothing to tie there)
            if fam == "F3" and pct > 0 and phase:
                assert (phase, sf, of) == (2, tag, tag - len(a)) and s1 == _rules(variant)[1], (tag, SETTINGS[si])
                f3_phase2 += 1
    assert min(n.values()) >= 25, n
    assert f3_phase2 >= 12, f3_phase2
    assert len(case_table()) >= 260


def test_overlap_score_equals_reference_on_the_table(ctx):
    for a, bs in groups():
        for si, (variant, pct, movl) in enumerate(SETTINGS):
            got = capi.overlap_score(ctx, a, bs, pct, movl, variant)
            exp = _rows(a, bs, si)
            bad = np.flatnonzero((got != exp).any(axis=1))
            assert not len(bad), (SETTINGS[si], len(a), a[:20], bs[bad[0]][:20], len(bs[bad[0]]), got[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("n, mis, pct, movl", F4_CASES)
def test_score_over_length_exactly_on_min_pct(ctx, n, mis, pct, movl):
    """(n - mis) / n == float32(min_pct): phase 3 takes it with '>=' (SAM, REGION) and not with the '>' of Overlap.cpp;
    phase 2 (the swapped pair) takes it under every variant."""
    pairs = {tag[4]: (a, b) for fam, tag, a, b in case_table() if fam == "F4" and tag[:4] == (n, mis, pct, movl)}
    assert np.float32(n - mis) / np.float32(n) == np.float32(pct)
    for variant in (SAM, CONTIG, REGION):
        strict3, init = _rules(variant)
        fwd = (init, 0, 0, init, 0) if variant == CONTIG else (0, 0, 0, n - mis, 70)
        for (a, b), exp in ((pairs["fwd"], fwd), (pairs["swapped"], (init, 0, 0, n - mis, -70))):
            assert align3_fast(a, b, pct, movl, strict3, init) == exp, (variant, exp)
            got = capi.overlap_score(ctx, a, [b], pct, movl, variant)
            assert tuple(int(x) for x in got[0]) == exp, (variant, got[0], exp)


def _short_strings(rng, n):
    """n distinct strings of 6..12 bases around one 12-base text, so that their scores against it differ."""
    text = _rand(rng, 12)
    out = {text[:6], text[3:], text[2:11], text}
    while len(out) < n:
        ln = int(rng.integers(6, 13))
        at = int(rng.integers(0, 13 - ln))
        out.add(_mutate(rng, text[at:at + ln], int(rng.integers(0, 2)), int(rng.integers(0, 2))))
    return text, sorted(out)


def test_overlap_score_grid_stride(ctx):
    """4100 candidates: past the 4096-workgroup cap, so the first workgroups take a second candidate."""
    rng = np.random.default_rng(9)
    a, distinct = _short_strings(rng, 7)
    pick = rng.integers(0, len(distinct), 4100)
    cands = [distinct[i] for i in pick]
    for variant, pct, movl in ((SAM, .5, 0), (CONTIG, .75, 2)):
        ref = np.array([align3_fast(a, b, pct, movl, *_rules(variant)) for b in distinct], np.int32)
        assert len({tuple(r) for r in ref}) >= 4
        got = capi.overlap_score(ctx, a, cands, pct, movl, variant)
        assert np.array_equal(got, ref[pick]), np.flatnonzero((got != ref[pick]).any(axis=1))[:5]


def test_pool_score_equals_reference_on_the_table(ctx):
    """Queries by pool index and as explicit strings, forward, reverse-complemented on the device and both: the rows
    of the reference on the query and on its host reverse complement, forward rows first."""
    strings = sorted({s for _, _, a, b in case_table() for s in (a, b)})
    index = {s: i for i, s in enumerate(strings)}
    pool = capi.OvlPool(ctx, strings)
    try:
        for a, bs in groups():
            assert set(a) <= set(b"ACGTN")
            cands = [index[b] for b in bs]
            for si, (variant, pct, movl) in enumerate(SETTINGS):
                exp = np.stack([_rows(a, bs, si), _rows(revcomp(a), bs, si)])
                both = pool.score(cands, pct, movl, variant, 2, query=index[a])
                assert both.shape == (2, len(bs), 5)
                for strand in (0, 1):
                    bad = np.flatnonzero((both[strand] != exp[strand]).any(axis=1))
                    assert not len(bad), (SETTINGS[si], strand, a[:20], len(a), bs[bad[0]][:20], both[strand][bad[0]],
                                          exp[strand][bad[0]])
                    one = pool.score(cands, pct, movl, variant, strand, query=index[a])
                    assert one.shape == (1, len(bs), 5) and np.array_equal(one[0], exp[strand]), (SETTINGS[si], strand)
                    one = pool.score(cands, pct, movl, variant, strand, a_explicit=a)
                    assert np.array_equal(one[0], exp[strand]), (SETTINGS[si], strand, "explicit")
                assert np.array_equal(pool.score(cands, pct, movl, variant, 2, a_explicit=a), exp), (SETTINGS[si], "explicit")
    finally:
        pool.free()


def test_pool_grid_stride_and_buffer_regrowth(ctx):
    """One pool, three calls: 8 candidates; 4100 x 2 strands = 8200 work items (past the 8192-workgroup cap, and the
    candidate / output buffers regrow past their first 4096); 105 000 x 2 strands, whose 4.2 MB of results do not fit
    the 4 MiB page-locked buffer and come back through the pageable read-back."""
    rng = np.random.default_rng(21)
    a, distinct = _short_strings(rng, 16)
    pool = capi.OvlPool(ctx, distinct + [a])
    variant, pct, movl = SAM, .5, 0
    ref = np.stack([np.array([align3_fast(q, b, pct, movl, *_rules(variant)) for b in distinct], np.int32)
                    for q in (a, revcomp(a))])
    assert len({tuple(r) for r in ref[0]}) >= 6 and len({tuple(r) for r in ref[1]}) >= 3
    assert not np.array_equal(ref[0], ref[1])
    try:
        for n in (8, 4100, 105_000):
            pick = rng.integers(0, 16, n).astype(np.int32)
            got = pool.score(pick, pct, movl, variant, 2, query=16)
            assert got.shape == (2, n, 5)
            assert got.nbytes > (1 << 22) or n < 105_000
            for strand in (0, 1):
                assert np.array_equal(got[strand], ref[strand][pick]), \
                    (n, strand, np.flatnonzero((got[strand] != ref[strand][pick]).any(axis=1))[:5])
        got = pool.score(np.arange(8, dtype=np.int32), pct, movl, variant, 1, a_explicit=a)   # and small again
        assert np.array_equal(got[0], ref[1][:8])
    finally:
        pool.free()


def test_pool_updates_leave_the_other_entries_alone(ctx):
    """rfx_ovl_pool_set: shorter, longer within the entry's room, beyond it (the entry moves to the arena's end), empty,
    and one entry so long that the arena is reallocated and copied.  After each step the changed entry and the
    untouched ones score as a host mirror of the pool says."""
    rng = np.random.default_rng(33)
    text = _rand(rng, 4000)
    cur = [text[40 * i:40 * i + 150] for i in range(11)] + [b"ACGT"]       # entry 11 is never scored
    pool = capi.OvlPool(ctx, cur)
    scored = list(range(11))
    checks = ((SAM, .95, 20), (CONTIG, .9, 5))

    def check(step):
        for query in (0, 3, 5):
            for variant, pct, movl in checks:
                got = pool.score(scored, pct, movl, variant, 2, query=query)
                for strand, a in ((0, cur[query]), (1, revcomp(cur[query]))):
                    exp = np.array([align3_fast(a, cur[j], pct, movl, *_rules(variant)) for j in scored], np.int32)
                    assert np.array_equal(got[strand], exp), (step, query, strand, np.flatnonzero((got[strand] != exp).any(axis=1)))
        return sum(int((pool.score(scored, .95, 20, SAM, 0, query=q)[0, :, 3] > 0).sum()) for q in (0, 3, 5))

    def put(i, s):
        pool.set(i, s)
        cur[i] = s

    try:
        assert check("start") >= 9                           # neighbours overlap: the scores are not all "nothing"
        put(3, text[120:200])                                # shorter
        check("shorter")
        put(3, text[120:120 + 289])                          # longer, within its room of 150 + 75 + 64 = 289
        check("longer in place")
        put(3, text[100:100 + 290])                          # one more than its room: moves behind the last entry
        check("moved")
        put(5, text[200:1500])                               # far beyond (and now the query is 1300 long)
        check("moved far")
        put(4, b"")                                          # empty
        check("empty")
        put(4, text[150:310])                                # and back to something, in place
        check("refilled")
        put(11, _rand(rng, 1_300_000))                       # the arena (about 1 MiB of slack) has to grow and be copied
        assert check("arena grown") >= 9
        put(0, text[0:700])                                  # and a move inside the new arena
        check("moved after growth")
    finally:
        pool.free()


def test_refusals_leave_the_pool_usable(ctx):
    rng = np.random.default_rng(5)
    strings = [_rand(rng, 100), _rand(rng, 120), _rand(rng, 150 * 1024 - 16 - 100 + 1)]
    pool = capi.OvlPool(ctx, strings)
    exp = np.array([align3_fast(strings[0], strings[j], .5, 0, False, 0) for j in (0, 1)], np.int32)
    try:
        for bad in ([0, 3], [-1], [1, 0, 2**31 - 1]):
            with pytest.raises(capi.RufusError, match=rf"\({capi.E_INVAL}\)"):
                pool.score(bad, .5, 0, SAM, 0, query=0)
        with pytest.raises(capi.RufusError, match=rf"\({capi.E_INVAL}\)"):
            pool.score([0, 1], .5, 0, SAM, 3, query=0)
        with pytest.raises(capi.RufusError, match=rf"\({capi.E_INVAL}\)"):
            pool.score([0, 1], .5, 0, SAM, 0, query=3)
        with pytest.raises(capi.RufusError, match=rf"\({capi.E_INVAL}\)"):
            pool.set(3, b"ACGT")
        # alen + max_blen + 16 one byte over the 150 KiB of LDS
        with pytest.raises(capi.RufusError, match=rf"\({capi.E_RANGE}\)"):
            pool.score([1, 2], .5, 0, SAM, 2, query=0)
        with pytest.raises(capi.RufusError, match=rf"\({capi.E_RANGE}\)"):
            pool.score([0, 1], .5, 0, SAM, 0, a_explicit=strings[2] + b"ACGTACGTACGTACGTACGTA")
        with pytest.raises(capi.RufusError, match=rf"\({capi.E_RANGE}\)"):
            capi.overlap_score(ctx, strings[0], [strings[1], strings[2]], .5, 0, SAM)
        assert np.array_equal(pool.score([0, 1], .5, 0, SAM, 0, query=0)[0], exp)
        assert np.array_equal(capi.overlap_score(ctx, strings[0], strings[:2], .5, 0, SAM), exp)
    finally:
        pool.free()


# ---------------------------------------------------------------------------------------------------
# K7
# ---------------------------------------------------------------------------------------------------
def _lengths(k):
    return [0, 1, k - 1, k, k + 1, 31, 32, 33, 64, 65, 300, 2000]


KINDS = ("listed", "revcomp", "run", "last", "n_in_a", "qual", "t40")


def _annotate_case(k, block, seed=77):
    """(seqs, quals, hash-list text) of one block.  Listed: a few random k-mers, every window of a 2k + 5 base `run`
    text, and T * k (with its reverse complement A * k; for k = 32 the key of T * 32 is all ones, the table's empty
    marker).  Each contig is random text with one kind of content planted where its length allows:
      listed / revcomp  listed k-mers (their reverse complements) at random places;
      run               a stretch of the run text: consecutive listed windows, coverage climbs to k;
      last              a listed k-mer as the very last window (never counted) and one more inside;
      n_in_a            A * k with an N in it (N packs as A and must not match), and an intact A * k;
      qual              listed k-mers with one base of quality '!', '"', '#' (bad) or '$' (good) inside;
      t40               T * 40."""
    rng = np.random.default_rng(seed + k)
    listed = [_rand(rng, k) for _ in range(6)]
    run = _rand(rng, 2 * k + 5)
    text = b"".join(km + b" 5\n" for km in listed + [run[i:i + k] for i in range(k + 6)] + [b"T" * k])

    def contig(length, kind):
        s, q = bytearray(_rand(rng, length)), bytearray(b"I" * length)
        if length > 2 and rng.random() < 0.3:
            s[int(rng.integers(0, length))] = ord("N")

        def plant(piece, at=None):
            if len(piece) < length:
                at = int(rng.integers(0, length - len(piece))) if at is None else at
                s[at:at + len(piece)] = piece
                return at
            return None

        if kind in ("listed", "revcomp"):
            for _ in range(1 + length // 100):
                km = listed[int(rng.integers(0, 6))]
                plant(km if kind == "listed" else revcomp(km))
        elif kind == "run":
            plant(run if length > len(run) else run[:max(length - 1, 0)], 0 if length <= len(run) + 1 else None)
        elif kind == "last":
            plant(listed[0])
            if length >= k:
                s[length - k:] = listed[1]
        elif kind == "n_in_a":
            at = plant(b"A" * k)
            if length > 3 * k:
                other = (at + k + 1) if at + 2 * k + 2 < length else 0
                s[other:other + k] = b"A" * (k // 2) + b"N" + b"A" * (k - k // 2 - 1)
        elif kind == "qual":
            for i in range(1 + length // 60):
                at = plant(listed[i % 6])
                if at is not None:
                    q[at + int(rng.integers(0, k))] = b"!\"#$"[i % 4]
        elif kind == "t40":
            if length > 40:
                plant(b"T" * 40)
            else:
                s[:] = b"T" * length
        return bytes(s), bytes(q)

    if block == "one":                         # one contig, one workgroup with one live thread
        spec = [(300, "run")]
    elif block == "uniform64":                 # one full workgroup, every contig of one length
        spec = [(300, KINDS[i % 7]) for i in range(64)]
    elif block == "uniform65_short":           # k + 1 bases each: exactly one window that counts, and a second workgroup
        spec = [(k + 1, ("listed", "last", "t40", "run")[i % 4]) for i in range(65)]
    else:                                      # ragged65: every length with (12 and 7 are coprime) varying content
        lens = _lengths(k)
        spec = [(lens[i % 12], KINDS[i % 7]) for i in range(65)]
    seqs, quals = zip(*(contig(ln, kind) for ln, kind in spec))
    return list(seqs), list(quals), text


@pytest.mark.parametrize("block", ["one", "uniform64", "uniform65_short", "ragged65"])
@pytest.mark.parametrize("k", [5, 16, 25, 31, 32])
def test_annotate_equals_reference(ctx, k, block):
    seqs, quals, text = _annotate_case(k, block)
    keys = capi.hashlist_keys(text, k)
    assert (np.uint64(2**64 - 1) in keys) == (k == 32)
    want_cov = annotate_ref(seqs, quals, keys, k)
    assert want_cov.sum() > 0 and len(want_cov) == sum(len(s) for s in seqs)
    if block in ("one", "uniform64", "ragged65"):
        assert want_cov.max() == k                        # a run of listed windows climbs all the way
    mset = capi.MutantSet(ctx, keys, k)
    blk = ctx.upload(capi.PackedReads.from_reads(seqs, quals, 3, capi.PACK_FILTER))
    try:
        got = mset.annotate(blk)
        assert got.dtype == np.uint32 and got.shape == want_cov.shape
        bad = np.flatnonzero(got != want_cov)
        assert not len(bad), (k, block, bad[:10], got[bad[:10]], want_cov[bad[:10]])
    finally:
        blk.free()
        mset.free()


def test_annotate_named_cases(ctx):
    """The answers written out: the last window, N inside A * k, the quality threshold, the all-ones key."""
    k = 5
    keys = capi.hashlist_keys(b"ACGTA 5\nAAAAA 5\n", k)
    mset = capi.MutantSet(ctx, keys, k)
    q = b"I" * 12
    cases = [(b"GGACGTAGG", q[:9], [0, 0, 1, 1, 1, 1, 1, 0, 0]),
             (b"GGGGACGTA", q[:9], [0] * 9),                          # the listed k-mer is the last window
             (b"GGTACGTGG", q[:9], [0, 0, 1, 1, 1, 1, 1, 0, 0]),      # its reverse complement
             (b"GAANAAG", q[:7], [0] * 7),                            # N packs as A
             (b"GAAAAAAG", q[:8], [0, 1, 2, 2, 2, 2, 1, 0]),
             (b"GGACGTAGG", b"IIII#IIII", [0] * 9),                   # quality 2: bad
             (b"GGACGTAGG", b"IIII$IIII", [0, 0, 1, 1, 1, 1, 1, 0, 0]),   # quality 3: good
             (b"", b"", []), (b"A", b"I", [0])]
    seqs, quals, exp = zip(*cases)
    blk = ctx.upload(capi.PackedReads.from_reads(list(seqs), list(quals), 3, capi.PACK_FILTER))
    try:
        flat = [x for e in exp for x in e]
        assert annotate_ref(seqs, quals, keys, k).tolist() == flat
        assert mset.annotate(blk).tolist() == flat
    finally:
        blk.free()
        mset.free()
    keys = capi.hashlist_keys(b"T" * 32 + b" 5\n", 32)
    mset = capi.MutantSet(ctx, keys, 32)
    blk = ctx.upload(capi.PackedReads.from_reads([b"T" * 40, b"G" + b"A" * 33], [b"I" * 40, b"I" * 34], 3, capi.PACK_FILTER))
    try:
        t40 = [min(i + 1, 8, 39 - i) for i in range(39)] + [0]         # the 8 windows ending at 31..38
        a33 = [0] + [1] * 32 + [0]                                     # A * 32 at 1..32; the one at 2..33 is the last window
        flat = t40 + a33
        assert annotate_ref([b"T" * 40, b"G" + b"A" * 33], [b"I" * 40, b"I" * 34], keys, 32).tolist() == flat
        assert mset.annotate(blk).tolist() == flat
    finally:
        blk.free()
        mset.free()
