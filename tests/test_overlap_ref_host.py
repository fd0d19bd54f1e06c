"""CPU: the host references of tests/overlap_ref.py against each other and against hand-worked cases, so that the GPU
tests compare the kernels with something that is itself pinned."""
import numpy as np

from tests.overlap_ref import align3_fast, align3_one, annotate_ref


def _random_pairs(n, seed=20251):
    """Pairs of substrings (lengths 0..40) of one 80-base string -- 30 % of the time a periodic one with unit 1..4 --
    with 0..2 substitutions and 4 % 'N' each."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        if rng.random() < 0.3:
            unit = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 5))))
            common = (unit * 80)[:80]
        else:
            common = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, 80))
        pair = []
        for _ in (0, 1):
            ln = int(rng.integers(0, 41))
            at = int(rng.integers(0, 80 - ln + 1))
            s = bytearray(common[at:at + ln])
            for _ in range(int(rng.integers(0, 3))):
                if ln:
                    s[int(rng.integers(0, ln))] = b"ACGT"[int(rng.integers(0, 4))]
            for p in range(ln):
                if rng.random() < 0.04:
                    s[p] = ord("N")
            pair.append(bytes(s))
        yield (pair[0], pair[1], float(rng.choice([0, .5, .75, .9, .95, .98, 1])), int(rng.choice([0, 1, 5, 20, 50])),
               *((True, -1) if rng.random() < 0.5 else (False, 0)))


def test_align3_fast_equals_the_literal_loop():
    n = differ = 0
    seen = set()
    for a, b, pct, movl, strict3, init in _random_pairs(3200):
        want = align3_one(a, b, pct, movl, strict3, init)
        got, phase = align3_fast(a, b, pct, movl, strict3, init, with_phase=True)
        assert got == align3_fast(a, b, pct, movl, strict3, init)
        differ += got != want
        assert got == want, (a, b, pct, movl, strict3, init, got, want)
        assert (phase == 0) == (got[3] == init)
        seen.add((phase, got[2]))
        n += 1
    assert n >= 3000 and differ == 0
    # the draw reaches every outcome: nothing accepted, each phase, a perfect phase 1
    assert {(0, 0), (1, 0), (2, 0), (3, 0), (1, 1)} <= seen, seen


def test_align3_hand_worked():
    # identical strings: one phase-1 offset, perfect, phases 2 and 3 not entered
    assert align3_fast(b"ACGTACGT", b"ACGTACGT", .9, 2, False, 0) == (8, 0, 1, 8, 0)
    # B inside A at offset 3: overlap -3 (A is not the smaller one: the sign of src/OverlapSam.cpp:91)
    assert align3_fast(b"TTTACGTAGG", b"ACGTA", 1.0, 1, False, 0) == (5, -3, 1, 5, -3)
    assert align3_fast(b"ACGTA", b"TTTACGTAGG", 1.0, 1, False, 0) == (5, 3, 1, 5, 3)
    # A's last 4 = B's first 4 (phase 2): overlap = 3 - alen + 1
    assert align3_fast(b"GGGGGGACCA", b"ACCATTTTTT", 1.0, 2, False, 0, with_phase=True) == ((0, 0, 0, 4, -6), 2)
    # swapped: B's last 4 = A's first 4 (phase 3): overlap = blen - 3 - 1
    assert align3_fast(b"ACCATTTTTT", b"GGGGGGACCA", 1.0, 2, False, 0, with_phase=True) == ((0, 0, 0, 4, 6), 3)
    # 'N' never matches, not even 'N'; nothing accepted keeps the variant's start value
    assert align3_fast(b"N", b"N", 0.0, 0, True, -1) == (0, 0, 0, 0, 0)
    assert align3_fast(b"N", b"N", 0.5, 0, True, -1) == (-1, 0, 0, -1, 0)
    assert align3_fast(b"", b"ACGT", 0.0, 0, True, -1) == (-1, 0, 0, -1, 0)
    for args in ((b"ACCATTTTTT", b"GGGGGGACCA", 1.0, 2, True, -1), (b"", b"", 0.0, 0, False, 0), (b"A", b"A", 1.0, 1, True, -1)):
        assert align3_fast(*args) == align3_one(*args)


def test_phase3_strictness_at_an_exact_percentage():
    """19 of 20 is exactly float32(.95): '>=' (OverlapSam, OverlapRegion) takes it, the '>' of Overlap.cpp phase 3 does not."""
    p = b"ACGTTGCAAGCTTAGCCATG"
    a, b = b"T" + p[1:] + b"G" * 30, b"C" * 30 + p
    for fn in (align3_one, align3_fast):
        assert fn(a, b, .95, 10, False, 0) == (0, 0, 0, 19, 30)
        assert fn(a, b, .95, 10, True, -1) == (-1, 0, 0, -1, 0)
        assert fn(b, a, .95, 10, True, -1) == (-1, 0, 0, 19, -30)     # phase 2 is '>=' everywhere


def _key(kmer: bytes) -> int:
    v = 0
    for ch in kmer:
        v = v * 4 + b"ACGT".index(ch)
    return v


def test_annotate_ref_hand_worked():
    k = 3
    keys = {_key(b"ACG"), _key(b"CGT"), _key(b"AAA")}
    q = b"I" * 20
    cov = annotate_ref([b"TACGTT"], [q], keys, k)              # ACG at 1..3, CGT at 2..4
    assert cov.tolist() == [0, 1, 2, 2, 1, 0]
    assert annotate_ref([b"TTACG"], [q], keys, k).tolist() == [0] * 5          # the last window never counts
    assert annotate_ref([b"TTACGA"], [q], keys, k).tolist() == [0, 0, 1, 1, 1, 0]
    assert annotate_ref([b"AANAAAT"], [q], keys, k).tolist() == [0, 0, 0, 1, 1, 1, 0]   # N is no A
    assert annotate_ref([b"TACGTT"], [b"II#III"], keys, k).tolist() == [0] * 6  # '#' - 33 = 2 < 3: both windows bad
    assert annotate_ref([b"TACGTT"], [b"II$III"], keys, k).tolist() == [0, 1, 2, 2, 1, 0]   # '$' - 33 = 3: good
    assert annotate_ref([b"TACGTT"], [b"III"], keys, k).tolist() == [0] * 6     # no quality character: bad
    both = annotate_ref([b"", b"A", b"TACGTT", b"AAAAAA"], [b"", q, q, q], keys, k)
    assert both.tolist() == [0] + [0, 1, 2, 2, 1, 0] + [1, 2, 3, 2, 1, 0]
