"""tests/run_map_ref.py against a brute-force minimizer per k-mer (no GPU): every k-mer's window is hashed on its own,
m-mer by m-mer, from the bases; the reference's rows are decoded and must tile the read's k-mer end positions with exactly
the brute-force runs."""
import numpy as np
import pytest

from tests import run_map_ref as ref
from tests.binned_ref import HASH_MUL, HASH_XOR, mmer_len, planted_minimizer, window_of


def _hash(c: int) -> int:
    h = ((c ^ HASH_XOR) * HASH_MUL) & 0xFFFFFFFF
    return h ^ (h >> 15)


def _brute_kmers(codes, valid, k, canonical):
    """p -> (minimizer hash with the position in its low five bits, end of the minimizer m-mer), valid k-mers only."""
    m, wl, out = mmer_len(k), window_of(k), {}
    for p in range(k - 1, len(codes)):
        if not all(valid[p - k + 1:p + 1]):
            continue
        best = None
        for q in range(p - wl + 1, p + 1):                # the m-mer of bases q - m + 1 .. q
            f = r = 0
            for j in range(q - m + 1, q + 1):
                f = (f << 2) | int(codes[j])
            for j in range(q, q - m, -1):
                r = (r << 2) | (3 - int(codes[j]))
            key = (_hash(min(f, r) if canonical else f) & 0xFFFFFFE0) | (q & 31)
            if best is None or key < best[0]:
                best = (key, q)
        out[p] = best
    return out


def _decode(row, k):
    """A row's entries -> (runs [(first end, last end, back, half)], gaps [(first, last)], count)."""
    cnt = ref.entry_count(row)
    flags = int(np.frombuffer(row[28:32].tobytes(), np.uint32)[0])
    runs, gaps, pos = [], [], k - 1
    for i in range(min(cnt, 28)):
        lo, hi = int(row[i]) & 15, int(row[i]) >> 4
        if lo == 15:
            gaps.append((pos, pos + hi))
            pos += hi + 1
        else:
            runs.append((pos, pos + lo, hi, (flags >> i) & 1 if cnt <= 27 else None))
            pos += lo + 1
    return runs, gaps, cnt


def _reads(seed, k, n=60):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.choice([0, 10, 24, 25, 31, 32, 33, 64, 65, 89, 150, 160]))
        codes = rng.integers(0, 4, L).astype(np.uint8)
        valid = np.ones(L, bool)
        kind = i % 6
        if kind == 1 and L:                               # scattered N
            valid[rng.integers(0, L, max(1, L // 40))] = False
        elif kind == 2 and L > 40:                        # a long stretch of N
            a = int(rng.integers(0, L - 30))
            valid[a:a + int(rng.integers(17, 30))] = False
        elif kind == 3:                                   # equal m-mers: the position breaks the tie at every base
            codes[:] = rng.integers(0, 4)
        elif kind == 4 and L:                             # a short period
            codes[:] = np.resize(rng.integers(0, 4, int(rng.integers(2, 5))), L)
        elif kind == 5:
            valid[:] = False
        elif kind == 0 and L >= 64:                       # a minimizer that stays for a whole window: the cap's cut
            m, c = mmer_len(k), planted_minimizer(k)
            codes[20:20 + m] = [(c >> (2 * (m - 1 - j))) & 3 for j in range(m)]
        out.append((codes, valid))
    return out


@pytest.mark.parametrize("k", [23, 25, 27, 31])
@pytest.mark.parametrize("canonical", [True, False])
def test_reference_rows_are_the_brute_force_runs(k, canonical):
    reads = _reads(1000 * k + canonical, k)
    width = max(len(c) for c, _ in reads)
    codes, valid = np.zeros((len(reads), width), np.uint8), np.zeros((len(reads), width), bool)
    for r, (c, v) in enumerate(reads):
        codes[r, :len(c)], valid[r, :len(c)] = c, v
    all_runs = ref.read_runs(codes, valid, k, canonical)
    cap, seen_over, seen_gap, seen_cap = ref.run_cap(k), 0, 0, 0
    for r, (c, v) in enumerate(reads):
        row, over = ref.map_row(all_runs[r], k)
        brute = _brute_kmers(c, v, k, canonical)
        runs, gaps, cnt = _decode(row, k)
        assert over == (cnt == 31)
        if over:
            seen_over += 1
            assert (row[28:] == 0xFF).all()
        else:
            assert cnt == len(runs) + len(gaps) <= 27 and (row[cnt:28] == 0xFF).all()
        covered = set()
        for i, (a, b, back, half) in enumerate(runs):
            keys = {brute[p] for p in range(a, b + 1)}    # (KeyError: a run over an invalid k-mer)
            assert len(keys) == 1 and b - a + 1 <= cap
            key, q = next(iter(keys))
            assert b - q == back and (half is None or half == (key >> 5) & 1)
            covered.update(range(a, b + 1))
            if not over or i + 1 < len(runs):             # maximal: the k-mer behind is invalid, another minimizer's, or the cap
                nxt = brute.get(b + 1)
                assert nxt is None or nxt != (key, q) or b - a + 1 == cap
                seen_cap += nxt == (key, q)
            assert a == k - 1 or (a - 1) not in brute or brute[a - 1] != (key, q) or (a - 1) in covered
        for a, b in gaps:
            seen_gap += 1
            assert b - a < 16 and not any(p in brute for p in range(a, b + 1))
        if not over:                                      # every valid k-mer is in a run; what follows the last run is invalid
            assert covered == set(brute)
        else:
            assert covered <= set(brute)
    assert seen_over and seen_gap and (cap >= window_of(k) or seen_cap)


def test_unpack_block_reads_words_and_masks():
    rng = np.random.default_rng(5)
    lens = np.array([0, 1, 31, 32, 33, 64, 150], np.uint32)
    nw = (lens.astype(np.int64) + 31) // 32
    off = np.concatenate([[0], np.cumsum(nw)]).astype(np.uint32)
    codes = [rng.integers(0, 4, int(L)) for L in lens]
    valid = [rng.integers(0, 2, int(L)).astype(bool) for L in lens]
    words, acgt = np.zeros(int(off[-1]), np.uint64), np.zeros(int(off[-1]), np.uint32)
    for r, L in enumerate(lens):
        for i in range(int(L)):
            words[off[r] + i // 32] |= np.uint64(int(codes[r][i]) << (2 * (i % 32)))
            acgt[off[r] + i // 32] |= np.uint32(int(valid[r][i]) << (i % 32))
    c, v = ref.unpack_block({"codes": words, "acgt": acgt, "word_off": off, "len": lens})
    for r, L in enumerate(lens):
        assert (c[r, :L] == codes[r]).all() and (v[r, :L] == valid[r]).all() and not v[r, L:].any()
