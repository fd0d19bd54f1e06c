"""Host reference of a read block's RUN MAP (rufus_amd/csrc/rfx_msp.hip, k_msp_part1 HMODE 4), written
from the format's definition in numpy and plain Python.  No GPU and nothing of the kernels: this is what they are compared
with.

A read's 32 bytes say how its k-mer end positions k - 1, k, .. fall into super-k-mers:
  * every m-mer (m = mmer_len(k)) that ends at base p has the hash (mmer_hash(canonical m-mer) & ~31) | (p & 31);
  * the minimizer of the k-mer that ends at p is the minimum of that over its window_of(k) m-mers -- the position in the
    low five bits breaks ties between equal m-mers;
  * a RUN is a stretch of consecutive valid k-mers (no invalid base inside) with the same minimizer, cut at the number of
    k-mers a record holds (`run_cap`);
  * bytes 0 .. 26: one entry per run, low nibble n - 1, high nibble `back` (the run's last k-mer ends `back` bases behind
    the end of the minimizer m-mer); k-mer end positions that no run covers and that lie BEFORE a run are gap entries,
    low nibble 15, high nibble length - 1, at most 16 positions each (what follows the last run is not recorded);
  * dword 7: bit i = entry i is a run whose minimizer hash has MSP_HALF_BIT set; bits 27 .. 31 the number of entries.
    A read with more than 27 entries has no map: dword 7 is all ones (count 31), the read is on the block's overflow
    list, and bytes 0 .. 27 keep its first 28 entries (nobody reads them).  Unused bytes are 0xFF.
"""
import numpy as np

from tests.binned_ref import mmer_hash, mmer_len, np_revcomp, window_of

MSP_HMASK = 0xFFFFFFE0
MSP_HALF_BIT = 32
RMAP_ENTRIES = 27


def run_cap(k: int) -> int:
    """k-mers per record (rfx_devutil.h msp_nmax): a whole super-k-mer, n - 1 < 15, k + n - 1 <= 43 bases."""
    w, c = window_of(k), 44 - k
    return min(w, c) if w < 15 else min(15, c)


def unpack_block(packed: dict):
    """The arrays of ReadBlock.get() -> (codes, valid): uint8 / bool matrices of shape (reads, longest read), a read's
    bases first, invalid behind its end (one invalid base closes the last run: so does the padding)."""
    lens = np.asarray(packed["len"], np.int64)
    n, width = len(lens), int(lens.max()) if len(lens) else 0
    codes, valid = np.zeros((n, max(width, 1)), np.uint8), np.zeros((n, max(width, 1)), bool)
    words, acgt, off = packed["codes"], packed["acgt"], np.asarray(packed["word_off"], np.int64)
    for r in range(n):
        L = int(lens[r])
        if L == 0:
            continue
        nw = (L + 31) // 32
        w = words[off[r]:off[r] + nw]
        two = (w[:, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))) & np.uint64(3)
        codes[r, :L] = two.reshape(-1)[:L]
        a = np.asarray(acgt[off[r]:off[r] + nw], np.uint32)
        valid[r, :L] = ((a[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(-1)[:L].astype(bool)
    return codes, valid


def position_hashes(codes: np.ndarray, k: int, canonical: bool) -> np.ndarray:
    """h[r, p] of the m-mer that ends at base p of read r (uint64; all ones where p < m - 1)."""
    m = mmer_len(k)
    n, width = codes.shape
    h = np.full((n, width), 0xFFFFFFFF, np.uint64)
    if width < m:
        return h
    f = np.zeros((n, width - m + 1), np.uint64)
    for j in range(m):                                    # base p - m + 1 + j sits 2 (m - 1 - j) bits up
        f |= codes[:, j:width - m + 1 + j].astype(np.uint64) << np.uint64(2 * (m - 1 - j))
    c = f
    if canonical:
        c = np.minimum(f, np_revcomp(f.reshape(-1), m).reshape(f.shape))
    pos = np.arange(m - 1, width, dtype=np.uint64)
    h[:, m - 1:] = (mmer_hash(c) & np.uint64(MSP_HMASK)) | (pos & np.uint64(31))
    return h


def read_runs(codes: np.ndarray, valid: np.ndarray, k: int, canonical: bool):
    """Per read the list of its runs (first k-mer end, last k-mer end, minimizer hash)."""
    n, width = codes.shape
    wl, cap = window_of(k), run_cap(k)
    h = position_hashes(codes, k, canonical)
    mh = h.copy()
    for j in range(1, wl):                                # the minimum over the m-mers ending at p - wl + 1 .. p
        mh[:, j:] = np.minimum(mh[:, j:], h[:, :width - j])
    bad = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(~valid, axis=1)], axis=1)
    kv = np.zeros((n, width), bool)                       # the k-mer ending at p has no invalid base
    if width >= k:
        kv[:, k - 1:] = (bad[:, k:] - bad[:, :width - k + 1]) == 0
    out = []
    for r in range(n):
        runs, kvr, mhr, rs = [], kv[r].tolist(), mh[r].tolist(), -1
        for p in range(k - 1, width + 1):
            go_on = rs >= 0 and p < width and kvr[p] and mhr[p] == mhr[p - 1] and p - rs < cap
            if rs >= 0 and not go_on:
                runs.append((rs, p - 1, mhr[p - 1]))
                rs = -1
            if rs < 0 and p < width and kvr[p]:
                rs = p
        out.append(runs)
    return out


def map_row(runs, k: int):
    """(the read's 32 bytes as a uint8 array, whether it is on the overflow list) from its runs."""
    entries, flags, pos = [], 0, k - 1
    for rs, e, minh in runs:
        g = rs - pos
        while g:
            step = min(g, 16)
            entries.append(0xF | ((step - 1) << 4))
            g -= step
        back = (e - (minh & 31)) & 31
        assert e - rs < 15 and back < 16
        if minh & MSP_HALF_BIT and len(entries) < RMAP_ENTRIES:
            flags |= 1 << len(entries)
        entries.append((e - rs) | (back << 4))
        pos = e + 1
    row = np.full(32, 0xFF, np.uint8)
    keep = entries[:28]
    row[:len(keep)] = keep
    over = len(entries) > RMAP_ENTRIES
    row[28:32] = np.frombuffer(np.uint32(0xFFFFFFFF if over else flags | (len(entries) << 27)).tobytes(), np.uint8)
    return row, over


def block_map(packed: dict, k: int, canonical: bool):
    """(rows, overflow): the (reads, 32) uint8 map of a downloaded block and the sorted indices of its reads without one."""
    codes, valid = unpack_block(packed)
    rows, over = np.zeros((len(codes), 32), np.uint8), []
    for r, runs in enumerate(read_runs(codes, valid, k, canonical)):
        rows[r], o = map_row(runs, k)
        if o:
            over.append(r)
    return rows, np.array(over, np.uint32)


def entry_count(row: np.ndarray) -> int:
    """Entries of a row (31: no map)."""
    return int(row[31]) >> 3
