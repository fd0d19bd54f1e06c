"""A numpy statement of ``rfx_reads_select`` (not a test): which reads a mask selects, and the packed arrays of the
selected reads cut out of the packed arrays of the block.  tests/test_select_host.py checks it against the host packer
over the selected reads' TEXT; tests/test_select_gpu.py checks the kernels against it."""
import numpy as np

EVEN = np.uint64(0x5555555555555555)
ONE = np.uint64(1)


def effective_mask(mask, n: int, pairs: bool) -> np.ndarray:
    """The ceil(n / 64) mask words with a bit per SELECTED read: bits at or above n cleared; pairs: read r is selected
    when bit r or bit r ^ 1 is set (the last read of an odd block has no mate and goes by its own bit)."""
    nw = (n + 63) // 64
    m = np.array(np.asarray(mask, dtype=np.uint64)[:nw], dtype=np.uint64)
    if nw == 0:
        return m
    tail = np.uint64(0xFFFFFFFFFFFFFFFF) if n % 64 == 0 else np.uint64((1 << (n % 64)) - 1)
    m[-1] &= tail
    if pairs:
        m = m | ((m & EVEN) << ONE) | ((m >> ONE) & EVEN)
        m[-1] &= tail
    return m


def selected_reads(mask, n: int, pairs: bool) -> np.ndarray:
    """Indices of the selected reads, ascending (uint32)."""
    m = effective_mask(mask, n, pairs)
    bits = np.unpackbits(m.view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(bits).astype(np.uint32)


def select_packed(arrays: dict, n: int, mask, pairs: bool):
    """(arrays, origin): the dict ``ReadBlock.get()`` would return for the block of the selected reads (an array the
    source lacks stays None), and the index of every selected read in the source."""
    origin = selected_reads(mask, n, pairs)
    lens = np.asarray(arrays["len"][:n], dtype=np.uint32)[origin]
    nwords = (lens.astype(np.uint64) + np.uint64(31)) // np.uint64(32)
    word_off = np.zeros(len(origin) + 1, dtype=np.uint32)
    word_off[1:] = np.cumsum(nwords)
    src = np.concatenate([np.arange(int(arrays["word_off"][r]), int(arrays["word_off"][r]) + int(w), dtype=np.int64)
                          for r, w in zip(origin, nwords)] + [np.zeros(0, np.int64)])
    out = {"word_off": word_off, "len": lens}
    for name in ("codes", "acgt", "good"):
        a = arrays.get(name)
        out[name] = None if a is None else np.ascontiguousarray(a[src])
    return out, origin


# ---------------------------------------------------------------------------------------------------
# the shapes both test files use
# ---------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 150, 151, 250, 1500)      # around the word and two-word boundaries, ragged
READ_COUNTS = (0, 1, 2, 3, 63, 64, 65, 129)                         # around the mask word boundary, odd and even
_ALPHABET = np.frombuffer(b"ACGT" * 6 + b"N", dtype=np.uint8)        # 4 % N


def ragged_reads(rng, n: int):
    """(seqs, quals): n reads whose lengths walk through LENGTHS from a random start, with Ns and low qualities."""
    start = int(rng.integers(0, len(LENGTHS)))
    seqs, quals = [], []
    for i in range(n):
        L = LENGTHS[(start + i) % len(LENGTHS)]
        seqs.append(_ALPHABET[rng.integers(0, len(_ALPHABET), L)].tobytes())
        quals.append((33 + rng.integers(2, 41, L)).astype(np.uint8).tobytes())      # a third below min_q = 15
    return seqs, quals


def masks_for(rng, n: int) -> dict:
    """name -> mask of ceil(n / 64) words (at least one): none, all, alternating, last read only, mate-2 bits only, random
    (all with zeros at and above bit n), and two of them with every bit at or above n set."""
    nw = max(1, (n + 63) // 64)
    rnd = rng.integers(0, 1 << 32, nw, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, nw, dtype=np.uint64)
    last = np.zeros(nw, np.uint64)
    if n:
        last[(n - 1) // 64] = ONE << np.uint64((n - 1) % 64)
    valid = np.zeros(nw, np.uint64)
    valid[:(n + 63) // 64] = effective_mask(np.full(nw, ~np.uint64(0)), n, False)
    out = {"none": np.zeros(nw, np.uint64), "all": valid.copy(), "alternating": EVEN & valid, "last": last,
           "mate2": ~EVEN & valid, "random": rnd & valid}
    out["none+garbage"] = ~valid
    out["random+garbage"] = out["random"] | ~valid
    return out


def packed_dict(p, n: int) -> dict:
    """A capi.PackedReads as the dict ReadBlock.get() returns."""
    nw = int(p.word_off[n])
    return {"codes": p.codes[:nw], "acgt": None if p.acgt is None else p.acgt[:nw],
            "good": None if p.good is None else p.good[:nw], "word_off": p.word_off[:n + 1], "len": p.len[:n]}
