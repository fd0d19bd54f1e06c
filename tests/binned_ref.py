"""Host reference of the binned route, shared by the tests: the bin function restated in numpy, hand-made reads whose k-mers
fall into a bin of one's choosing, and a store / a set difference computed from the oracle's counts.  No GPU, no fixtures,
and nothing of rufus_amd's device classes: this is what the kernels are compared with."""
import functools

import numpy as np

import oracle

SIZE = 8 << 30
M32 = np.uint64(0xFFFFFFFF)
HASH_XOR, HASH_MUL = 0x5BD1E995, 0x9E3779B1
HASH_MUL_INV = pow(HASH_MUL, -1, 1 << 32)


# ---- host restatements ---------------------------------------------------------------------------------------------
def np_revcomp(keys: np.ndarray, n: int) -> np.ndarray:
    x, r = keys.astype(np.uint64), np.zeros(len(keys), np.uint64)
    for _ in range(n):
        r = (r << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x = x >> np.uint64(2)
    return r


def np_bin(keys: np.ndarray, k: int, bits: int) -> np.ndarray:
    """rfx_devutil.h msp_key_bin restated: window k - 15 from k = 26 on, else 11; m = k - (window - 1); the minimum over the
    k-mer's own canonical m-mers of the upper 27 bits of mmer_hash, spread by msp_binhash, its top `bits` bits."""
    M32 = np.uint64(0xFFFFFFFF)
    wl = k - 15 if k >= 26 else 11
    m = k - (wl - 1)
    mmask = np.uint64((1 << (2 * m)) - 1)
    keys = keys.astype(np.uint64)
    minh = np.full(len(keys), 0xFFFFFFFF, np.uint64)
    for i in range(wl):
        f = (keys >> np.uint64(2 * i)) & mmask
        c = np.minimum(f, np_revcomp(f, m))
        h = ((c ^ np.uint64(0x5BD1E995)) * np.uint64(0x9E3779B1)) & M32
        h = h ^ (h >> np.uint64(15))
        minh = np.minimum(minh, h & np.uint64(0xFFFFFFE0))
    bh = ((((minh & np.uint64(0xFFFFFFE0)) * np.uint64(0xC2B2AE3D)) & M32) >> np.uint64(1)) | ((minh & np.uint64(32)) << np.uint64(26))
    return (bh >> np.uint64(32 - bits)).astype(np.uint32)


def by_key(keys, counts):
    o = np.argsort(keys, kind="stable")
    return np.asarray(keys, np.uint64)[o], np.asarray(counts, np.uint64)[o]


# ---- k-mers in a bin of one's choosing -------------------------------------------------------------------------------
def window_of(k: int) -> int:
    return k - 15 if k >= 26 else 11


def mmer_len(k: int) -> int:
    return k - (window_of(k) - 1)


def mmer_hash(c: np.ndarray) -> np.ndarray:
    h = ((np.asarray(c, np.uint64) ^ np.uint64(HASH_XOR)) * np.uint64(HASH_MUL)) & M32
    return h ^ (h >> np.uint64(15))


def mmer_unhash(h: np.ndarray) -> np.ndarray:
    """The 32-bit word whose mmer_hash is h: the xorshift by 15 undone, times the multiplier's inverse mod 2^32, the xor."""
    h = np.asarray(h, np.uint64)
    x = h ^ (h >> np.uint64(15)) ^ (h >> np.uint64(30))
    return ((x * np.uint64(HASH_MUL_INV)) & M32) ^ np.uint64(HASH_XOR)


def mmer_bins(mmers: np.ndarray, bits: int) -> np.ndarray:
    """The bin of every k-mer whose minimizer is the m-mer (np_bin's last step, on that m-mer's hash)."""
    minh = mmer_hash(mmers) & np.uint64(0xFFFFFFE0)
    bh = (((minh * np.uint64(0xC2B2AE3D)) & M32) >> np.uint64(1)) | ((minh & np.uint64(32)) << np.uint64(26))
    return (bh >> np.uint64(32 - bits)).astype(np.uint32)


def mmer_bin(mmer: int, bits: int) -> int:
    return int(mmer_bins(np.array([mmer], np.uint64), bits)[0])


@functools.lru_cache(maxsize=None)
def _planted_targets(k: int, n_targets: int) -> np.ndarray:
    """Canonical m-mers with the hashes t << 5, t = 0 .. n_targets - 1, in that order: those that fit 2m bits and are not
    above their reverse complement.  A hash this small is below that of (nearly) every other m-mer of a k-mer."""
    m = mmer_len(k)
    c = mmer_unhash(np.arange(n_targets, dtype=np.uint64) << np.uint64(5))
    c = c[c < np.uint64(1 << (2 * m))]
    return c[c <= np_revcomp(c, m)]


def planted_minimizer(k: int) -> int:
    """A canonical m-mer whose mmer_hash is so small that it is the minimizer of any k-mer that contains it."""
    return int(_planted_targets(k, 4096)[0])


@functools.lru_cache(maxsize=None)
def planted_pair(k: int, coarse: int, fine: int, n_targets: int = 1 << 20):
    """(planted_minimizer(k), a second planted m-mer): their bins agree at `coarse` bits and differ at `fine` bits."""
    assert coarse < fine
    first = planted_minimizer(k)
    c = _planted_targets(k, n_targets)[1:]
    c = c[(mmer_bins(c, coarse) == mmer_bin(first, coarse)) & (mmer_bins(c, fine) != mmer_bin(first, fine))]
    assert len(c), f"no second minimizer among {n_targets} targets"
    return first, int(c[0])


def kmer_text(key: int, k: int) -> bytes:
    return oracle.jf_decode(key, k).encode()


@functools.lru_cache(maxsize=None)
def kmers_in_one_bin(k: int, n: int, seed: int, mmer: int = -1) -> tuple:
    """n distinct canonical k-mers that contain the planted m-mer (`mmer`, by default planted_minimizer(k)) at a random
    offset, as byte strings of exactly k bases: one read each, one k-mer each.  All of them lie in the m-mer's bin at 28
    bits -- asserted here -- and therefore in one bin at every bit count."""
    mmer = planted_minimizer(k) if mmer < 0 else mmer
    m, wl = mmer_len(k), window_of(k)
    rng = np.random.default_rng(seed)
    keys = np.zeros(0, np.uint64)
    while len(keys) < n:
        want = 2 * n + 64
        r = rng.integers(0, 1 << (2 * k), want, dtype=np.uint64)
        sh = rng.integers(0, wl, want).astype(np.uint64) * np.uint64(2)
        r = (r & ~(np.uint64((1 << (2 * m)) - 1) << sh)) | (np.uint64(mmer) << sh)
        r = np.minimum(r, np_revcomp(r, k))
        r = r[np_bin(r, k, 28) == np.uint32(mmer_bin(mmer, 28))]
        keys = np.concatenate([keys, r])
        _, first = np.unique(keys, return_index=True)
        keys = keys[np.sort(first)]
    keys = keys[:n]
    assert len(np.unique(keys)) == n and (np_bin(keys, k, 28) == mmer_bin(mmer, 28)).all()
    return tuple(kmer_text(int(x), k) for x in keys)


def random_reads(n: int, length: int, seed: int) -> tuple:
    rows = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, (n, length))]
    return tuple(row.tobytes() for row in rows)


# ---- the reference ---------------------------------------------------------------------------------------------------
def expected_store(reads, k: int, lower: int, upper: int = 2**64 - 1):
    """(keys, counts) of the oracle's count of `reads` with lower <= count <= upper."""
    rec = oracle.count(None, k, SIZE, lower, upper, reads=reads)
    return rec.keys, rec.counts


def expected_candidates(subject, controls, lo: int, hi: int):
    """subject, controls: (keys, counts) of stores.  The subject's records with lo <= count <= hi whose key no control store
    holds, sorted by key."""
    keys, counts = by_key(*subject)
    keep = (counts >= np.uint64(lo)) & (counts <= np.uint64(hi))
    for ck, _ in controls:
        keep &= ~np.isin(keys, np.asarray(ck, np.uint64))
    return keys[keep], counts[keep]
