"""Inputs of the tests of `RUFUS.Filter A.fastq.gz B.fastq.gz` (tests/test_filter_bgzf_host.py, tests/test_filter_bgzf_gpu.py):
ragged mate pairs drawn from a small genome, a hash list that pulls a small share of them, and the pulled records as the
oracle's filter gives them.  Not a conftest: the test modules import it."""
import numpy as np

import oracle

K, MIN_Q, THRESH = 25, 15, 1
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def ragged_pairs(n_pairs, seed=5, genome_len=400_000):
    """(genome, [mate-1 records], [mate-2 records]): reads of 26 .. 150 bases (half of them 150), N and lower-case bases,
    low qualities; mate-2 headers are longer than mate-1's, so the two files' records differ in length."""
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, genome_len)].tobytes()
    m1, m2 = [], []
    for i in range(n_pairs):
        at = int(rng.integers(0, genome_len - 400))
        recs = []
        for mate in (1, 2):
            L = 150 if rng.random() < 0.5 else int(rng.integers(26, 151))
            s = bytearray(genome[at:at + L] if mate == 1 else genome[at + 400 - L:at + 400].translate(_COMP)[::-1])
            q = bytearray((33 + rng.integers(20, 41, L)).astype(np.uint8).tobytes())
            if rng.random() < 0.02:
                s[5:9] = bytes(s[5:9]).lower()
                q[10:14] = b"####"
            if rng.random() < 0.02:
                s[int(rng.integers(0, L))] = ord("N")
            name = b"@r%d/1" % i if mate == 1 else b"@r%d/2 the second mate of pair %d, with a comment" % (i, i)
            recs.append(name + b"\n" + bytes(s) + b"\n+\n" + bytes(q) + b"\n")
        m1.append(recs[0])
        m2.append(recs[1])
    return genome, m1, m2


def hash_list(genome, n_sites, seed=6):
    """Hash-list text: the 25 k-mers around n_sites positions of the genome, canonical, as `KMER COUNT` lines."""
    rng = np.random.default_rng(seed)
    out = []
    for p in rng.integers(100, len(genome) - 100, n_sites):
        c = genome[int(p) - 24:int(p) + 25]
        for i in range(25):
            km = c[i:i + K]
            out.append(min(km, km[::-1].translate(_COMP)) + b" 12\n")
    return b"".join(out)


def pulled(hl, m1, m2):
    """(indices of the pulled pairs, mate-1 bytes, mate-2 bytes) by the oracle's filter; m1 / m2: lists of records."""
    idx = oracle.FilterSet(hl).pairs(b"".join(m1), b"".join(m2), K, MIN_Q, THRESH)
    return idx, b"".join(m1[i] for i in idx), b"".join(m2[i] for i in idx)
