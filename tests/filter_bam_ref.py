"""The reference side of the `RUFUS.Filter --bam` tests (tests/test_filter_bam_host.py, tests/test_bam_filter_gpu.py,
tests/test_filter_bam_gpu.py): a record as `samtools view | PassThroughSamCheck.stranded` prints it
(src/PassThroughSamCheck.stranded.cpp:184-223), the feeder's pairing by QNAME (:225-281), the pulled pairs by the
oracle's filter, the QNAME hash, and a crafted BAM that holds every case the route branches on.  Independent of the
product: plain Python over tests/bam_ref.py's reader.  Not a conftest: the test modules import it."""
import functools

import numpy as np

import oracle
from tests import bam_ref as R
from tests import filter_bgzf_ref as F

K, MIN_Q, THRESH = F.K, F.MIN_Q, F.THRESH
_COMP = {ord("A"): "T", ord("C"): "G", ord("G"): "C", ord("T"): "A", ord("N"): "N"}
M64 = (1 << 64) - 1


def qname(r) -> bytes:
    """The printed QNAME: the name field's bytes up to the first NUL."""
    return r["name"].split(b"\0")[0]


def stranded_printed(r):
    """(SEQ, QUAL) bytes of a record of bam_ref.read_records as the stranded feeder prints them."""
    seq = r["seq"]  # ('*' for l_seq == 0)
    qual = "*" if not r["l_seq"] or r["qual"][0] == 0xFF else "".join(chr(33 + min(q, 93)) for q in r["qual"])
    if r["flag"] & 16:
        seq = "".join(_COMP.get(ord(c), "") for c in reversed(seq))  # every other letter vanishes
        qual = qual[::-1]
    return seq.encode(), qual.encode()


def name_hash(name: bytes) -> int:
    """rfx_bam_core.h bam_name_hash: FNV-1a, then the splitmix64 finaliser."""
    h = 0xCBF29CE484222325
    for c in name:
        h = ((h ^ c) * 0x100000001B3) & M64
    h = (h + 0x9E3779B97F4A7C15) & M64
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & M64
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & M64
    return h ^ (h >> 31)


def feeder_pairs(bam: R.Bam, exclude=3328):
    """(mate-1 records, mate-2 records, chromosome log): in stream order over the kept records a record meets the waiting
    record of its name -- the LATER one is mate 1, the stored one mate 2 -- or waits; pairs in completion order.  A record
    is (kept index, name, SEQ, QUAL) with the printed forms."""
    waiting, m1, m2 = {}, [], []
    for i, r in enumerate(bam.kept(exclude)):
        rec = (i, qname(r)) + stranded_printed(r)
        if rec[1] in waiting:
            m1.append(rec)
            m2.append(waiting.pop(rec[1]))
        else:
            waiting[rec[1]] = rec
    return m1, m2, bam.chr_log(exclude)


def fastq(rec) -> bytes:
    return b"@" + rec[1] + b"\n" + rec[2] + b"\n+\n" + rec[3] + b"\n"


def scan(fs, rec, k=K, min_q=MIN_Q) -> int:
    """Windows of a printed record the oracle's paired scan finds in the set."""
    return fs.scan(rec[2], rec[3], k, min_q)


def expected(bam: R.Bam, hl: bytes, exclude=3328, k=K, min_q=MIN_Q, thresh=THRESH):
    """(Mate1 bytes, Mate2 bytes, chromosome log, indices of the pulled pairs among feeder_pairs) by the oracle's filter."""
    m1, m2, log = feeder_pairs(bam, exclude)
    assert all(len(r[2]) for r in m1), "an empty mate-1 sequence line: undefined in the reference, refused by the tools"
    t1, t2 = [fastq(r) for r in m1], [fastq(r) for r in m2]
    idx = oracle.FilterSet(hl).pairs(b"".join(t1), b"".join(t2), k, min_q, thresh) if t1 else []
    return b"".join(t1[i] for i in idx), b"".join(t2[i] for i in idx), log, [int(i) for i in idx]


def own_hash_list(bam: R.Bam, exclude=3328, n_reads=6) -> bytes:
    """A hash list for a file that has none: every 7th window of a few of its own paired reads."""
    m1, _, _ = feeder_pairs(bam, exclude)
    seqs = [r[2] for r in m1 if 30 <= len(r[2]) <= 200 and set(r[2]) <= set(b"ACGT")][:n_reads]
    return b"".join(s[i:i + K] + b" 9\n" for s in seqs for i in range(0, len(s) - K, 7))


def packed(bam: R.Bam, min_q, exclude=3328):
    """The host packer's filter block of the printed forms of the kept records (rufus_amd.capi.PackedReads)."""
    from rufus_amd import capi
    forms = [stranded_printed(r) for r in bam.kept(exclude)]
    return capi.PackedReads.from_reads([s for s, _ in forms], [q for _, q in forms], min_q, capi.PACK_FILTER)


def record_slices(bam: R.Bam, exclude=3328):
    """The raw bytes of every kept record, block_size field included."""
    ends = bam.starts[1:] + [len(bam.data)]
    return [bam.data[s:e] for r, s, e in zip(bam.records, bam.starts, ends) if not r["flag"] & exclude]


# ---- the crafted file -----------------------------------------------------------------------------------------------
GENOME_LEN, N_SITES = 60_000, 24
EDGE_L = (0, 1, 24, 25, 26, 31, 32, 33, 64, 65)


def _sites():
    return [int(p) for p in np.random.default_rng(6).integers(100, GENOME_LEN - 100, N_SITES)]  # (F.hash_list's own draw)


@functools.lru_cache(maxsize=2)
def crafted(seed=11):
    """(bam bytes, hash list, names of the special pairs).  About 9000 records of mostly 150 bases, 2.5 MB inflated: filler
    pairs of random bases (no hit), a few hundred pairs drawn from a 60 kb genome of which the hash list covers 24 sites,
    and the cases listed in the names."""
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed + 1).integers(0, 4, GENOME_LEN)].tobytes().decode()
    hl = F.hash_list(genome.encode(), N_SITES)
    sites = _sites()
    special = {}

    def q(n, lo=20):
        return bytes(rng.integers(lo, 41, n, dtype=np.uint8))

    def rnd(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))

    def over(site, L=150):  # L bases of the genome that hold the whole 49-base window of a site (L >= 49)
        at = site - 24 - int(rng.integers(0, L - 49 + 1))
        return genome[at:at + L]

    def away(L=150):  # L bases of the genome far from every site
        while True:
            at = int(rng.integers(0, GENOME_LEN - L))
            if all(abs(at + L // 2 - s) > L for s in sites):
                return genome[at:at + L]

    # slots: (position key, record); position keys spread the specials over the file, the filler takes the integers
    slots = []

    def put(at, name, flag, seq, qual="q", **kw):
        qual = q(len(seq)) if qual == "q" else qual
        slots.append((at, dict(name=name, flag=flag, seq=seq, qual=qual, **kw)))

    n_fill = 4000
    for i in range(n_fill):  # filler pairs, mates 1 .. 60 records apart
        a = i * 2 + float(rng.random())
        put(a, b"fill%d" % i, 99, rnd(150 if rng.random() < 0.8 else int(rng.integers(30, 150))))
        put(a + float(rng.integers(1, 60)), b"fill%d" % i, 147, rnd(150))
    for i in range(300):  # pairs from the genome: a share of them overlaps a site
        a = float(rng.uniform(0, 2 * n_fill))
        at = int(rng.integers(0, GENOME_LEN - 500))
        put(a, b"g%d" % i, 99, genome[at:at + 150])
        put(a + float(rng.integers(1, 200)), b"g%d" % i, 147, genome[at + 350:at + 500])
    far = 2 * n_fill * 0.85
    for i in range(3):  # hit record first, mate most of the file later; and the other way round
        put(100.5 + i, b"cross_hit_first%d" % i, 99, over(sites[i]))
        put(far + 100 + i, b"cross_hit_first%d" % i, 147, away())
        put(200.5 + i, b"cross_hit_second%d" % i, 163, away())
        put(far + 200 + i, b"cross_hit_second%d" % i, 83, over(sites[3 + i]))
    # reverse-strand records with IUPAC letters and `=`: the k-mer exists only after the vanished bases close up --
    # 60 bases around a site in pieces of 20 with a letter between them, so no piece holds a 25-mer
    for i, letters in enumerate(("R=", "MY", "KB")):
        s = sites[6 + i]
        g = genome[s - 30:s + 30]
        put(300.5 + i, b"vanish_hit%d" % i, 83, g[:20] + letters[0] + g[20:40] + letters[1] + g[40:], q(62, 30))
        put(310.5 + i, b"vanish_hit%d" % i, 163, away())
        # the same letters in a forward record stay where they are: no hit
        put(320.5 + i, b"iupac_fwd%d" % i, 99, g[:20] + letters[0] + g[20:40] + letters[1] + g[40:], q(62, 30))
        put(330.5 + i, b"iupac_fwd%d" % i, 147, away()[:40] + "SWHVD" + away()[:40])
    put(340.5, b"vanish_in_hit", 83, over(sites[9])[:149] + "R")  # a hit read that also loses a base
    put(341.5, b"vanish_in_hit", 163, away())
    # no qualities (0xFF ...): `*`, bad from the second base on -- over a site, and as the mate of a hit
    put(400.5, b"noqual_over_site", 99, over(sites[10]), None)
    put(401.5, b"noqual_over_site", 147, away(), None)
    put(402.5, b"noqual_mate_of_hit", 99, over(sites[11]))
    put(403.5, b"noqual_mate_of_hit", 147, away(), None)
    # the edge lengths, forward and reverse, over a site where they are long enough for a window
    for j, L in enumerate(EDGE_L):
        s = sites[12 + j % 4]
        seq = genome[s - 12:s - 12 + L]
        put(500.5 + 2 * j, b"edge%d" % L, 99, seq)
        put(501.5 + 2 * j, b"edge%d" % L, 147, away(max(L, 1)))      # (the later record is mate 1: never empty)
        if L:
            put(540.5 + 2 * j, b"edge_rev%d" % L, 99, away(40))
            put(541.5 + 2 * j, b"edge_rev%d" % L, 147, seq)
    put(560.5, b"empty_reverse_alone", 16, "")            # `*` vanishes: a read of 0 bases, which waits for ever
    put(561.5, b"all_vanish_alone", 16, "RYKM=")
    # a name with three records: a pair, and a waiter that is dropped; a hit record without a mate
    for j, a in enumerate((600.5, 650.5, far + 300)):
        put(a, b"three", (99, 147, 99)[j], over(sites[16]) if j == 0 else away())
    put(700.5, b"hit_alone", 0, over(sites[17]))
    # names that are prefixes of one another; a 254-byte name
    for j, nm in enumerate((b"pfx", b"pfx1", b"pfx12")):
        put(800.5 + j, nm, 99, over(sites[18]) if j == 1 else away())
        put(900.5 + 2 - j, nm, 147, away())
    long_name = b"L" * 254
    put(1000.5, long_name, 99, away())
    put(far + 400, long_name, 147, over(sites[19]))
    # a record with an excluded flag between the mates of a hit pair, under their name: it must not pair
    for j, fl in enumerate((256, 1024, 2048)):
        put(1100.5 + 10 * j, b"excl%d" % fl, 99, over(sites[20 + j]))
        put(1102.5 + 10 * j, b"excl%d" % fl, 99 | fl, away())
        put(1104.5 + 10 * j, b"excl%d" % fl, 147, away())
    slots.sort(key=lambda x: x[0])
    n = len(slots)
    recs = []
    for i, (_, r) in enumerate(slots):
        ref = -1 if i >= n - 150 or i % 997 == 5 else min(4, i * 5 // n)  # refID changes; -1 inside the file and at its end
        L = len(r["seq"])
        recs.append(R.record(r["name"], r["flag"], ref, i, [("M", L)] if L else [], r["seq"], r["qual"], b"NMC\x01" if i % 3 else b"",
                             next_ref=ref, next_pos=i, pad_nibble=int(rng.integers(0, 16))))
    special = {"cross": [b"cross_hit_first%d" % i for i in range(3)] + [b"cross_hit_second%d" % i for i in range(3)],
               "vanish": [b"vanish_hit%d" % i for i in range(3)]}
    return R.write(R.REFS, recs, b"@HD\tVN:1.6\tSO:unsorted\n", level=1), hl, special
