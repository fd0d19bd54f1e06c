"""The reference side of the `RUFUS.Filter.single --bam` tests (tests/test_filter_single_host.py,
tests/test_bam_gather_hits_gpu.py, tests/test_filter_single_bam_gpu.py): what `samtools view -F N X.bam |
PassThroughSamCheck.stranded.se CHR | RUFUS.Filter.single HashList stdin STUB K MinQ Threshold 1` writes, stated in plain
Python -- every kept record by itself, printed as the stranded feeder prints it (tests/filter_bam_ref.py stranded_printed;
src/PassThroughSamCheck.stranded.se.cpp:172-201 is the paired feeder's switch), scanned by the oracle's single-end scan
(src/RUFUS.Filter.ss.cpp:176-193: the last base IS examined) and written with `:MH<hits>` when the count reaches the
threshold (:194-203), in input order -- and a crafted BAM that holds every case the route branches on.  Independent of the
product.  Not a conftest: the test modules import it."""
import functools

import numpy as np

import oracle
from tests import bam_ref as R
from tests import bgzf_ref as B
from tests import filter_bam_ref as FB

K, MIN_Q = FB.K, FB.MIN_Q
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def single_scan(fs, r, k=K, min_q=MIN_Q, single_end=True) -> int:
    """Windows of a record of bam_ref.read_records, in its printed form, that the oracle's scan finds in the set."""
    seq, qual = FB.stranded_printed(r)
    return fs.scan(seq, qual, k, min_q, single_end=single_end)


def fastq_mh(r, hits) -> bytes:
    seq, qual = FB.stranded_printed(r)
    return b"@" + FB.qname(r) + b":MH%d\n" % hits + seq + b"\n+\n" + qual + b"\n"


def expected_single(bam: R.Bam, hl: bytes, exclude=3328, k=K, min_q=MIN_Q, thresh=1, records=None):
    """(STUB.Mutations.fastq bytes, chromosome log, kept indices of the written records, hit counts of ALL kept records).
    records: the kept records that take part (a region's), default all of them; the log is then theirs."""
    fs = oracle.FilterSet(hl, single_end=True)
    kept = bam.kept(exclude) if records is None else records
    hits = [single_scan(fs, r, k, min_q) for r in kept]
    idx = [i for i, h in enumerate(hits) if h >= thresh]
    log, current = [], b"notachr"
    for r in kept:
        name = bam.rname(r["ref_id"])
        if name != current:
            log.append(current)
            current = name
    log = b"".join(x + b"\n" for x in log + [current])
    return b"".join(fastq_mh(kept[i], hits[i]) for i in idx), log, idx, hits


def expected_single_sam(sam: bytes, hl: bytes, k=K, min_q=MIN_Q, thresh=1):
    """(STUB.Mutations.fastq bytes, chromosome log) of `RUFUS.Filter.single --sam` over SAM text: lines of fewer than eleven
    fields are skipped, a reverse-strand record is reverse-complemented with every base other than A C G T N dropped and
    its quality string reversed whole, a position without a quality character is bad."""
    fs = oracle.FilterSet(hl, single_end=True)
    drop = {ord(c): None for c in set(map(chr, range(256))) - set("ACGTN")}
    out, log, current = [], [], b"notachr"
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if len(f) < 11:
            continue
        if f[2] != current:
            log.append(current)
            current = f[2]
        seq, qual = f[9], f[10]
        if int(f[1]) & 16:
            seq = seq.decode("latin-1").translate(drop).encode().translate(_COMP)[::-1]
            qual = qual[::-1]
        hits = fs.scan(seq, qual, k, min_q, single_end=True)
        if hits >= thresh:
            out.append(b"@" + f[0] + b":MH%d\n" % hits + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out), b"".join(x + b"\n" for x in log + [current])


# ---- the crafted file -----------------------------------------------------------------------------------------------
N_RECORDS, PLANT_LEN, READ_LEN = 4500, 400, 150
EXCLUDED_AT = 200  # the position of the flag-1024 record: behind kept index 65, so positions 0 .. 65 are kept indices


def revcomp(s: str) -> str:
    return s.encode().translate(_COMP)[::-1].decode()


def make_plant(n, seed):
    """(n random bases, the hash list of all their 25-mers as `KMER COUNT` lines)."""
    plant = "".join("ACGT"[i] for i in np.random.default_rng(seed).integers(0, 4, n))
    return plant, b"".join(plant[i:i + K].encode() + b" 9\n" for i in range(n - K + 1))


def random_bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def planted_read(rng, plant, h, L=150, right=None):
    """L bases with exactly h hit windows: 24 + h bases of the plant between random flanks that do not continue it (h = 0:
    random bases).  right: the number of bases behind the plant's stretch (default: random)."""
    if h == 0:
        return random_bases(rng, L)
    n = 24 + h

    def other(c):  # a base that is not c
        return "ACGT"[("ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]

    a = int(rng.integers(1, len(plant) - n))
    right = int(rng.integers(0, L - n + 1)) if right is None else right
    left = L - n - right
    assert left >= 0 and right >= 0
    lf, rt = random_bases(rng, left), random_bases(rng, right)
    if left:
        lf = lf[:-1] + other(plant[a - 1])
    if right:
        rt = other(plant[a + n]) + rt[1:]
    return lf + plant[a:a + n] + rt


def planted_records(n, planted, plant, seed=23, L=60):
    """n raw BAM records (all kept; every third on the reverse strand; names of 2 .. 5 bytes) of L bases: exactly those at
    the indices `planted` hold hit windows, 1 and 3 of them alternating, the others random bases."""
    rng = np.random.default_rng(seed)
    planted, out, nth = set(planted), [], 0
    for i in range(n):
        h = 0
        if i in planted:
            h = 1 if nth % 2 == 0 else 3
            nth += 1
        printed = planted_read(rng, plant, h, L)
        rev = i % 3 == 1
        out.append(R.record(b"s%d" % i, 16 if rev else 0, i % 3, i, [("M", L)], revcomp(printed) if rev else printed,
                            bytes(rng.integers(20, 41, L, dtype=np.uint8)), b"NMC\x01" if i % 2 else b""))
    return out


@functools.lru_cache(maxsize=2)
def crafted_single(seed=17):
    """(bam bytes, hash list, {case name: QNAME}).  N_RECORDS records of mostly 150 bases (about 276 bytes each: 1.2 MB
    inflated, so arenas of 1 MiB cut it): reads of random bases (no hit), and reads that hold a stretch of the PLANT -- 400
    random bases all of whose 25-mers are the hash list -- flanked by bases that do not continue it, so a read's number of
    hit windows is known by construction.  The cases are listed in the names."""
    rng = np.random.default_rng(seed)
    plant, hl = make_plant(PLANT_LEN, seed + 1)

    def rnd(n):
        return random_bases(rng, n)

    def other(c):  # a base that is not c
        return "ACGT"[("ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]

    def hit_read(h, L=READ_LEN, right=None):
        return planted_read(rng, plant, h, L, right)

    def q(n, lo=20):
        return bytes(rng.integers(lo, 41, n, dtype=np.uint8))

    # position -> record spec; the filler: a read of random bases or (15 %) a read with a few hit windows, either strand
    specs = []
    for i in range(N_RECORDS):
        L = READ_LEN if rng.random() < 0.9 else int(rng.integers(30, READ_LEN))
        hit = rng.random() < 0.15
        h = int(rng.choice([1, 1, 2, 3, 5])) if hit else 0
        printed = hit_read(h, L) if hit else rnd(L)
        rev = rng.random() < 0.5
        specs.append(dict(name=b"r%d" % i, flag=16 if rev else 0, seq=revcomp(printed) if rev else printed, qual=q(L)))
    special = {}

    def put(at, case, seq, flag=0, qual="q", name=None):
        nm = name if name is not None else case.encode()
        specs[at] = dict(name=nm, flag=flag, seq=seq, qual=q(len(seq)) if qual == "q" else qual)
        special[case] = nm

    # selected records at kept indices 0, 63, 64, 65 and the last
    for at in (0, 63, 64, 65, N_RECORDS - 1):
        put(at, "at%d" % at, hit_read(3))
    # a forward read whose only hit window ends at its LAST base: the paired scan never examines that base
    put(70, "last_base", hit_read(1, right=0))
    # a reverse-strand read that hits only after its vanished IUPAC bases have closed up: the printed read holds 30 bases of
    # the plant (6 windows); the stored read has a letter after every 10 of them, so no stored 25-mer is the plant's
    a = int(rng.integers(1, PLANT_LEN - 31))
    lf, rt = rnd(59) + other(plant[a - 1]), other(plant[a + 30]) + rnd(59)
    core = revcomp(plant[a:a + 30])
    stored = revcomp(rt) + "".join(core[j:j + 10] + "RYK"[j // 10] for j in range(0, 30, 10)) + revcomp(lf)
    put(71, "vanish_hit", stored, flag=16)
    put(72, "iupac_fwd", stored, flag=0)  # in a forward record the letters stay where they are: no hit
    # exactly 1, exactly 2, 10 .. 99 and >= 100 hit windows: `:MH` with one, two and three digits
    put(73, "hits1", hit_read(1))
    put(74, "hits2", hit_read(2))
    put(75, "hits40", hit_read(40))
    put(76, "hits126", plant[50:50 + READ_LEN])  # wholly inside the plant: 126 windows
    put(77, "hits126_rev", revcomp(plant[100:100 + READ_LEN]), flag=16)
    # a hit window spoiled by one base below MinQ, and one spoiled by an N
    s = hit_read(1, right=40)
    ql = bytearray(q(READ_LEN))
    ql[READ_LEN - 40 - 12] = MIN_Q - 1
    put(78, "low_q_spoils", s, qual=bytes(ql))
    at_n = READ_LEN - 40 - 12
    put(79, "n_spoils", s[:at_n] + "N" + s[at_n + 1:])
    # `*`, forward and reverse; no qualities (0xFF) over bases that would hit; an excluded flag over bases that would hit
    put(80, "star_fwd", "", flag=0)
    put(81, "star_rev", "", flag=16)
    put(82, "noqual_would_hit", hit_read(5), qual=None)
    put(EXCLUDED_AT, "excluded_would_hit", hit_read(5), flag=1024)
    # two records of one QNAME that both hit: both are written, unpaired
    put(83, "twin_a", hit_read(2), flag=99, name=b"twin")
    put(90, "twin_b", hit_read(4), flag=147, name=b"twin")
    # a selected record right where the refID changes, and one that straddles every BGZF block boundary (an arena is cut at
    # one of them, whichever way the arenas are filled): same name and length as the record it replaces, so nothing moves
    n = N_RECORDS

    def ref_of(i):
        return -1 if i >= n - 100 else min(4, i * 5 // n)

    changes = [i for i in range(1, n) if ref_of(i) != ref_of(i - 1)]
    for i in changes:
        put(i, "ref_change%d" % i, hit_read(2, len(specs[i]["seq"])), name=specs[i]["name"])

    def size(sp, i):
        L = len(sp["seq"])
        return 36 + len(sp["name"]) + 1 + (4 if L else 0) + (L + 1) // 2 + L + (4 if i % 3 else 0)

    text = b"@HD\tVN:1.6\tSO:unsorted\n"
    at, starts = len(R.header(R.REFS, text)), []
    for i, sp in enumerate(specs):
        starts.append(at)
        at += size(sp, i)
    total = at
    straddle = []
    for i, sp in enumerate(specs):
        lo, hi = starts[i], starts[i] + size(sp, i)
        if lo // B.BLOCK_PAYLOAD != (hi - 1) // B.BLOCK_PAYLOAD and sp["name"] == b"r%d" % i and len(sp["seq"]) >= 60:
            put(i, "straddle%d" % i, hit_read(3, len(sp["seq"])), flag=sp["flag"] & ~16, name=sp["name"])
            straddle.append(i)
    recs = []
    for i, sp in enumerate(specs):
        L = len(sp["seq"])
        rec = R.record(sp["name"], sp["flag"], ref_of(i), i, [("M", L)] if L else [], sp["seq"], sp["qual"], b"NMC\x01" if i % 3 else b"",
                       next_ref=-1, next_pos=-1, pad_nibble=int(rng.integers(0, 16)))
        assert len(rec) == size(sp, i)
        recs.append(rec)
    special["_straddle"] = straddle
    special["_ref_changes"] = changes
    special["_starts"] = starts
    assert total > (1 << 20)
    return R.write(R.REFS, recs, text, level=1), hl, special


def clean_subset(bam: R.Bam, exclude=3328):
    """The kept records the text route and the reference tools accept: bases and qualities present, and the printed read
    not empty.  As a BAM file of its own."""
    recs = [bam.data[r["start"]:e] for r, e in zip(bam.records, bam.starts[1:] + [len(bam.data)])
            if not r["flag"] & exclude and r["l_seq"] and r["qual"][0] != 0xFF and FB.stranded_printed(r)[0]]
    return R.write(bam.refs, recs, bam.text, level=1)
