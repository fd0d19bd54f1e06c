"""A pure-Python BAM index (sections 5.2 and 5.3 of the SAM specification) over tests/bam_ref.py: the binning scheme, a
record's end and the region test of `samtools view X.bam REGION`, a BAI WRITER over bam_ref's block starts in two
granularities and both spellings of "end of block", and a reader with the one-range query of rfx_bai.hpp.  Independent
of the product: Python integers and struct.  Not a conftest and not a test: the region tests import it."""
import bisect
import struct

from tests import bgzf_ref as B

MAX_POS = 1 << 29
META_BIN = 37450
REF_OPS = "MDN=X"  # the operations that consume the reference


# ---- the binning scheme ---------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    beg, end = max(beg, 0), min(end, MAX_POS)
    if beg >= end:
        return []
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(first + (beg >> shift), first + (end >> shift) + 1)
    return bins


# ---- a record's extent ------------------------------------------------------------------------------------------------
def end_pos(rec):
    """pos + rlen; rlen = 1 for flag 4, no CIGAR operation or none that consumes the reference."""
    rlen = 0 if rec["flag"] & 4 else sum(ln for op, ln in rec["cigar"] if op in REF_OPS)
    return rec["pos"] + (rlen or 1)


def in_region(rec, tid, beg, end):
    return rec["ref_id"] == tid and rec["pos"] < end and end_pos(rec) > beg


def parse_region(text, names):
    """(tid, beg, end) or None for a text that is refused; names: the header's (bytes)."""
    names = [n.decode() for n in names]
    if text in names:
        return names.index(text), 0, MAX_POS
    name, colon, rest = text.rpartition(":")
    if not colon or name not in names:
        return None
    lo, dash, hi = rest.partition("-")
    lo, hi = lo.replace(",", ""), hi.replace(",", "")
    if not lo.isdigit() or (dash and not hi.isdigit()) or not lo.isascii() or not hi.isascii() or max(len(lo), len(hi)) > 18:
        return None
    beg, end = int(lo), int(hi) if dash else MAX_POS
    if beg < 1 or end < beg:
        return None
    return names.index(name), beg - 1, end


# ---- writer -----------------------------------------------------------------------------------------------------------
class _Voff:
    """Inflated offsets of a bam_ref.Bam as virtual offsets."""

    def __init__(self, bam):
        self.starts = bam.block_starts
        blocks = B.split(bam.bam)
        self.coff, at = [], 0
        for blk in blocks:
            self.coff.append(at)
            at += len(blk)
        self.isize = [B.parts(blk)[3] for blk in blocks]

    def start(self, x):
        """Offset x as the START of a record (a byte of data lies there, so the last block that begins at or in front of it
        holds it)."""
        i = bisect.bisect_right(self.starts, x) - 1
        assert x - self.starts[i] < self.isize[i]
        return self.coff[i] << 16 | (x - self.starts[i])

    def end(self, y, spelling):
        """Offset y as the END of a record: where y is a block's first byte it is also the end of the block in front."""
        i = bisect.bisect_right(self.starts, y) - 1
        if y == self.starts[i] and spelling == "same":
            j = i - 1
            while j > 0 and self.isize[j] == 0:
                j -= 1
            if j >= 0 and self.isize[j]:
                return self.coff[j] << 16 | self.isize[j]
        return self.coff[i] << 16 | (y - self.starts[i])


def build(bam, kind="fine", spelling="next", n_no_coor=True):
    """The .bai of a bam_ref.Bam.  kind "fine": a chunk per run of consecutive records of one bin (and the pseudo-bin), the
    linear index with its empty windows filled from the right; "coarse": every record of a reference in ONE chunk of bin 0
    and a linear index of that one offset.  spelling "next" / "same": a chunk that ends with a block ends at (next block, 0)
    or at (that block, its inflated size)."""
    v = _Voff(bam)
    ends = bam.starts[1:] + [len(bam.data)]
    out = [b"BAI\x01", struct.pack("<i", len(bam.refs))]
    for tid in range(len(bam.refs)):
        mine = [(r, e) for r, e in zip(bam.records, ends) if r["ref_id"] == tid]
        if not mine:
            out.append(struct.pack("<ii", 0, 0))
            continue
        bins, linear = {}, {}
        if kind == "coarse":
            bins[0] = [(v.start(mine[0][0]["start"]), v.end(max(e for _, e in mine), spelling))]
            linear[0] = bins[0][0][0]
        else:
            run = None  # [bin, first start, last end]
            for r, e in list(zip(bam.records, ends)) + [(None, None)]:
                b = reg2bin(r["pos"], end_pos(r)) if r is not None and r["ref_id"] == tid else None
                if run and b != run[0]:
                    bins.setdefault(run[0], []).append((v.start(run[1]), v.end(run[2], spelling)))
                    run = None
                if b is not None:
                    run = [b, r["start"], e] if run is None else [b, run[1], e]
            for r, _ in mine:
                for w in range(max(r["pos"], 0) >> 14, ((end_pos(r) - 1) >> 14) + 1):
                    linear[w] = min(linear.get(w, 1 << 64), v.start(r["start"]))
            mapped = sum(1 for r, _ in mine if not r["flag"] & 4)
            bins[META_BIN] = [(v.start(mine[0][0]["start"]), v.end(mine[-1][1], spelling)), (mapped, len(mine) - mapped)]
        out.append(struct.pack("<i", len(bins)))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
        n_intv = max(linear) + 1
        ioff, nxt = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):
            nxt = linear.get(w, nxt)
            ioff[w] = nxt
        out.append(struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *ioff))
    if n_no_coor:
        out.append(struct.pack("<Q", sum(1 for r in bam.records if r["ref_id"] < 0)))
    return b"".join(out)


# ---- reader and query -------------------------------------------------------------------------------------------------
def parse(bai):
    """[(bins {bin: [(beg, end)]} without the pseudo-bin, ioffset list)] per reference."""
    assert bai[:4] == b"BAI\x01"
    n_ref, at, refs = struct.unpack_from("<i", bai, 4)[0], 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, at)[0]
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", bai, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b != META_BIN:
                bins[b] = chunks
        n_intv = struct.unpack_from("<i", bai, at)[0]
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, bai, at + 4))))
        at += 4 + 8 * n_intv
    assert len(bai) - at in (0, 8)
    return refs


def query(index, tid, beg, end):
    """None (no chunk), or (START, STOP): START = the smallest max(chunk.beg, min_off), STOP = the largest chunk.end over the
    chunks of reg2bins(beg, end) with chunk.end > min_off = ioffset[min(beg >> 14, n_intv - 1)] (0 without a linear index)."""
    bins, ioff = index[tid]
    min_off = ioff[min(beg >> 14, len(ioff) - 1)] if ioff else 0
    chunks = [(max(b, min_off), e) for k in reg2bins(beg, end) for b, e in bins.get(k, ()) if e > min_off]
    if not chunks:
        return None
    return min(b for b, _ in chunks), max(e for _, e in chunks)


def blocks_between(bam, start, stop):
    """The BGZF blocks a walk from START's block to STOP's inflates: STOP's own only where STOP lies inside it."""
    v = _Voff(bam)
    last = (stop >> 16) if stop & 0xFFFF else (stop >> 16) - 1
    return sum(1 for c in v.coff if (start >> 16) <= c <= last)


# ---- the sorted file of the index tests -------------------------------------------------------------------------------
def sorted_bam(seed=51, n=6000, cut=4096):
    """About n records of 100 bases over three references, sorted by (refID, pos), hundreds of BGZF blocks; among them
    unmapped records placed at their mate's position, records with deletions, soft clips and long N operations, some
    excluded flags, refID -1 records at the end, and records that end exactly with their block (every 97th, and the last of
    every reference)."""
    import numpy as np

    from tests import bam_ref as R
    rng = np.random.default_rng(seed)
    refs = [(b"chrA", 3_000_000), (b"chrB:1", 2_000_000), (b"chrC", 40_000)]
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    recs, at = [], len(R.header(refs, text))

    def add(aligned, name, *rest):
        """aligned: an aux string pads the record so that it ENDS with a BGZF block (both spellings of that offset exist)."""
        nonlocal at
        rec = R.record(name, *rest, b"NMC\x01")
        if aligned:
            need = -(at + len(rec)) % cut
            need += cut if need < 5 else 0
            rec = R.record(name, *rest, b"NMC\x01XPZ" + b"p" * (need - 4) + b"\0")
            assert (at + len(rec)) % cut == 0
        recs.append(rec)
        at += len(rec)

    for tid, (_, length) in enumerate(refs):
        places = sorted(int(p) for p in rng.integers(0, length - 200, n // 3))
        for j, pos in enumerate(places):
            kind = int(rng.integers(0, 20))
            flag = int(rng.choice([0, 16, 99, 147])) | (1024 if kind == 7 else 0)
            cigar = [("M", 100)]
            if kind == 1:
                cigar = [("M", 40), ("D", int(rng.integers(1, 50))), ("M", 60)]
            elif kind == 2:
                cigar = [("S", 20), ("M", 80)]
            elif kind == 3:
                cigar = [("M", 50), ("N", int(rng.integers(1000, 40000))), ("M", 50)]
            elif kind == 4:
                flag, cigar = 4 | 1 | 64, []  # unmapped, placed at the mate's position
            add(j % 97 == 50 or j == len(places) - 1, b"s%d_%d" % (tid, len(recs)), flag, tid, pos, cigar, R._seq(rng, 100, True),
                bytes(rng.integers(2, 42, 100, dtype=np.uint8)))
    for i in range(40):
        add(i == 39, b"u%d" % i, 4, -1, -1, [], R._seq(rng, 100, True), bytes(rng.integers(2, 42, 100, dtype=np.uint8)))
    return R.write(refs, recs, text, cut, 1)


# ---- the record table of the region tests ---------------------------------------------------------------------------
TABLE_REFS = [(b"chr1", 1 << 29), (b"chr2", (1 << 31) - 1), (b"chr3", 1000)]
# (tid, beg, end): an ordinary window, and one whose answers differ between 32-bit and 64-bit arithmetic
TABLE_REGIONS = [(1, 100_000, 100_500), (1, (1 << 31) + 5, (1 << 31) + 10)]
BIG = (1 << 28) - 1  # the longest CIGAR operation


def region_table(n, seed=61):
    """n raw records (bam_ref.record) for TABLE_REGIONS[0] = chr2:[BEG, END): first the shapes the region test branches on --
    every CIGAR shape, flag 4 with a CIGAR, the exact boundaries, the other references, 64-bit sums -- then, 25 and more on
    each side of each boundary, then random records around the window."""
    import numpy as np

    from tests import bam_ref as R
    rng = np.random.default_rng(seed)
    tid, beg, end = TABLE_REGIONS[0]
    shapes = [
        (tid, beg + 10, []),                                            # 0 operations: rlen 1
        (tid, beg - 1, []),                                             # ... endpos == BEG: out
        (tid, beg, []),                                                 # ... endpos == BEG + 1: in
        (tid, beg - 30, [("M", 30)]),                                   # 1 operation, endpos == BEG: out
        (tid, beg - 30, [("M", 31)]),                                   # endpos == BEG + 1: in
        (tid, end - 1, [("M", 30)]),                                    # pos == END - 1: in
        (tid, end, [("M", 30)]),                                        # pos == END: out
        (tid, beg - 1500, [("M", 1 + j % 9) for j in range(300)]),      # 300 operations: rlen 1497, out
        (tid, beg - 1496, [("M", 1 + j % 9) for j in range(300)]),      # ... in by one base
        (tid, beg - 40, [(op, 10) for op in R.CIGAR_OPS]),              # all nine kinds: rlen 50 (M D N = X), in
        (tid, beg - 50, [(op, 10) for op in R.CIGAR_OPS]),              # ... endpos == BEG: out
        (tid, beg - 1, [("I", 20), ("S", 20)]),                         # only I / S: rlen 0 -> 1, endpos == BEG: out
        (tid, beg, [("S", 20), ("I", 20)]),                             # ... in
        (tid, 5, [("S", 10), ("N", beg)]),                              # S, N with a long N: endpos = 5 + BEG, in
        (tid, 5, [("S", 10), ("N", beg - 5)]),                          # ... endpos == BEG: out
        (0, beg + 10, [("M", 30)]),                                     # another reference
        (2, 10, [("M", 30)]),
        (-1, -1, []),                                                   # refID -1
        (-1, beg + 10, [("M", 30)]),
        (tid, (1 << 31) - 50, [("M", 100)]),                            # pos + rlen above 2^31 (in TABLE_REGIONS[1] only)
        (tid, 10, [("N", BIG)] * 16 + [("M", 16)]),                     # rlen == 2^32: in; a 32-bit sum is 0 -> 1: out
    ]
    recs = []
    for i, (ref, pos, cigar) in enumerate(shapes):
        recs.append((ref, pos, cigar, 0))
    recs.append((tid, beg - 1, [("M", 30)], 4))                         # flag 4 with a CIGAR: endpos = pos + 1 == BEG: out
    recs.append((tid, beg, [("M", 30)], 4))                             # ... in
    recs.append((tid, beg + 5, [("M", 30)], 1024))                      # in the region, excluded by its flag
    for j in range(26):                                                 # each side of each boundary
        recs.append((tid, beg - 40 - j, [("M", 40)], 0))                # endpos <= BEG: out
        recs.append((tid, beg - 40 - j, [("M", 41 + j)], 0))            # endpos > BEG: in
        recs.append((tid, end - 1 - j, [("M", 40)], 0))                 # pos < END: in
        recs.append((tid, end + j, [("M", 40)], 0))                     # pos >= END: out
    while len(recs) < n:
        L = int(rng.integers(20, 41))
        cigar = [("M", L)] if rng.random() < 0.7 else [("M", L // 2), ("D", int(rng.integers(1, 200))), ("M", L - L // 2)]
        recs.append((int(rng.choice([tid, tid, tid, 0, -1])), int(rng.integers(beg - 400, end + 400)), cigar,
                     int(rng.choice([0, 16, 99, 147, 4, 1024, 2048]))))
    out = []
    for i, (ref, pos, cigar, flag) in enumerate(recs[:n]):
        L = 20 + i % 21
        out.append(R.record(b"n" * (i % 4) + b"%d" % i, flag, ref, pos, cigar, R._seq(rng, L, i % 3 != 0),
                            bytes(rng.integers(2, 42, L, dtype=np.uint8)), b"NMC\x01" if i % 2 else b""))
    return out
