"""A pure-Python BAM writer and reader (sections 4.2 and 4.2.4 of the SAM specification) over the BGZF writer of
tests/bgzf_ref.py, and the files of the BAM tests (tests/test_bam_host.py, tests/test_bam_gpu.py,
tests/test_count_bam_gpu.py).  Independent of the product: the reader inflates with zlib and follows block_size with
Python integers.  Not a conftest: the test modules import it."""
import os
import struct
import zlib

import numpy as np

from tests import bgzf_ref as B

SEQ_LETTERS = "=ACMGRSVTWYHKDBN"
NIBBLE = {c: i for i, c in enumerate(SEQ_LETTERS)}
CIGAR_OPS = "MIDNSHP=X"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testRun")


# ---- writer ---------------------------------------------------------------------------------------------------------
def header(refs, text=b""):
    """magic, l_text, text, n_ref, and (l_name, name NUL, l_ref) per reference; refs = [(name bytes, length)]."""
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out.append(struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length))
    return b"".join(out)


def record(name=b"r", flag=0, ref_id=-1, pos=-1, cigar=(), seq="", qual=None, aux=b"", next_ref=-1, next_pos=-1, tlen=0,
           mapq=0, pad_nibble=0, raw_name=None):
    """One alignment record, block_size included.  seq: a string over all 16 letters; pad_nibble: what the unused low nibble
    of an odd-length sequence holds; raw_name: the name field's bytes as they are (its NUL included)."""
    nm = name + b"\0" if raw_name is None else raw_name
    assert 1 <= len(nm) <= 255
    n = [NIBBLE[c] for c in seq]
    if len(n) & 1:
        n.append(pad_nibble)
    packed = bytes(n[i] << 4 | n[i + 1] for i in range(0, len(n), 2))
    q = (b"\xff" * len(seq)) if qual is None else qual
    assert len(q) == len(seq)
    cg = b"".join(struct.pack("<I", ln << 4 | CIGAR_OPS.index(op)) for op, ln in cigar)
    body = (struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), mapq, 4680, len(cigar), flag, len(seq), next_ref, next_pos, tlen) +
            nm + cg + packed + q + aux)
    return struct.pack("<I", len(body)) + body


def write(refs, records, text=b"", cut=B.BLOCK_PAYLOAD, level=6, eof=True):
    """A BAM file: a BGZF block per `cut` inflated bytes, wherever that falls."""
    return B.write(header(refs, text) + b"".join(records), level, cut, eof)


# ---- reader ---------------------------------------------------------------------------------------------------------
def inflate(bam: bytes):
    """(inflated bytes, [inflated offset of every block's first byte])."""
    out, starts, at = [], [], 0
    for blk in B.split(bam):
        _, payload, crc, isize = B.parts(blk)
        data = zlib.decompress(payload, -15)
        assert len(data) == isize and zlib.crc32(data) == crc
        starts.append(at)
        out.append(data)
        at += isize
    return b"".join(out), starts


def read_header(data: bytes):
    """(refs, text, offset of the first record)."""
    assert data[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", data, 4)[0]
    text = data[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", data, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", data, at)[0]
        name = data[at + 4:at + 4 + l_name - 1]
        refs.append((name, struct.unpack_from("<i", data, at + 4 + l_name)[0]))
        at += 8 + l_name
    return refs, text, at


def read_records(data: bytes, at: int):
    """Every record from byte `at`: dicts with start, flag, ref_id, seq (the letters samtools view prints; '*' for none)."""
    recs = []
    while at < len(data):
        bs = struct.unpack_from("<I", data, at)[0]
        assert at + 4 + bs <= len(data), "the file ends inside a record"
        ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", data, at + 4)
        p = at + 36
        name = data[p:p + l_name - 1]
        p += l_name
        cigar = [(CIGAR_OPS[v & 15], v >> 4) for v in struct.unpack_from("<%dI" % n_cig, data, p)]
        p += 4 * n_cig
        sq = data[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(SEQ_LETTERS[sq[i >> 1] >> 4 if not i & 1 else sq[i >> 1] & 15] for i in range(l_seq))
        qual = data[p:p + l_seq]
        recs.append({"start": at, "name": name, "flag": flag, "ref_id": ref_id, "pos": pos, "mapq": mapq, "cigar": cigar,
                     "seq": seq if l_seq else "*", "l_seq": l_seq, "qual": qual, "next_ref": nref, "next_pos": npos, "tlen": tlen})
        at += 4 + bs
    return recs


class Bam:
    """A BAM file as the tests want it: refs, records, where the records start in the inflated stream."""

    def __init__(self, bam: bytes):
        self.bam = bam
        self.data, self.block_starts = inflate(bam)
        self.refs, self.text, self.first = read_header(self.data)
        self.records = read_records(self.data, self.first)
        self.starts = [r["start"] for r in self.records]

    def kept(self, exclude=3328):
        return [r for r in self.records if not r["flag"] & exclude]

    def kept_seqs(self, exclude=3328):
        return [r["seq"].encode() for r in self.kept(exclude)]

    def rname(self, ref_id):
        return b"*" if ref_id < 0 else self.refs[ref_id][0]

    def runs(self, exclude=3328):
        """[(first kept index, refID)] wherever the kept records' refID changes."""
        out = []
        for i, r in enumerate(self.kept(exclude)):
            if not out or out[-1][1] != r["ref_id"]:
                out.append((i, r["ref_id"]))
        return out

    def sam_text(self, exclude=3328):
        """The eleven mandatory fields `samtools view -F exclude` prints per kept record (no aux fields)."""
        lines = []
        for r in self.kept(exclude):
            cg = "".join("%d%s" % (ln, op) for op, ln in r["cigar"]) or "*"
            qual = "*" if not r["l_seq"] or r["qual"][0] == 0xFF else "".join(chr(33 + min(q, 93)) for q in r["qual"])
            rnext = b"*" if r["next_ref"] < 0 else (b"=" if r["next_ref"] == r["ref_id"] else self.rname(r["next_ref"]))
            lines.append(b"\t".join([r["name"], b"%d" % r["flag"], self.rname(r["ref_id"]), b"%d" % (r["pos"] + 1),
                                     b"%d" % r["mapq"], cg.encode(), rnext, b"%d" % (r["next_pos"] + 1), b"%d" % r["tlen"],
                                     r["seq"].encode(), qual.encode()]) + b"\n")
        return b"".join(lines)

    def chr_log(self, exclude=3328):
        """What src/PassThroughSamCheck.cpp:140-155 writes for the kept records: its initial `current`, the previous RNAME
        at every change, the last one at the end."""
        out, current = [], b"notachr"
        for r in self.kept(exclude):
            name = self.rname(r["ref_id"])
            if name != current:
                out.append(current)
                current = name
        out.append(current)
        return b"".join(x + b"\n" for x in out)

    def straddlers(self):
        """Records that begin in one BGZF block and end in another."""
        ends = self.starts[1:] + [len(self.data)]
        bounds = set(self.block_starts[1:])
        return sum(1 for s, e in zip(self.starts, ends) if any(s < b < e for b in bounds))


def fixture(name):
    return open(os.path.join(GOLDEN, name + ".bam"), "rb").read()


# ---- the files ------------------------------------------------------------------------------------------------------
REFS = [(b"chr%d" % i, 1000000 + i) for i in range(1, 6)]
EDGE_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 150, 151, 1500)
EXCLUDED = (256, 512, 1024, 2048, 3072, 3328)


def _seq(rng, n, acgt_only=False):
    letters = "ACGT" if acgt_only else SEQ_LETTERS
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


def synthetic(seed=31, n=700, cut=B.BLOCK_PAYLOAD, level=1):
    """Every shape the pack and the framing branch on: the edge lengths, all 16 nibbles, odd lengths with a nonzero pad
    nibble, names of 1 .. 254 bytes (every start residue mod 4), 0 and 300 cigar ops, aux data, every excluded flag."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        L = EDGE_LENGTHS[i % len(EDGE_LENGTHS)] if i < 4 * len(EDGE_LENGTHS) else int(rng.integers(0, 200))
        seq = SEQ_LETTERS[:L] if i == 5 * len(EDGE_LENGTHS) else _seq(rng, L, acgt_only=rng.random() < 0.5)
        name = bytes(rng.integers(33, 127, 1 + i % 254, dtype=np.uint8)) if i % 3 else b""
        flag = int(rng.choice([0, 16, 99, 147, 4])) | (EXCLUDED[i % len(EXCLUDED)] if i % 7 == 3 else 0)
        cigar = [("M", 1 + j % 9) for j in range(300)] if i % 50 == 7 else ([("M", L)] if L and i % 2 else [])
        aux = b"NMC\x03" + b"RGZgroup%d\0" % i if i % 4 == 1 else b""
        ref = [-1, 0, 0, 1, 1, 1, 4, 2][(i // 40) % 8] if i % 97 else -1
        recs.append(record(name, flag, ref, int(rng.integers(-1, 1000000)), cigar, seq,
                           bytes(rng.integers(0, 42, L, dtype=np.uint8)) if i % 5 else None, aux, next_ref=ref,
                           next_pos=int(rng.integers(-1, 1000000)), pad_nibble=int(rng.integers(1, 16))))
    return write(REFS, recs, b"@HD\tVN:1.6\n", cut, level)


def adversarial(tile=16384, seed=32):
    """Bytes that look like records where none start: a record whose B:C aux array holds the bytes of many well-formed
    records (more than two tiles of them), read names and qualities that hold plausible record headers, and records of more
    than 3 * tile bytes.  Plain records lie between them."""
    rng = np.random.default_rng(seed)

    def plain(i):
        L = int(rng.integers(30, 152))
        return record(b"read%d" % i, int(rng.choice([0, 16, 99, 1024])), int(rng.integers(-1, 5)), int(rng.integers(0, 100000)),
                      [("M", L)], _seq(rng, L, True), bytes(rng.integers(2, 42, L, dtype=np.uint8)), b"NMC\x01")

    fakes = b"".join(plain(1000 + i) for i in range(max(40, 2 * tile // 200 + 40)))
    assert len(fakes) > 2 * tile
    recs = [plain(i) for i in range(30)]
    recs.append(record(b"aux_holds_records", 0, 1, 5, [("M", 50)], _seq(rng, 50, True), None,
                       b"XBBC" + struct.pack("<I", len(fakes)) + fakes))
    recs += [plain(100 + i) for i in range(30)]
    fake_head = plain(2000)[:36]
    for i in range(20):  # a header in the name (raw bytes, NULs and all) and in the qualities
        L = 40 + i
        recs.append(record(flag=0, ref_id=2, pos=7, cigar=[("M", L)], seq=_seq(rng, L, True), qual=(fake_head + bytes(L))[:L],
                           raw_name=fake_head + b"\0"))
        recs.append(plain(200 + i))
    long_len = 2 * (3 * tile + 1000)  # > 3 * tile bytes of sequence alone
    recs.append(record(b"long", 0, 3, 9, [("M", long_len)], _seq(rng, long_len), None))
    recs += [plain(300 + i) for i in range(30)]
    return write(REFS, recs, b"", 40000, 1)
