"""A pure-Python BGZF writer and the corpus of the BGZF decoder's tests (tests/test_bgzf_host.py, tests/test_bgzf_gpu.py).

BGZF (the SAM specification's section on it): gzip members (RFC 1952) of at most 64 KiB, each with its own size in a `BC`
extra subfield and a raw deflate stream (RFC 1951) as its payload.  The writer here frames what ``zlib.compressobj``
emits; the hand-assembled streams come from the small bit writer below, with ``zlib.decompress(x, -15)`` as their oracle.
Not a conftest: the test modules import it.
"""
import struct
import zlib

import numpy as np

BLOCK_PAYLOAD = 65280  # what bgzip puts into one block


def frame(payload: bytes, crc: int, isize: int, extra_before: bytes = b"") -> bytes:
    """One BGZF block around a raw deflate stream."""
    extra = extra_before + b"BC\x02\x00"
    total = 12 + len(extra) + 2 + len(payload) + 8
    assert total <= 65536, total
    extra += struct.pack("<H", total - 1)
    return (b"\x1f\x8b\x08\x04" + b"\x00\x00\x00\x00" + b"\x00\xff" + struct.pack("<H", len(extra)) + extra + payload +
            struct.pack("<II", crc & 0xFFFFFFFF, isize))


def deflate(data: bytes, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def block(data: bytes, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, extra_before=b"", raw=None) -> bytes:
    """`data` as one BGZF block (raw: a deflate stream made elsewhere that inflates to `data`)."""
    assert len(data) <= 65536
    return frame(deflate(data, level, mem_level, strategy) if raw is None else raw, zlib.crc32(data), len(data), extra_before)


EOF = block(b"")
assert len(EOF) == 28


def write(data: bytes, level=6, cut=BLOCK_PAYLOAD, eof=True) -> bytes:
    """`data` as a BGZF file: a block per `cut` bytes and the EOF marker."""
    out = [block(data[i:i + cut], level) for i in range(0, len(data), cut)]
    return b"".join(out) + (EOF if eof else b"")


def split(bgzf: bytes):
    """The blocks of a BGZF byte string (BC first, as this writer frames them)."""
    out, at = [], 0
    while at < len(bgzf):
        xlen = struct.unpack_from("<H", bgzf, at + 10)[0]
        ex, bs = bgzf[at + 12:at + 12 + xlen], None
        i = 0
        while i < xlen:
            slen = struct.unpack_from("<H", ex, i + 2)[0]
            if ex[i:i + 2] == b"BC":
                bs = struct.unpack_from("<H", ex, i + 4)[0] + 1
            i += 4 + slen
        out.append(bgzf[at:at + bs])
        at += bs
    return out


def parts(blk: bytes):
    """(header, payload, crc, isize) of one block."""
    xlen = struct.unpack_from("<H", blk, 10)[0]
    crc, isize = struct.unpack_from("<II", blk, len(blk) - 8)
    return blk[:12 + xlen], blk[12 + xlen:-8], crc, isize


def reframe(blk: bytes, payload=None, crc=None, isize=None) -> bytes:
    """The block with another payload / CRC / ISIZE and BSIZE put right."""
    _, p, c, n = parts(blk)
    return frame(p if payload is None else payload, c if crc is None else crc, n if isize is None else isize)


# ---- a bit writer for the streams zlib never writes --------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):  # header fields and extra bits: least significant bit first
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code_len):  # a Huffman code: most significant bit first
        code, length = code_len
        for i in range(length - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


def canon(lengths: dict):
    """symbol -> (code, length) of the canonical Huffman code with these lengths (RFC 1951 3.2.2)."""
    code, out = 0, {}
    for length in range(1, 16):
        for sym in sorted(s for s, n in lengths.items() if n == length):
            out[sym] = (code, length)
            code += 1
        code <<= 1
    return out


FIXED_LIT = canon({**{s: 8 for s in range(144)}, **{s: 9 for s in range(144, 256)}, **{s: 7 for s in range(256, 280)},
                   **{s: 8 for s in range(280, 288)}})
FIXED_DIST = canon({s: 5 for s in range(32)})
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(w: Bits, final, hlit, hdist, clc_lens: dict, cl_seq, n_clc=None):
    """BFINAL, BTYPE = 2, the three counts, the code-length code's lengths and the code-length symbols `cl_seq`:
    (symbol, extra value) with 2 / 3 / 7 extra bits for 16 / 17 / 18."""
    w.put(final, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    if n_clc is None:
        n_clc = max(4, 1 + max(CL_ORDER.index(s) for s in clc_lens))
    w.put(n_clc - 4, 4)
    for s in CL_ORDER[:n_clc]:
        w.put(clc_lens.get(s, 0), 3)
    codes = canon(clc_lens)
    for sym, extra in cl_seq:
        w.code(codes[sym])
        if sym >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[sym])


_LIT4 = canon({65: 2, 67: 2, 256: 2, 257: 2})  # 'A', 'C', end of block, length 3


def hand_far_match(rng):
    """(a) a stored block of 32768 bytes, then a fixed block with a match of length 258 at distance 32768."""
    data = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = Bits()
    w.put(0, 1), w.put(0, 2), w.align()
    w.put(32768, 16), w.put(32768 ^ 0xFFFF, 16), w.raw(data)
    w.put(1, 1), w.put(1, 2)
    w.code(FIXED_LIT[285])                       # length 258
    w.code(FIXED_DIST[29]), w.put(32768 - 24577, 13)  # distance 24577 + 8191
    w.code(FIXED_LIT[256])
    return data + data[:258], w.bytes()


def hand_run_across(final=1):
    """(b) a dynamic block whose repeat code 16 runs from the last literal/length length into the distance lengths."""
    w = Bits()
    # lengths: 65 zeros, 2 ('A'), 0, 2 ('C'), 188 zeros, 2 (256), then 16 x 5: symbol 257 and the four distance codes
    dynamic_header(w, final, 258, 4, {0: 2, 2: 2, 16: 2, 18: 2},
                   [(18, 65 - 11), (2, 0), (0, 0), (2, 0), (18, 138 - 11), (18, 50 - 11), (2, 0), (16, 5 - 3)])
    dist = canon({0: 2, 1: 2, 2: 2, 3: 2})
    for s in (65, 67, 65, 67):
        w.code(_LIT4[s])
    w.code(_LIT4[257]), w.code(dist[1])  # length 3, distance 2
    w.code(_LIT4[256])
    return b"ACACACA", w.bytes()


def hand_one_dist_code():
    """(c) a dynamic block with one distance code, of length 1 (RFC 1951: "one distance code of zero bits ... one bit")."""
    w = Bits()
    dynamic_header(w, 1, 258, 1, {0: 2, 1: 2, 2: 2, 18: 2},
                   [(18, 65 - 11), (2, 0), (0, 0), (2, 0), (18, 138 - 11), (18, 50 - 11), (2, 0), (2, 0), (1, 0)])
    w.code(_LIT4[65])
    w.code(_LIT4[257]), w.code((0, 1))  # length 3, the one distance code: distance 1
    w.code(_LIT4[67])
    w.code(_LIT4[256])
    return b"AAAAC", w.bytes()


# ---- the corpus -------------------------------------------------------------------------------------------------------
def fastq_text(rng, n_records, read_len=150, genome_len=6000):
    """Strict 4-line FASTQ of reads drawn from a small genome (so sequence lines repeat at every distance)."""
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, genome_len)]
    out = []
    for i in range(n_records):
        at = int(rng.integers(0, genome_len - read_len))
        q = (33 + np.minimum(rng.geometric(0.15, read_len), 41)).astype(np.uint8)
        out.append(b"@read%d/1\n" % i + genome[at:at + read_len].tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    return b"".join(out)


def fibonacci_bytes(rng, n_symbols=21):
    fib = [1, 1]
    while len(fib) < n_symbols:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, 40 + i, np.uint8) for i, f in enumerate(fib)])
    rng.shuffle(data)
    return data.tobytes()


PERIODS = (2, 3, 63, 64, 65, 127, 128, 129)


def corpus():
    """[(name, original bytes, the BGZF block)] -- every shape at which the decoder branches, one block each."""
    rng = np.random.default_rng(20)
    fq = fastq_text(rng, 220)[:BLOCK_PAYLOAD]
    assert len(fq) == BLOCK_PAYLOAD
    out = [("fastq_l6", fq, block(fq, 6)),
           ("fastq_l1", fq, block(fq, 1)),
           ("fastq_l9_mem1", fq, block(fq, 9, mem_level=1)),
           ("fastq_fixed", fq, block(fq, 6, strategy=zlib.Z_FIXED)),
           ("fastq_l0", fq[:60000], block(fq[:60000], 0)),
           ("all_A", b"A" * BLOCK_PAYLOAD, block(b"A" * BLOCK_PAYLOAD))]
    for p in PERIODS:
        unit = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, p)].tobytes()
        data = (unit * (4000 // p + 1))[:4000]
        out.append(("period_%d" % p, data, block(data)))
    fib = fibonacci_bytes(rng)
    assert len(fib) == 28656
    out.append(("fibonacci", fib, block(fib, 6, strategy=zlib.Z_HUFFMAN_ONLY)))
    out.append(("empty", b"", EOF))
    out.append(("one_byte", b"x", block(b"x")))
    # ISIZE 65536, the format's limit (bgzip stops at 65280).  Stored, 65536 bytes do not fit a block (BSIZE is 16 bits):
    # text that deflates does.
    big = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 65536)].tobytes()
    out.append(("isize_65536", big, block(big, 1)))
    for name, (data, raw) in (("hand_far_match", hand_far_match(rng)), ("hand_run_across", hand_run_across()),
                              ("hand_one_dist_code", hand_one_dist_code())):
        assert zlib.decompress(raw, -15) == data, name  # zlib accepts what the bit writer made
        out.append((name, data, block(data, raw=raw)))
    return out


def big_file(n_blocks=300, text_bytes=5 << 20):
    """(original bytes, [blocks]) of about n_blocks blocks in shuffled order: FASTQ text at levels 1 / 6 / 9, the corpus
    blocks over and over, EOF markers in the middle and one at the end."""
    rng = np.random.default_rng(21)
    text = fastq_text(rng, text_bytes // 330)
    items = [(text[i:i + BLOCK_PAYLOAD], block(text[i:i + BLOCK_PAYLOAD], (1, 6, 9)[(i // BLOCK_PAYLOAD) % 3]))
             for i in range(0, len(text), BLOCK_PAYLOAD)]
    small = [(d, b) for _, d, b in corpus()]
    i = 0
    while len(items) < n_blocks - 1:
        items.append(small[i % len(small)])
        i += 1
    order = rng.permutation(len(items))
    items = [items[j] for j in order] + [(b"", EOF)]
    return b"".join(d for d, _ in items), [b for _, b in items]


# ---- the corrupt set ------------------------------------------------------------------------------------------------------
def _fixed(tokens, final=1):
    w = Bits()
    w.put(final, 1), w.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple) and t[0] == "raw":
            w.code(t[1])
        else:
            w.code(FIXED_LIT[t])
    return w.bytes()


def refusals():
    """[(name, status the core must give, block)]: one mutation per refusal of rfx_bgzf_core.h (the numbers are its
    bgzf_status)."""
    good = block(b"ACGTACGTAACCGGTT" * 40)
    _, pay, crc, isize = parts(good)
    out = []

    def raw(name, status, payload, n=7):
        out.append((name, status, frame(payload, 0, n)))

    w = Bits()
    w.put(1, 1), w.put(3, 2)
    raw("block_type_3", 1, w.bytes())
    w = Bits()
    w.put(1, 1), w.put(0, 2), w.align(), w.put(4, 16), w.put(4, 16), w.raw(b"abcd")
    raw("stored_len", 2, w.bytes(), 4)
    for name, hlit, hdist in (("hlit_287", 287, 4), ("hdist_31", 258, 31)):
        w = Bits()
        dynamic_header(w, 1, hlit, hdist, {0: 2, 2: 2, 16: 2, 18: 2}, [])
        raw(name, 3, w.bytes() + b"\x00" * 8)
    w = Bits()
    dynamic_header(w, 1, 258, 4, {0: 1, 2: 1, 18: 1}, [], n_clc=16)
    raw("oversubscribed", 4, w.bytes() + b"\x00" * 8)
    w = Bits()
    dynamic_header(w, 1, 258, 4, {0: 2, 18: 2}, [], n_clc=16)
    raw("incomplete", 5, w.bytes() + b"\x00" * 8)
    w = Bits()  # one code of one bit is an incomplete code too where it is the code-length code (zlib refuses it as well)
    dynamic_header(w, 1, 258, 4, {0: 1}, [], n_clc=16)
    raw("incomplete_single_code_length_code", 5, w.bytes() + b"\x00" * 8)
    w = Bits()
    dynamic_header(w, 1, 258, 4, {0: 2, 2: 2, 16: 2, 18: 2}, [(16, 0)])
    raw("repeat_no_previous", 6, w.bytes() + b"\x00" * 8)
    w = Bits()
    dynamic_header(w, 1, 258, 4, {0: 2, 2: 2, 16: 2, 18: 2}, [(18, 127), (18, 127)])
    raw("run_past_end", 7, w.bytes() + b"\x00" * 8)
    w = Bits()  # the good header of hand_run_across without a length for symbol 256
    dynamic_header(w, 1, 258, 4, {0: 2, 2: 2, 16: 2, 18: 2},
                   [(18, 65 - 11), (2, 0), (0, 0), (2, 0), (18, 138 - 11), (18, 50 - 11), (0, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0)])
    raw("no_end_of_block", 8, w.bytes() + b"\x00" * 8)
    raw("litlen_286", 9, _fixed([65, 286, 256]))
    raw("dist_30", 10, _fixed([65, 257, ("raw", FIXED_DIST[30]), 256]))
    raw("distance_too_far", 11, _fixed([65, 257, ("raw", FIXED_DIST[1]), 256]))
    out.append(("output_beyond_isize", 12, reframe(good, isize=isize - 1)))
    out.append(("output_short", 13, reframe(good, isize=isize + 1)))
    out.append(("input_exhausted", 14, reframe(good, payload=pay[:-3])))
    out.append(("trailing_byte", 15, reframe(good, payload=pay + b"\x00")))
    out.append(("crc_mismatch", 16, reframe(good, crc=crc ^ 0x100)))
    return out


def seeded_damage(n=200, seed=22):
    """[(name, block, may_pass)]: single-byte flips and payload truncations of corpus blocks.  may_pass: the damage is in a
    gzip header field the decoder ignores (MTIME, XFL, OS) or in the last payload byte, whose unused bits are padding."""
    rng = np.random.default_rng(seed)
    blocks = [b for name, _, b in corpus() if name != "empty"]
    out = []
    for i in range(n):
        b = blocks[int(rng.integers(0, len(blocks)))]
        head, pay, crc, isize = parts(b)
        if i % 2 == 0:
            at = int(rng.integers(0, len(b)))
            x = bytearray(b)
            x[at] ^= int(rng.integers(1, 256))
            out.append(("flip_%d_at_%d" % (i, at), bytes(x), 4 <= at < 10 or at == len(head) + len(pay) - 1))
        else:
            cut = int(rng.integers(1, min(len(pay), 64) + 1))
            out.append(("cut_%d_by_%d" % (i, cut), reframe(b, payload=pay[:-cut]), False))
    return out
