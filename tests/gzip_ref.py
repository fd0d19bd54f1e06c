"""The corpus and the truths of the plain-gzip decoder's tests (tests/test_gzip_host.py, tests/test_gzip_gpu.py,
tests/test_cli_gzip_gpu.py).

Inputs come from Python's ``zlib`` / ``gzip`` and the small bit writer of tests/bgzf_ref.py.  Truth for the bytes is
``zlib``'s own inflate; truth for the deflate block boundaries is zlib's ``inflate(Z_BLOCK)`` walk through ``ctypes`` on
the machine's libz (``data_type`` bits 7 and 6, ``total_in * 8 - (data_type & 7)``) -- never the code under test.
Not a conftest: the test modules import it.
"""
import ctypes as C
import ctypes.util
import functools
import struct
import zlib

import numpy as np

from tests import bgzf_ref as B

OS_UNIX = 3


# ---- gzip members ----------------------------------------------------------------------------------------------------
def member(data: bytes, raw=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, fname=None, extra=None, comment=None,
           fhcrc=False, flg_or=0) -> bytes:
    """One gzip member (RFC 1952) around a raw deflate stream (made here, or `raw`)."""
    if raw is None:
        raw = B.deflate(data, level, mem_level, strategy)
    flg = (4 if extra is not None else 0) | (8 if fname is not None else 0) | (16 if comment is not None else 0) | (2 if fhcrc else 0)
    head = b"\x1f\x8b\x08" + bytes([flg | flg_or]) + b"\x00\x00\x00\x00" + b"\x00" + bytes([OS_UNIX])
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\x00"
    if comment is not None:
        head += comment + b"\x00"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + raw + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def header_len(buf: bytes, at=0) -> int:
    """The bytes of the member header at buf[at:]."""
    assert buf[at:at + 3] == b"\x1f\x8b\x08"
    flg, p = buf[at + 3], at + 10
    if flg & 4:
        p += 2 + struct.unpack_from("<H", buf, p)[0]
    for bit in (8, 16):
        if flg & bit:
            p = buf.index(b"\x00", p) + 1
    if flg & 2:
        p += 2
    return p - at


def inflate_all(buf: bytes) -> bytes:
    """Every member of a gzip file, by zlib; raises zlib.error on what zlib refuses (a truncated member included)."""
    out, rest = [], buf
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        if not d.eof:
            raise zlib.error("truncated")
        rest = d.unused_data
    return b"".join(out)


# ---- zlib's own block walk ---------------------------------------------------------------------------------------------
class _ZStream(C.Structure):
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_uint), ("total_in", C.c_ulong), ("next_out", C.c_void_p),
                ("avail_out", C.c_uint), ("total_out", C.c_ulong), ("msg", C.c_char_p), ("state", C.c_void_p),
                ("zalloc", C.c_void_p), ("zfree", C.c_void_p), ("opaque", C.c_void_p), ("data_type", C.c_int),
                ("adler", C.c_ulong), ("reserved", C.c_ulong)]


@functools.lru_cache(None)
def _libz():
    lib = C.CDLL(ctypes.util.find_library("z") or "libz.so.1")
    lib.zlibVersion.restype = C.c_char_p
    return lib


def block_starts(raw: bytes):
    """[(bit offset, BFINAL, BTYPE)] of every deflate block of a raw deflate stream, by zlib's inflate(Z_BLOCK)."""
    lib = _libz()
    s = _ZStream()
    assert lib.inflateInit2_(C.byref(s), -15, lib.zlibVersion(), C.sizeof(_ZStream)) == 0
    src = C.create_string_buffer(raw, len(raw))
    out = C.create_string_buffer(1 << 20)
    s.next_in, s.avail_in = C.addressof(src), len(raw)
    bits = [0]
    try:
        while True:
            s.next_out, s.avail_out = C.addressof(out), len(out)
            r = lib.inflate(C.byref(s), 5)  # Z_BLOCK
            assert r in (0, 1), r
            if r == 1:
                break
            if (s.data_type & 128) and not (s.data_type & 64):
                bits.append(s.total_in * 8 - (s.data_type & 7))
    finally:
        lib.inflateEnd(C.byref(s))

    def get(bit, n):
        v = int.from_bytes(raw[bit >> 3:(bit >> 3) + 4], "little") >> (bit & 7)
        return v & ((1 << n) - 1)

    return [(b, get(b, 1), get(b + 1, 2)) for b in bits]


def file_block_starts(gz: bytes):
    """block_starts of a ONE-member gzip file, as bit offsets in the file."""
    h = header_len(gz)
    return [(b + 8 * h, f, t) for b, f, t in block_starts(gz[h:-8])]


# ---- hand-written streams ----------------------------------------------------------------------------------------------
_LIT = B.canon({65: 2, 67: 2, 256: 2, 285: 2})  # 'A', 'C', end of block, length 258


def _hand_header(w, final):
    """A dynamic header: literals 'A' and 'C', end of block and length 258 in two bits each, ONE distance code (symbol 29)."""
    B.dynamic_header(w, final, 286, 30, {0: 2, 1: 2, 2: 2, 18: 2},
                     [(18, 65 - 11), (2, 0), (0, 0), (2, 0), (18, 138 - 11), (18, 50 - 11), (2, 0), (18, 28 - 11), (2, 0),
                      (18, 29 - 11), (1, 0)])


def hand_window_edge(rng):
    """(data, raw): a dynamic block of exactly 32768 literals, then a dynamic block that BEGINS with a match of length 258
    at distance 32768 -- its source starts at the first byte of the block before -- then an empty final block."""
    first = np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, 32768)].tobytes()
    tail = np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, 500)].tobytes()
    w = B.Bits()
    _hand_header(w, 0)
    for ch in first:
        w.code(_LIT[ch])
    w.code(_LIT[256])
    second_bit = len(w.out) * 8 + w.n
    _hand_header(w, 0)
    w.code(_LIT[285]), w.code((0, 1)), w.put(32768 - 24577, 13)
    for ch in tail:
        w.code(_LIT[ch])
    w.code(_LIT[256])
    w.put(1, 1), w.put(1, 2), w.code(B.FIXED_LIT[256])
    data = first + first[:258] + tail
    raw = w.bytes()
    assert zlib.decompress(raw, -15) == data
    return data, raw, second_bit


def _bits_slice(raw: bytes, lo: int, hi: int) -> bytes:
    """Bits [lo, hi) of raw, moved to bit 0 of the first byte (the last byte zero-padded)."""
    v = int.from_bytes(raw, "little") >> lo
    v &= (1 << (hi - lo)) - 1
    return v.to_bytes((hi - lo + 7) // 8, "little")


def planted_false_positive(rng):
    """(data, gzip file, the planted block's bit offset in the file): a complete non-final dynamic block of a real stream,
    byte-aligned inside the payload of a stored block (zeros around it: no header there), then a real stream."""
    donor = B.deflate(B.fastq_text(rng, 400, genome_len=200000), 6, mem_level=4)
    st = block_starts(donor)
    pick = next(i for i, (b, f, t) in enumerate(st[:-1]) if f == 0 and t == 2 and 300 < (st[i + 1][0] - b) // 8 < 30000 and i > 0)
    blk = _bits_slice(donor, st[pick][0], st[pick + 1][0])
    payload = bytes(3000) + blk + bytes(2500)
    assert len(payload) < 65536
    rest = B.fastq_text(rng, 300, genome_len=200000)
    w = B.Bits()
    w.put(0, 1), w.put(0, 2), w.align()
    w.put(len(payload), 16), w.put(len(payload) ^ 0xFFFF, 16), w.raw(payload)
    raw = w.bytes() + B.deflate(rest, 6)
    data = payload + rest
    assert zlib.decompress(raw, -15) == data
    gz = member(data, raw=raw, fname=b"planted.fastq")
    return data, gz, 8 * (header_len(gz) + 5 + 3000)


# ---- the corpus --------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def big_text():
    """3.8 MB of FASTQ from a 2 Mb genome: deflates 3 : 1, a level-6 block is ~28 KB of input."""
    return B.fastq_text(np.random.default_rng(50), 11500, genome_len=2000000)


@functools.lru_cache(None)
def corpus():
    """[(name, original bytes, gzip file)] -- every shape at which the route branches."""
    rng = np.random.default_rng(51)
    big = big_text()
    mid = big[:1 << 20]
    small = big[:300000]
    out = [("fastq_l6", big, member(big, level=6, fname=b"big.fastq")),
           ("fastq_l1", mid, member(mid, level=1)),
           ("fastq_l9", mid, member(mid, level=9)),
           ("fixed", small, member(small, strategy=zlib.Z_FIXED)),  # no candidate anywhere: one chunk
           ("stored", small[:200000], member(small[:200000], level=0))]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b"".join(c.compress(small[i:i + 10000]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(small), 10000)) + c.flush()
    out.append(("full_flush", small, member(small, raw=raw)))
    out.append(("all_A", b"A" * 900000, member(b"A" * 900000)))  # output >> input: 900 KB from under 1 KB
    a, b = big[:150000], big[150000:400000]
    out.append(("three_members", a + b, member(a, fname=b"a") + member(b"") + member(b, level=1)))
    out.append(("all_header_fields", small, member(small, extra=b"XY\x03\x00abc", fname=b"name.fastq", comment=b"a comment",
                                                   fhcrc=True)))
    data, raw, _ = hand_window_edge(rng)
    out.append(("hand_window_edge", data, member(data, raw=raw)))
    data, gz, _ = planted_false_positive(rng)
    out.append(("planted", data, gz))
    for name, data, gz in out:
        assert inflate_all(gz) == data, name
    return out


def refusals():
    """[(name, gzip file)]: each must be refused."""
    rng = np.random.default_rng(52)
    text = big_text()[:120000]
    good = member(text, fname=b"x.fastq")
    out = [("crc_flipped", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:]),
           ("isize_wrong", good[:-4] + struct.pack("<I", len(text) + 1)),
           ("reserved_flg_bit", member(text, flg_or=0x20)),
           ("cm_not_8", good[:2] + b"\x07" + good[3:]),
           ("second_member_bad_magic", good + b"\x1f\x8c" + good[2:])]
    for cut in sorted(int(x) for x in rng.integers(1, len(good) - 1, 12)):
        out.append(("truncated_at_%d" % cut, good[:cut]))
    out.append(("truncated_in_trailer", good[:-3]))
    return out


def seeded_damage(n=200, seed=53):
    """[(name, damaged file, what zlib makes of it: bytes or None)]: single-byte damages of a small two-member file."""
    rng = np.random.default_rng(seed)
    text = big_text()[:40000]
    good = member(text[:25000], fname=b"d.fastq") + member(text[25000:], level=1)
    out = []
    for i in range(n):
        at = int(rng.integers(0, len(good)))
        x = bytearray(good)
        x[at] ^= int(rng.integers(1, 256))
        try:
            want = inflate_all(bytes(x))
        except zlib.error:
            want = None
        out.append(("damage_%d_at_%d" % (i, at), bytes(x), want))
    return out
