"""The FASTA texts of tests/test_fasta_gpu.py and tests/test_fasta_host.py, and a packer written here: what
rfx_pack_reads(RFX_PACK_COUNT) makes of sequences (include/rufus_hip.h: A0 C1 G2 T3 in either case with the ACGT mask bit
set, everything else code 0 without it), in a few lines of numpy that share nothing with the code under test."""
import zlib

import numpy as np

_CODE = np.zeros(256, np.uint64)
_OK = np.zeros(256, np.uint64)
for _i, _ch in enumerate(b"ACGT"):
    for _c in (_ch, _ch | 0x20):
        _CODE[_c], _OK[_c] = _i, 1
_SH2 = (2 * np.arange(32)).astype(np.uint64)
_SH1 = np.arange(32).astype(np.uint64)


def pack(seqs):
    """dict len / word_off / codes / acgt / max_len of the sequences as a count block."""
    lens = np.array([len(s) for s in seqs], np.uint32)
    nw = (lens.astype(np.uint64) + np.uint64(31)) // np.uint64(32)
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum(nw, out=off[1:])
    codes, mask = np.zeros(int(off[-1]), np.uint64), np.zeros(int(off[-1]), np.uint32)
    for s, o, w in zip(seqs, off[:-1], nw):
        if w:
            a = np.zeros(int(w) * 32, np.uint8)
            a[:len(s)] = np.frombuffer(s, np.uint8)
            a = a.reshape(-1, 32)
            codes[int(o):int(o + w)] = (_CODE[a] << _SH2).sum(axis=1, dtype=np.uint64)  # (disjoint bits: the sum is the OR)
            mask[int(o):int(o + w)] = (_OK[a] << _SH1).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return {"len": lens, "word_off": off.astype(np.uint32), "codes": codes, "acgt": mask,
            "max_len": int(lens.max()) if len(lens) else 0}


def read_crcs(p):
    """[(len, crc32 of the read's code words then mask words)]: what tests/host/fasta_harness.cpp prints per read."""
    out = []
    for r, L in enumerate(p["len"]):
        a, b = int(p["word_off"][r]), int(p["word_off"][r + 1])
        out.append((int(L), zlib.crc32(p["codes"][a:b].tobytes() + p["acgt"][a:b].tobytes())))
    return out


def bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def wrap(seq: bytes, width: int, eol=b"\n") -> bytes:
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def record(name: bytes, seq: bytes, width: int = 60, eol=b"\n") -> bytes:
    return b">" + name + eol + wrap(seq, width, eol)


def cases():
    """[(name, text)]: the shapes at which the line join can go wrong."""
    rng = np.random.default_rng(19)
    out = []
    for w in (1, 31, 32, 33, 60, 64, 70):
        out.append((f"width {w}", b"".join(record(b"w%d_%d some words" % (w, i), bases(rng, L), w)
                                           for i, L in enumerate((200, 95, 3 * w + 1, w, 2 * w)))))
    ragged = b">ragged\n"
    for w in rng.integers(1, 90, 40):
        ragged += bases(rng, int(w)) + b"\n"
    out.append(("ragged widths within one record", ragged + record(b"after", bases(rng, 77), 13)))
    out.append(("empty lines inside and at the end of a record",
                b">a\nACGT\n\n\nGGCC\n\n>b\n\n\nTTTT\nAC\n\n\n>c\nACGTACGTACGTACGTACGTACGTACGTACGTA\n\n"))
    out.append(("headers in a row, first and last", b">a\n>b\n>c\nACGTT\n>d\n>e\nAC\n>f\n>g\n>h\n"))
    out.append(("two headers first, two last", b">a\n>b\nACG\n>c\n>d\n"))
    out.append(("only headers", b">a\n>b\n>c\n"))
    out.append(("a '>' inside a sequence line", b">r\nAC>GT\nA>\nACGT>ACGT>\n>s\nG>\n"))
    out.append(("a header full of '>' and base letters", b">>>ACGT>>ACGT>ACGTACGTACGTACGTACGTACGTACGTACGT>\nACGT\n>ACGTACGT\nTTGA\n"))
    out.append(("CR LF line ends", b"".join(record(b"crlf%d" % i, bases(rng, L), 31, b"\r\n") for i, L in enumerate((62, 100, 5)))))
    out.append(("lower case, N and IUPAC letters",
                b"".join(record(b"iupac%d" % i, bases(rng, L, b"ACGTacgtNnRYKMSWBDHVrykm.-*"), 60) for i, L in enumerate((300, 64, 33)))))
    out.append(("a last line without its newline", record(b"x", bases(rng, 100), 60) + b">y\n" + bases(rng, 45)))
    out.append(("a last header without its newline", record(b"x", bases(rng, 70), 60) + b">y"))
    out.append(("a lone '>' at the end", record(b"x", bases(rng, 33), 60) + b">"))
    out.append(("exactly 32, 64 and 32 m + 1 bases", b"".join(record(b"e%d" % L, bases(rng, L), 60) for L in (32, 64, 97, 33, 1, 31))))
    out.append(("sequence lines at each byte residue", b"".join(record(b"r" * i, bases(rng, 150 + i), 60 + i) for i in range(1, 9))))
    out.append(("one record only", record(b"only", bases(rng, 500), 60)))
    out.append(("3000 records of 40 to 300 bases",
                b"".join(record(b"c%d" % i, bases(rng, int(L)), 60) for i, L in enumerate(rng.integers(40, 301, 3000)))))
    out.append(("one record of 1025 bases", record(b"just past the switch", bases(rng, 1025), 60)))
    out.append(("one record of 200000 bases in 70 columns", long_text()))
    return out


def long_text():
    return record(b"chrL a chromosome", bases(np.random.default_rng(23), 200000, b"ACGTACGTACGTACGTACGTN"), 70)


def small_text():
    """A text of every kind of line, short enough that every prefix of it is run."""
    return b">a b>c\nACGTN\n\nacg>t\r\n>\n>>x\n>e\nTTGACCA\nGG"


def big_text(n_bytes=3 << 20, seed=29):
    """About n_bytes of records of 200 to 6000 bases in 60-column lines; the headers hold '>' characters and the last line
    has no newline."""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        rec = record(b"seq%d>>x>y len>%d" % (i, i * 7), bases(rng, int(rng.integers(200, 6001))), 60)
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:-1]
