"""Host-side mirror of the reference's command-line operators for the hot path, on top of the C-ABI.

Each function keeps the name, argument meaning and file formats of the tool it mirrors:

=====================  ==========================================================================
``jellyfish_count``    ``jellyfish count -m K -s SIZE [-C] [-L n] [-U n] -o OUT IN...``
                       (scripts/RunJellyForRUFUS.sh:29)
``jellyfish_histo``    ``jellyfish histo [-f] DB``  (scripts/RunJellyForRUFUS.sh:37)
``jellyfish_dump``     ``jellyfish dump -c DB``  (scripts/Overlap.shorter.sh:247)
``jellyfish_query``    ``jellyfish query -s FASTA DB``  (scripts/CheckJellyHashList.sh:12)
``rufus_merge``        RUFUS's modified ``jellyfish merge F1 F2 ...``  (runRufus.sh:925)
``check_jelly_hash_list``  scripts/CheckJellyHashList.sh:12  (query + MinCov/MaxCov awk filters)
``rufus_filter``       ``RUFUS.Filter HashList M1 M2 STUB K MinQ Thresh Threads``  (runRufus.sh:967)
``rufus_filter_single``  ``RUFUS.Filter.single HashList FQ STUB K MinQ Thresh Threads``
=====================  ==========================================================================

Text parsing and file I/O happen here on the host; all arithmetic (k-mer extraction, hashing,
counting, sorting, set difference, read scan) runs in the HIP kernels behind ``rufus_amd.capi``.
"""
from __future__ import annotations

import json
import zlib

import numpy as np

from . import capi

_CODES = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODES[_c] = _i
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------
# k-mer text <-> jellyfish key (jf/include/jellyfish/mer_dna.hpp: first base most significant)
# ---------------------------------------------------------------------------------------------------
def keys_to_text(keys: np.ndarray, k: int) -> list:
    keys = np.asarray(keys, dtype=np.uint64)
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    codes = ((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)
    rows = _LETTERS[codes]
    return [r.tobytes().decode() for r in rows]


def text_to_key(kmer: str) -> int:
    v = 0
    for ch in kmer.upper().encode():
        c = int(_CODES[ch])
        if c > 3:
            raise ValueError(f"Invalid mer '{kmer}'")
        v = (v << 2) | c
    return v


def revcomp_key(key: int, k: int) -> int:
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (key & 3))
        key >>= 2
    return r


# ---------------------------------------------------------------------------------------------------
# sequence files
# ---------------------------------------------------------------------------------------------------
def parse_sequences(data: bytes) -> list:
    """Sequences of a FASTA/FASTQ file the way jellyfish's parser sees them
    (jf/include/jellyfish/mer_overlap_sequence_parser.hpp:124-251): type sniffed from the first byte,
    multi-line records joined, qualities skipped by length."""
    if not data:
        return []
    lines = data.split(b"\n")
    if data[:1] == b">":
        out, cur = [], None
        for ln in lines:
            if ln[:1] == b">":
                if cur is not None:
                    out.append(b"".join(cur))
                cur = []
            elif cur is not None:
                cur.append(ln)
        if cur is not None:
            out.append(b"".join(cur))
        return out
    if data[:1] != b"@":
        raise ValueError("Unsupported format")
    # fast path: strict 4-line records
    n4 = len(lines) - (1 if lines[-1] == b"" else 0)
    if n4 % 4 == 0 and all(l[:1] == b"+" for l in lines[2:n4:4][:64]):
        seqs, quals, plus = lines[1:n4:4], lines[3:n4:4], lines[2:n4:4]
        if all(p[:1] == b"+" for p in plus) and all(len(s) == len(q) for s, q in zip(seqs, quals)):
            return seqs
    out, i, n = [], 0, len(lines)
    while i < n:
        if lines[i] == b"":
            i += 1
            continue
        if lines[i][:1] != b"@":
            raise ValueError("Invalid fastq sequence")
        i += 1
        seq = []
        while i < n and lines[i][:1] != b"+":
            seq.append(lines[i])
            i += 1
        s = b"".join(seq)
        i += 1
        q = 0
        while i < n and q < len(s):
            q += len(lines[i])
            i += 1
        if q != len(s):
            raise ValueError("Invalid fastq sequence")
        out.append(s)
    return out


def parse_fastq4(data: bytes):
    """Strict 4-line FASTQ as RUFUS.Filter reads it (src/RUFUS.Filter.cpp:162-175): (headers, seqs, plus, quals)."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    n = len(lines) // 4 * 4
    return lines[0:n:4], lines[1:n:4], lines[2:n:4], lines[3:n:4]


# ---------------------------------------------------------------------------------------------------
# .Jhash files
# ---------------------------------------------------------------------------------------------------
class JhashFile:
    """A ``binary/sorted`` jellyfish database held as device records plus its header facts."""

    def __init__(self, records: capi.Records, cols: np.ndarray, canonical: bool, counter_len: int = 4):
        self.records, self.cols, self.canonical, self.counter_len = records, cols, canonical, counter_len

    @property
    def k(self):
        return self.records.k

    @property
    def lsize(self):
        return self.records.lsize

    def write(self, path: str, argv=()):
        hdr = capi.jhash_header(self.k, self.lsize, self.cols, self.canonical, self.counter_len, argv)
        with open(path, "wb") as f:
            f.write(hdr)
            f.write(self.records.payload(self.counter_len))

    @classmethod
    def read(cls, ctx: capi.Context, path: str) -> "JhashFile":
        blob = open(path, "rb").read()
        digits = blob[:9]
        if not digits.isdigit() or blob[9:10] != b"{":
            raise ValueError(f"Failed to parse header of file '{path}'")
        hlen = int(digits)
        hdr = json.loads(blob[9:9 + hlen].rstrip(b"\0"))
        if hdr.get("format") != "binary/sorted":
            raise ValueError(f"Unsupported format '{hdr.get('format')}'")
        k = hdr["key_len"] // 2
        cols = np.array(hdr["matrix1"]["columns"], dtype=np.uint64)
        lsize = capi.ceil_log2(hdr["size"])
        rec = capi.Records.load(ctx, k, lsize, cols, blob[9 + hlen:], hdr["counter_len"])
        return cls(rec, cols, bool(hdr.get("canonical", False)), hdr["counter_len"])


def is_bam(data: bytes) -> bool:
    """A BGZF file whose first block inflates to the BAM magic."""
    if data[:4] != b"\x1f\x8b\x08\x04":
        return False
    try:
        nb, used, _ = capi.bgzf_scan(data[:1 << 16], 1)
        return nb == 1 and zlib.decompress(data[:used], 31)[:4] == b"BAM\x01"
    except (capi.RufusError, zlib.error):
        return False


def _bam_arenas(ctx: capi.Context, data: bytes, arena_bytes: int, region=None, index: bytes | None = None):
    """The settled arenas of a BAM file, one after the other: yields (arena, whole records, header).  The arena is reset
    when the caller comes back for the next.  region (`samtools view X.bam REGION`): every arena gets bam_set_region before
    it is handed out; with `index` (the .bai file's bytes) only the blocks of capi.bai_query's range are inflated, without it
    all of them."""
    hdr = capi.bam_header(data)
    if hdr is None:
        raise ValueError("the BAM header is not whole")
    at, skip, stop_at, reg = hdr["first_block"], hdr["skip"], len(data), None
    if region is not None:
        reg = capi.bam_region_parse(region, hdr["names"])
        if index is not None:
            rng = capi.bai_query(index, hdr["n_ref"], len(data), *reg)
            if rng is None:
                return
            at, skip, stop_at = rng[0] >> 16, rng[0] & 0xFFFF, rng[1] >> 16
            if rng[1] & 0xFFFF:  # STOP lies inside a block: that block is the last
                nb, used, _ = capi.bgzf_scan(data[stop_at:stop_at + 65536], 1)
                if nb != 1:
                    raise ValueError(f"no whole BGZF block at byte {stop_at} of the BAM file")
                stop_at += used
    ranged = stop_at != len(data) or at != hdr["first_block"]
    data = data[:stop_at]
    arenas = [capi.TextArena(ctx, arena_bytes), capi.TextArena(ctx, arena_bytes)]
    try:
        cur = 0
        while True:
            a = arenas[cur]
            while at < len(data) and a.bytes + 65536 <= arena_bytes:
                nb, used, _ = capi.bgzf_scan(data[at:at + (8 << 20)], min((arena_bytes - a.bytes) // 65536, 4096))
                if nb == 0:
                    raise ValueError(f"no whole BGZF block at byte {at} of the BAM file")
                a.append_bgzf(data[at:at + used])
                at += used
            last = at >= len(data)
            # (a range's last block holds whatever follows the region: its cut record goes to the other arena and is dropped)
            n, _ = a.bam_settle(None if last and not ranged else arenas[cur ^ 1], skip, hdr["n_ref"])
            skip = 0
            if reg is not None:
                a.bam_set_region(*reg)
            if n:
                yield a, n, hdr
            a.reset()
            if last:
                arenas[cur ^ 1].reset()
            if last:
                break
            cur ^= 1
    finally:
        for a in arenas:
            a.close()


def bam_read_blocks(ctx: capi.Context, data: bytes, exclude_flags: int = 3328, arena_bytes: int = 256 << 20, region=None,
                    index: bytes | None = None):
    """The records of a BAM file with flag & exclude_flags == 0 as count blocks, an arena at a time: yields (block, runs,
    reference names) -- what `samtools view -F 3328 X.bam | PassThroughSamCheck` hands the counter, found and packed on the
    device (capi.bam_header, TextArena.append_bgzf / bam_settle / bam_parse).  region, index: `samtools view X.bam REGION`
    (_bam_arenas).  The caller frees the blocks."""
    for a, _, hdr in _bam_arenas(ctx, data, arena_bytes, region, index):
        blk, runs = a.bam_parse(exclude_flags)
        yield blk, runs, hdr["names"]


def is_plain_gzip(data: bytes) -> bool:
    """A gzip file (magic 1f 8b, deflate) that is not BGZF: what a sequencer or an archive hands out as .fastq.gz."""
    if data[:3] != b"\x1f\x8b\x08":
        return False
    try:
        return capi.bgzf_scan(data[:1 << 16], 1)[0] == 0
    except capi.RufusError:
        return True


def gzip_read_blocks(ctx: capi.Context, data: bytes, arena_bytes: int = 256 << 20, piece: int = 128 << 20):
    """The reads of a plain-gzip FASTQ file as count blocks, an arena at a time, inflated on the device
    (capi.GzipStream.append: the stream cut speculatively, a chain rule on the host; TextArena.settle / parse): what
    `zcat F.fastq.gz |` hands the counter.  Strict 4-line FASTQ only.  The caller frees the blocks."""
    arenas = [capi.TextArena(ctx, arena_bytes), capi.TextArena(ctx, arena_bytes)]
    gz = capi.GzipStream(ctx)
    try:
        cur, at = 0, 0

        def sink(a):
            if a.bytes:
                block = a.parse(capi.PACK_COUNT)
                if block is None:
                    raise ValueError("compressed input must be strict 4-line FASTQ")
                yield block
            a.reset()

        while at < len(data):
            a = arenas[cur]
            n = min(piece, len(data) - at)
            got, used = gz.append(a, data[at:at + n], at + n == len(data))
            at += used
            if got or used:
                continue
            if gz.need():  # the arena is full
                before = a.bytes
                if a.settle(arenas[cur ^ 1]) == before:
                    raise ValueError("compressed input must be strict 4-line FASTQ")
                yield from sink(a)
                cur ^= 1
            else:
                piece *= 2
        a, nx = arenas[cur], arenas[cur ^ 1]
        if a.settle(nx):  # a file without a final newline gets one
            nx.append(b"\n")
            yield from sink(a)
            nx.settle(None)
            yield from sink(nx)
        else:
            yield from sink(a)
    finally:
        gz.close()
        for a in arenas:
            a.close()


def jellyfish_count(ctx: capi.Context, inputs, k: int, size: int, canonical: bool = True, lower: int = 0,
                    upper: int = 2**64 - 1, out: str | None = None, capacity: int = 0, argv=(),
                    mode: int = capi.COUNT_AUTO, region=None, index: bytes | None = None) -> JhashFile:
    """Count the k-mers of FASTA/FASTQ files (paths or bytes; a plain-gzip FASTQ is inflated on the device); a BAM file is counted as `samtools view -F 3328` of it, with
    `region` as `samtools view -F 3328 X.bam REGION` (ONE BAM input; index: its .bai's bytes, or None for the whole walk)."""
    if region is not None and len(inputs) != 1:
        raise ValueError("region goes with ONE BAM input")
    table = capi.CountTable(ctx, k, size, canonical, capacity, mode=mode)
    try:
        for src in inputs:
            data = src if isinstance(src, (bytes, bytearray)) else open(src, "rb").read()
            if is_bam(bytes(data)):
                for block, _, _ in bam_read_blocks(ctx, bytes(data), region=region, index=index):
                    try:
                        table.add(block)
                    finally:
                        block.free()
                continue
            if region is not None:
                raise ValueError("region goes with a BAM input: only a BAM's records carry a position")
            if is_plain_gzip(bytes(data)):  # (FASTQ: anything else wants `zcat`, as the executable says)
                for block in gzip_read_blocks(ctx, bytes(data)):
                    try:
                        table.add(block)
                    finally:
                        block.free()
                continue
            seqs = parse_sequences(bytes(data))
            block = ctx.upload(capi.PackedReads.from_reads(seqs, flags=capi.PACK_COUNT))
            try:
                table.add(block)
            finally:
                block.free()
        rec = table.finish(lower, upper)
    finally:
        table.free()
    jf = JhashFile(rec, capi.jf_matrix(capi.ceil_log2(size), k), canonical)
    if out:
        jf.write(out, argv)
    return jf


def histo_text(h: np.ndarray, full: bool = False) -> str:
    """jf/sub_commands/histo_main.cc:82-84: ``count n`` rows, empty bins only with -f."""
    return "".join(f"{i} {int(v)}\n" for i, v in enumerate(h) if full or v > 0)


def jellyfish_histo(db: JhashFile, full: bool = False) -> str:
    return histo_text(db.records.histo(), full)


def jellyfish_dump(db: JhashFile) -> str:
    keys, counts, _ = db.records.get()
    return "".join(f"{t} {int(c)}\n" for t, c in zip(keys_to_text(keys, db.k), counts))


def jellyfish_query(db: JhashFile, kmers) -> str:
    """``KMER COUNT`` per query k-mer; canonicalised when the database is (query_main.cc:115)."""
    keys = []
    for km in kmers:
        key = text_to_key(km)
        if db.canonical:
            key = min(key, revcomp_key(key, db.k))
        keys.append(key)
    keys = np.array(keys, dtype=np.uint64)
    counts = db.records.query(keys)
    return "".join(f"{t} {int(c)}\n" for t, c in zip(keys_to_text(keys, db.k), counts))


def rufus_merge(ctx: capi.Context, files) -> str:
    """stdout of RUFUS's modified ``jellyfish merge``: ``KMER\\tCOUNT`` for keys in exactly one input, count >= 5."""
    keys, counts = capi.merge_unique(ctx, [f.records for f in files], 5)
    return "".join(f"{t}\t{int(c)}\n" for t, c in zip(keys_to_text(keys, files[0].k), counts))


def check_jelly_hash_list(db: JhashFile, merge_text: str, min_cov: int, max_cov: int) -> str:
    kmers = [ln.split()[0] for ln in merge_text.splitlines() if ln.strip()]
    out = []
    for ln in jellyfish_query(db, kmers).splitlines():
        c = int(ln.split()[1])
        if min_cov <= c <= max_cov:
            out.append(ln + "\n")
    return "".join(out)


def hash_list(ctx: capi.Context, subject: JhashFile, others, min_cov: int, max_cov: int) -> str:
    """Fused runRufus.sh:925-926: same text as rufus_merge | check_jelly_hash_list, one device pass."""
    keys, counts = capi.unique_to_subject(ctx, subject.records, [o.records for o in others], min_cov, max_cov)
    return "".join(f"{t} {int(c)}\n" for t, c in zip(keys_to_text(keys, subject.k), counts))


def hash_list_of_run(res: dict, k: int) -> str:
    """The ``kmer count`` text (runRufus.sh:925-926, the .HashList file) of a wgs.WgsTrio.run() result: its mutant_keys
    and mutant_counts, line for line as hash_list() writes them."""
    keys = np.asarray(res["mutant_keys"], dtype=np.uint64)
    counts = np.asarray(res["mutant_counts"])
    if keys.ndim != 1 or keys.shape != counts.shape:
        raise ValueError("hash_list_of_run: mutant_keys and mutant_counts of one length")
    return "".join(f"{t} {int(c)}\n" for t, c in zip(keys_to_text(keys, k), counts))


# ---------------------------------------------------------------------------------------------------
# RUFUS.Filter
# ---------------------------------------------------------------------------------------------------
def _mask_bits(mask: np.ndarray, n: int) -> np.ndarray:
    bits = np.unpackbits(mask.view(np.uint8), bitorder="little")[:n]
    return bits.astype(bool)


def rufus_filter(ctx: capi.Context, hashlist: str, mate1: str, mate2: str, stub: str, k: int, min_q: int, thresh: int,
                 threads: int = 1) -> int:
    """Writes ``STUB.Mutations.Mate1.fastq`` / ``Mate2``; returns the number of pulled pairs.  Pairs
    are written in input order (the reference's order depends on OpenMP scheduling)."""
    keys = capi.hashlist_keys(open(hashlist, "rb").read(), k, single_end=False)
    h1, s1, p1, q1 = parse_fastq4(open(mate1, "rb").read())
    h2, s2, p2, q2 = parse_fastq4(open(mate2, "rb").read())
    if any(len(s) == 0 for s in s1) or any(len(s) == 0 for s in s2):
        raise ValueError("empty sequence line (undefined behaviour in the reference; rejected)")
    n = len(s1)
    mset = capi.MutantSet(ctx, keys, k)
    pulled = np.zeros(n, dtype=bool)
    try:
        for seqs, quals in ((s1, q1), (s2[:n], q2[:n])):
            blk = ctx.upload(capi.PackedReads.from_reads(seqs, quals, min_q, capi.PACK_FILTER))
            try:
                _, mask, _ = mset.filter(blk, thresh, last_base_skipped=True, want_hits=False)
            finally:
                blk.free()
            pulled[:len(seqs)] |= _mask_bits(mask, len(seqs))
    finally:
        mset.free()
    with open(stub + ".Mutations.Mate1.fastq", "wb") as f1, open(stub + ".Mutations.Mate2.fastq", "wb") as f2:
        for i in np.flatnonzero(pulled):
            f1.write(h1[i] + b"\n" + s1[i] + b"\n" + p1[i] + b"\n" + q1[i] + b"\n")
            if i < len(s2):
                f2.write(h2[i] + b"\n" + s2[i] + b"\n" + p2[i] + b"\n" + q2[i] + b"\n")
    return int(pulled.sum())


def rufus_filter_single(ctx: capi.Context, hashlist: str, fastq: str, stub: str, k: int, min_q: int, thresh: int,
                        threads: int = 1) -> int:
    """``STUB.Mutations.fastq`` with ``:MH<hits>`` appended to each header (src/RUFUS.Filter.ss.cpp:198)."""
    keys = capi.hashlist_keys(open(hashlist, "rb").read(), k, single_end=True)
    h, s, p, q = parse_fastq4(open(fastq, "rb").read())
    mset = capi.MutantSet(ctx, keys, k)
    try:
        blk = ctx.upload(capi.PackedReads.from_reads(s, q, min_q, capi.PACK_FILTER))
        try:
            hits, mask, _ = mset.filter(blk, thresh, last_base_skipped=False)
        finally:
            blk.free()
    finally:
        mset.free()
    pulled = _mask_bits(mask, len(s))
    with open(stub + ".Mutations.fastq", "wb") as f:
        for i in np.flatnonzero(pulled):
            f.write(h[i] + b":MH%d\n" % int(hits[i]) + s[i] + b"\n" + p[i] + b"\n" + q[i] + b"\n")
    return int(pulled.sum())


# ---------------------------------------------------------------------------------------------------
# packed blocks back to text
# ---------------------------------------------------------------------------------------------------
def decode_reads(arrays: dict) -> list:
    """The sequences of a packed block, from the dict ``capi.ReadBlock.get()`` returns (codes, word_off, len and, if
    there, acgt): ``A C G T`` by the 2-bit codes, ``N`` where the ACGT bit is clear (which base it was is not kept)."""
    codes, word_off, lens, acgt = arrays["codes"], arrays["word_off"], arrays["len"], arrays.get("acgt")
    pos = (2 * np.arange(32)).astype(np.uint64)
    letters = _LETTERS[((codes[:, None] >> pos[None, :]) & np.uint64(3)).astype(np.intp)]      # words x 32
    if acgt is not None:
        valid = np.unpackbits(np.ascontiguousarray(acgt, dtype="<u4").view(np.uint8), bitorder="little").reshape(-1, 32)
        letters = np.where(valid.astype(bool), letters, np.uint8(ord("N")))
    flat = np.ascontiguousarray(letters, dtype=np.uint8).reshape(-1).tobytes()
    return [flat[32 * int(w):32 * int(w) + int(n)] for w, n in zip(word_off[:len(lens)], lens)]


# ---------------------------------------------------------------------------------------------------
# RUFUS.Filter --bam
# ---------------------------------------------------------------------------------------------------
_SEQ_LETTERS = b"=ACMGRSVTWYHKDBN"
_REVCOMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _bam_printed(rec: bytes):
    """(QNAME, SEQ, QUAL) of one raw BAM record (block_size field first) as `samtools view | PassThroughSamCheck.stranded`
    prints it: reverse strand reverse-complemented with every base but A C G T N dropped, its quality string reversed."""
    l_name, flag, l_seq = rec[12], int.from_bytes(rec[18:20], "little"), int.from_bytes(rec[20:24], "little")
    at = 36 + l_name + 4 * int.from_bytes(rec[16:18], "little")
    name = rec[36:36 + l_name].split(b"\0")[0]
    nib = np.frombuffer(rec[at:at + (l_seq + 1) // 2], np.uint8)
    seq = np.frombuffer(_SEQ_LETTERS, np.uint8)[np.stack([nib >> 4, nib & 15], 1).reshape(-1)[:l_seq]].tobytes() if l_seq else b"*"
    q = rec[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq]
    qual = b"*" if not l_seq or q[0] == 0xFF else bytes(33 + min(v, 93) for v in q)
    if flag & 16:
        seq = bytes(c for c in seq[::-1] if c in b"ACGTN").translate(_REVCOMP)
        qual = qual[::-1]
    return name, seq, qual


def filter_bam(ctx: capi.Context, data: bytes, hash_list: bytes, k: int, min_q: int, thresh: int, exclude_flags: int = 3328,
               arena_bytes: int = 256 << 20, region=None, index: bytes | None = None):
    """``RUFUS.Filter --bam`` on the bytes of a BAM file: (Mate1 bytes, Mate2 bytes, chromosome log) -- what `samtools view
    -F exclude_flags | PassThroughSamCheck.stranded | RUFUS.Filter` writes.  Two passes, both on the device: the scan of
    every kept record in its stranded form (TextArena.bam_parse_filter, MutantSet.filter, bam_name_hashes of the hits),
    then the pull of every record of a hit name (NameSet, bam_mark_names, bam_gather); the few pulled records are printed
    and paired by name here.  region, index: both passes as `samtools view -F exclude_flags X.bam REGION` (_bam_arenas)."""
    mset = capi.MutantSet(ctx, capi.hashlist_keys(hash_list, k, single_end=False), k)
    hit_index, hit_hash, refs, names, base = [], [], [], [], 0
    try:
        for a, _, hdr in _bam_arenas(ctx, data, arena_bytes, region, index):
            names = hdr["names"]
            blk, runs = a.bam_parse_filter(min_q, exclude_flags)
            try:
                _, mask, n_hit = mset.filter(blk, thresh, last_base_skipped=True, want_hits=False)
                n = blk.n
            finally:
                blk.free()
            refs += [int(r) for r in runs[:, 1]]
            if n_hit:
                hit_hash.append(a.bam_name_hashes(n, mask, exclude_flags))
                hit_index += [base + int(i) for i in np.flatnonzero(_mask_bits(mask, n))]
            base += n
    finally:
        mset.free()
    log, current = [], b"notachr"
    for r in refs:
        name = b"*" if r < 0 else names[r]
        if name != current:
            log.append(current)
            current = name
    log = b"".join(x + b"\n" for x in log + [current])
    if not hit_index:
        return b"", b"", log
    hits, waiting, out1, out2, base = set(hit_index), {}, [], [], 0
    nset = capi.NameSet(ctx, np.concatenate(hit_hash))
    try:
        for a, _, _ in _bam_arenas(ctx, data, arena_bytes, region, index):
            mask, n_kept, n_marked = a.bam_mark_names(nset, exclude_flags)
            if n_marked:
                blob, p = a.bam_gather(mask, n_kept, exclude_flags), 0
                for i in np.flatnonzero(_mask_bits(mask, n_kept)):
                    size = 4 + int.from_bytes(blob[p:p + 4], "little")
                    name, seq, qual = _bam_printed(blob[p:p + size])
                    p += size
                    hit = base + int(i) in hits
                    if name not in waiting:
                        waiting[name] = (seq, qual, hit)
                        continue
                    seq2, qual2, hit2 = waiting.pop(name)  # the later record is mate 1, the stored one mate 2
                    if not seq:
                        raise ValueError("empty sequence line (undefined behaviour in the reference; rejected)")
                    if hit or hit2:
                        out1.append(b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n")
                        out2.append(b"@" + name + b"\n" + seq2 + b"\n+\n" + qual2 + b"\n")
            base += n_kept
    finally:
        nset.free()
    return b"".join(out1), b"".join(out2), log


def filter_bam_single(ctx: capi.Context, data: bytes, hash_list: bytes, k: int, min_q: int, thresh: int, exclude_flags: int = 3328,
                      arena_bytes: int = 256 << 20, region=None, index: bytes | None = None):
    """``RUFUS.Filter.single --bam`` on the bytes of a BAM file: (STUB.Mutations.fastq bytes, chromosome log) -- what
    `samtools view -F exclude_flags | PassThroughSamCheck.stranded.se | RUFUS.Filter.single` writes.  One pass, on the
    device: per arena the stranded filter form (TextArena.bam_parse_filter) and the records whose count of hit windows --
    the last base examined -- reaches `thresh`, with that count (TextArena.bam_gather_hits); the few pulled records are
    printed here with `:MH<hits>`.  region, index: as `samtools view -F exclude_flags X.bam REGION` (_bam_arenas)."""
    mset = capi.MutantSet(ctx, capi.hashlist_keys(hash_list, k, single_end=True), k)
    out, refs, names = [], [], []
    try:
        for a, _, hdr in _bam_arenas(ctx, data, arena_bytes, region, index):
            names = hdr["names"]
            blk, runs = a.bam_parse_filter(min_q, exclude_flags)
            try:
                blob, hits, _ = a.bam_gather_hits(mset, blk, thresh, last_base_skipped=False, exclude_flags=exclude_flags)
            finally:
                blk.free()
            refs += [int(r) for r in runs[:, 1]]
            p = 0
            for h in hits:
                size = 4 + int.from_bytes(blob[p:p + 4], "little")
                name, seq, qual = _bam_printed(blob[p:p + size])
                p += size
                out.append(b"@" + name + b":MH%d\n" % int(h) + seq + b"\n+\n" + qual + b"\n")
            if p != len(blob):
                raise ValueError("the gathered records do not add up")
    finally:
        mset.free()
    log, current = [], b"notachr"
    for r in refs:
        name = b"*" if r < 0 else names[r]
        if name != current:
            log.append(current)
            current = name
    return b"".join(out), b"".join(x + b"\n" for x in log + [current])
