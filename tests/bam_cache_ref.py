"""A pure-Python reader and writer of the BAM-kind packed-read cache, written from the description at the top of
rufus_amd/csrc/host/rfx_bam_cache.hpp (tests/test_bam_cache_host.py, tests/test_count_filter_bam_cache_gpu.py), and a
brute-force statement of what a fetch plan must satisfy.  Independent of the product.  Not a conftest: the test modules
import it."""
import struct

import numpy as np

FILE_MAGIC = struct.unpack("<Q", b"RBAMCAC1")[0]
CHUNK_MAGIC = struct.unpack("<Q", b"BMCHUNK1")[0]
INDEX_MAGIC = struct.unpack("<Q", b"BMINDEX1")[0]
DONE_MAGIC = struct.unpack("<Q", b"CACHDONE")[0]
SAM_FILE_MAGIC = struct.unpack("<Q", b"RPKCACH1")[0]  # rfx_packed_cache.hpp's
HEADER = struct.Struct("<QiIQQQQQQQII16x")            # magic min_q exclude done bam stream n_chunks n_blocks index_off n_records n_ref names_bytes
CHUNK = struct.Struct("<QQQQIIII")                    # magic seq stream_off bytes n n_words n_runs 0
assert HEADER.size == 96 and CHUNK.size == 48
CHUNK_ARRAYS = (("hash", np.uint64), ("start", np.uint32), ("rbytes", np.uint32), ("len", np.uint32), ("word_off", np.uint32),
                ("codes", np.uint64), ("good", np.uint32), ("runs", np.uint32))


def _pad8(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 8)


def header_bytes(c, done=True) -> bytes:
    names = b"".join(n + b"\0" for n in c["names"])
    return HEADER.pack(FILE_MAGIC, c["min_q"], c["exclude_flags"], DONE_MAGIC if done else 0, c["bam_bytes"], c["stream_bytes"],
                       len(c["chunks"]), len(c["blocks"]), c["index_off"], sum(len(ch["hash"]) for ch in c["chunks"]), len(c["names"]),
                       len(names))


def chunk_bytes(seq, ch) -> bytes:
    n, w, r = len(ch["hash"]), len(ch["codes"]), len(ch["runs"]) // 2
    assert len(ch["word_off"]) == n + 1 and len(ch["good"]) == w
    body = b"".join(_pad8(np.ascontiguousarray(ch[k], dtype=t).tobytes()) for k, t in CHUNK_ARRAYS)
    return CHUNK.pack(CHUNK_MAGIC, seq, ch["stream_off"], CHUNK.size + len(body), n, w, r, 0) + body


def write(c) -> bytes:
    """c: {min_q, exclude_flags, names [bytes], chunks [{stream_off, hash, start, rbytes, len, word_off, codes, good, runs
    (flat: first kept index, refID as uint32, ...)}], blocks [(csize, isize)]}; bam_bytes, stream_bytes and index_off are
    computed here."""
    c = dict(c)
    names = _pad8(b"".join(n + b"\0" for n in c["names"]))
    chunks = b"".join(chunk_bytes(i, ch) for i, ch in enumerate(c["chunks"]))
    c["index_off"] = HEADER.size + len(names) + len(chunks)
    c["bam_bytes"] = sum(cs for cs, _ in c["blocks"])
    c["stream_bytes"] = sum(n for _, n in c["blocks"])
    index, fo, so = [struct.pack("<QQ", INDEX_MAGIC, len(c["blocks"]))], 0, 0
    for cs, n in c["blocks"]:
        index.append(struct.pack("<QQII", fo, so, cs, n))
        fo, so = fo + cs, so + n
    h = header_bytes(c)
    return h + names + chunks + b"".join(index) + h


def read(blob: bytes):
    """The parts of a cache, by the description alone; AssertionError where it is not one."""
    assert len(blob) >= 2 * HEADER.size and len(blob) % 8 == 0
    (magic, min_q, exclude, done, bam_bytes, stream_bytes, n_chunks, n_blocks, index_off, n_records, n_ref,
     names_bytes) = HEADER.unpack_from(blob, 0)
    assert magic == FILE_MAGIC and done == DONE_MAGIC and blob[:HEADER.size] == blob[-HEADER.size:]
    names = blob[HEADER.size:HEADER.size + names_bytes].split(b"\0")
    assert names[-1] == b"" and len(names) - 1 == n_ref
    at = HEADER.size + names_bytes + (-names_bytes % 8)
    chunks = []
    while at < index_off:
        cm, seq, stream_off, nbytes, n, w, r, zero = CHUNK.unpack_from(blob, at)
        assert cm == CHUNK_MAGIC and seq == len(chunks) and zero == 0
        ch, o = {"stream_off": stream_off}, at + CHUNK.size
        for k, t in CHUNK_ARRAYS:
            count = {"word_off": n + 1, "codes": w, "good": w, "runs": 2 * r}.get(k, n)
            ch[k] = np.frombuffer(blob, t, count, o).copy()
            o += count * np.dtype(t).itemsize
            o += -o % 8
        assert o == at + nbytes
        chunks.append(ch)
        at = o
    assert at == index_off and len(chunks) == n_chunks and sum(len(c["hash"]) for c in chunks) == n_records
    im, nb = struct.unpack_from("<QQ", blob, index_off)
    assert im == INDEX_MAGIC and nb == n_blocks and index_off + 16 + 24 * n_blocks + HEADER.size == len(blob)
    blocks, fo, so = [], 0, 0
    for i in range(n_blocks):
        f, s, cs, n = struct.unpack_from("<QQII", blob, index_off + 16 + 24 * i)
        assert (f, s) == (fo, so)
        blocks.append((cs, n))
        fo, so = fo + cs, so + n
    assert (fo, so) == (bam_bytes, stream_bytes)
    return {"min_q": min_q, "exclude_flags": exclude, "names": names[:-1], "chunks": chunks, "blocks": blocks, "bam_bytes": bam_bytes,
            "stream_bytes": stream_bytes, "index_off": index_off}


def same(a, b) -> bool:
    if any(a[k] != b[k] for k in ("min_q", "exclude_flags", "names", "blocks")) or len(a["chunks"]) != len(b["chunks"]):
        return False
    return all(x["stream_off"] == y["stream_off"] and all(np.array_equal(x[k], np.asarray(y[k], dtype=t)) for k, t in CHUNK_ARRAYS)
               for x, y in zip(a["chunks"], b["chunks"]))


# ---- what a fetch plan must satisfy ------------------------------------------------------------------------------------
def blocks_of(isizes, off, nbytes):
    """Brute force: the blocks (of ISIZE > 0) that hold any byte of [off, off + nbytes)."""
    out, at = [], 0
    for i, n in enumerate(isizes):
        if n and at < off + nbytes and off < at + n:
            out.append(i)
        at += n
    return out


def check_plan(isizes, sel, capacity, batches, stream: bytes):
    """batches: [(inflated, first, n, [block index], [arena offset])] as the product planned them for the records `sel`
    [(stream offset, bytes)] over blocks that inflate to `isizes` bytes each; `stream`: the concatenated inflated bytes."""
    starts = np.concatenate([[0], np.cumsum(isizes)])
    at = 0
    for inflated, first, n, blocks, offs in batches:
        assert first == at and n >= 1 and len(offs) == n
        assert blocks == sorted(set(blocks)) and all(isizes[k] for k in blocks)
        assert inflated == sum(isizes[k] for k in blocks) <= capacity
        arena = b"".join(stream[starts[k]:starts[k + 1]] for k in blocks)
        want = set()
        for (off, nbytes), a in zip(sel[first:first + n], offs):
            mine = blocks_of(isizes, off, nbytes)
            want.update(mine)
            j = blocks.index(mine[0])
            assert blocks[j:j + len(mine)] == mine           # every one of its blocks, side by side
            assert arena[a:a + nbytes] == stream[off:off + nbytes]
        assert want == set(blocks)                            # and no block that no record of the batch needs
        at += n
    assert at == len(sel)
