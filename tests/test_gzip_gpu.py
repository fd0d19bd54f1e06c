"""GPU: plain gzip inflated on the device (rfx_text_append_gzip; k_gz_find / k_gz_walk / k_gz_inflate / k_gz_windows /
k_gz_resolve / k_gz_crc, rufus_amd/csrc/rfx_gzip.hip) into the text arena of K1.

The corpus, the refusals and the truths are those of tests/gzip_ref.py (zlib's bytes; zlib's own Z_BLOCK walk for the block
starts).  The same bytes have passed tests/test_gzip_host.py in the host harness under the sanitizers first (the decoder core
and the chain rule are one source for both): run that file first, and do not re-run this one to look at a fault again."""
import pytest

from rufus_amd import capi
from tests import gzip_ref as G

pytestmark = pytest.mark.gpu
MiB = 1 << 20
GUARD = bytes((i * 37 + 11) & 255 for i in range(4096))


def inflate(ctx, gz, arena_bytes, piece):
    """(text, stats, confirmed starts, arenas used): `gz` through rfx_text_append_gzip in pieces of `piece` bytes, presented
    again from `consumed`; a full arena is fetched and reset.  Every arena begins with guard bytes and ends with what fits of them."""
    cap = arena_bytes + len(GUARD)
    arena = capi.TextArena(ctx, cap)
    out, arenas = [], 0

    def empty():
        nonlocal arenas
        tail = GUARD[::-1][:cap - arena.bytes]  # (what fits behind the text)
        arena.append(tail)
        got = arena.fetch()
        assert got[:len(GUARD)] == GUARD and got[len(got) - len(tail):] == tail
        out.append(got[len(GUARD):len(got) - len(tail)])
        arena.reset()
        arena.append(GUARD)
        arenas += 1

    try:
        with capi.GzipStream(ctx) as s:
            arena.append(GUARD)
            at = 0
            while at < len(gz):
                n = min(piece, len(gz) - at)
                got, used = s.append(arena, gz[at:at + n], at + n == len(gz))
                assert used <= n and arena.bytes <= cap
                at += used
                if got or used:
                    continue
                if s.need():
                    assert s.need() > cap - arena.bytes  # it really did not fit
                    empty()
                else:
                    assert n < len(gz) - at
                    piece *= 2
            empty()
            return b"".join(out), s.stats(), s.starts(), arenas
    finally:
        arena.close()


@pytest.mark.parametrize("chunk,arena_bytes,piece", [(1024, MiB, 100000), (16384, MiB, 100000), (8 * MiB, 4 * MiB, 1000000)])
def test_corpus_inflates_like_zlib(ctx, monkeypatch, chunk, arena_bytes, piece):
    """Arenas of 1 MiB: the 3.6 MB text crosses arenas and batches and the window buffer carries the history; pieces of
    100 000 bytes end inside a block.  A chunk above the file size makes every member ONE chunk (it must fit an arena)."""
    monkeypatch.setenv("RFX_GZIP_CHUNK", str(chunk))
    for name, data, gz in G.corpus():
        text, st, starts, arenas = inflate(ctx, gz, arena_bytes, piece)
        assert text == data, name
        assert st["bytes"] == len(data) and st["confirmed"] == len(starts) and st["members"] == (3 if name == "three_members" else 1), name
        if name == "fastq_l6":
            assert arenas >= (4 if chunk < MiB else 1) and st["batches"] >= arenas
        if name in ("fixed", "stored"):
            assert st["found"] == 0 and st["confirmed"] == 1, name  # no candidate anywhere: one chunk
        if name == "planted" and chunk == 1024:
            assert st["dropped"] >= 1
        if chunk > MiB and name != "planted":
            assert st["confirmed"] == st["members"], name


def test_speculation_really_happened(ctx, monkeypatch):
    """Level-6 text, 64 KiB chunks: every confirmed chunk start is one of zlib's true block starts, and at least three in
    four of the nominal boundaries with a true non-final dynamic start before the next boundary gave a confirmed chunk."""
    monkeypatch.setenv("RFX_GZIP_CHUNK", "65536")
    name, data, gz = G.corpus()[0]
    assert name == "fastq_l6"
    text, st, starts, _ = inflate(ctx, gz, 8 * MiB, len(gz))
    assert text == data
    truth = G.file_block_starts(gz)
    assert set(starts) <= {b for b, _, _ in truth}
    dyn = [b for b, f, t in truth if f == 0 and t == 2]
    cb = 65536 * 8
    boundaries = [k for k in range(-(-len(gz) * 8 // cb)) if any(k * cb <= b < (k + 1) * cb for b in dyn)]
    assert len(boundaries) >= 15
    assert st["confirmed"] >= 0.75 * len(boundaries) and st["confirmed"] == len(starts)
    assert st["rounds"] <= 3 and st["batches"] == 1


def test_refusals_are_format_errors(ctx, monkeypatch):
    monkeypatch.setenv("RFX_GZIP_CHUNK", "16384")
    for name, gz in G.refusals():
        with pytest.raises(capi.RufusError, match=r"\(-8\) rfx_gzip: member "):
            inflate(ctx, gz, MiB, 50000)
    # a chunk larger than an empty arena
    with pytest.raises(capi.RufusError, match=r"\(-8\) rfx_gzip: member 0, chunk 0: a chunk of 3145728 inflated bytes does not fit"):
        inflate(ctx, G.member(b"A" * (3 * MiB)), MiB, 50000)
    # the context goes on to inflate a good file
    name, data, gz = G.corpus()[1]
    assert inflate(ctx, gz, 2 * MiB, 200000)[0] == data


def test_seeded_damage_is_refused_or_inflates_like_zlib(ctx, monkeypatch):
    monkeypatch.setenv("RFX_GZIP_CHUNK", "1024")
    passed = 0
    for name, gz, want in G.seeded_damage(60):
        try:
            text = inflate(ctx, gz, MiB, 9000)[0]
        except capi.RufusError as e:
            assert "(-8) rfx_gzip:" in str(e), name
            continue
        assert want is not None and text == want, name
        passed += 1
    assert passed < 10


def test_tools_count_reads_plain_gzip(ctx):
    from rufus_amd import tools
    big = G.big_text()
    lines = big[:600000].split(b"\n")
    text = b"\n".join(lines[:(len(lines) - 1) // 4 * 4]) + b"\n"
    a = tools.jellyfish_count(ctx, [text], 25, 1 << 22)
    b = tools.jellyfish_count(ctx, [G.member(text[:250000], fname=b"r.fastq") + G.member(text[250000:], level=9)], 25, 1 << 22)
    assert tools.jellyfish_dump(a) == tools.jellyfish_dump(b) and len(tools.jellyfish_dump(a)) > 100000
