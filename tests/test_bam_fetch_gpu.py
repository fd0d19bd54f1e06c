"""GPU, C-ABI through capi: a kept record's address (rfx_bam_locate), records fetched by address out of BGZF blocks that
were inflated out of context (rfx_bam_fetch), and the mark of an array of hashes against a name set (rfx_nameset_mark).
The reference is plain Python over tests/bam_ref.py's reader: Bam.starts, slices of Bam.data, a Python set.  Fails without
the feature: the entry points do not exist."""
import struct

import numpy as np
import pytest

from rufus_amd import capi, tools
from tests import bam_ref as R
from tests import bgzf_ref as B

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def bams():
    out = {"synthetic": R.Bam(R.synthetic()), "adversarial": R.Bam(R.adversarial())}
    for name in ("Child", "Mother", "Father"):
        out[name] = R.Bam(R.fixture(name))
    return out


# ---- rfx_bam_locate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [None, "256"])
@pytest.mark.parametrize("exclude", [3328, 0])
@pytest.mark.parametrize("name", ["synthetic", "adversarial", "Child", "Mother", "Father"])
def test_locate_gives_every_kept_record_its_arena_offset_and_size(ctx, bams, monkeypatch, name, exclude, tile):
    bam = bams[name]
    if tile:
        monkeypatch.setenv("RFX_BAM_TILE", tile)
    kept = bam.kept(exclude)
    want_start = np.array([r["start"] for r in kept], np.int64)
    want_bytes = np.array([4 + struct.unpack_from("<I", bam.data, r["start"])[0] for r in kept], np.int64)
    for arena_bytes in (64 << 20, 1 << 20):
        hdr = capi.bam_header(bam.bam)
        first = [i for i, at in enumerate(np.cumsum([0] + [len(b) for b in B.split(bam.bam)])) if at == hdr["first_block"]][0]
        base, at, n_arenas = bam.block_starts[first], 0, 0
        for a, n_rec, _ in tools._bam_arenas(ctx, bam.bam, arena_bytes):
            # a settled arena ends with its last whole record: its kept records are those that start in front of its end
            in_arena = int(np.searchsorted(want_start, base + a.bytes) - at)
            assert len(a.bam_name_hashes(in_arena, exclude_flags=exclude)) == in_arena  # (the arena's own kept count)
            start, nbytes = a.bam_locate(in_arena, exclude)
            assert np.array_equal(start.astype(np.int64), want_start[at:at + in_arena] - base)
            assert np.array_equal(nbytes.astype(np.int64), want_bytes[at:at + in_arena])
            for wrong in (in_arena + 1, in_arena - 1):
                if wrong >= 0:
                    with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_locate"):
                        a.bam_locate(wrong, exclude)
            at += in_arena
            base += a.bytes
            n_arenas += 1
        assert at == len(kept)
        assert n_arenas == 1 if len(bam.data) < arena_bytes else n_arenas >= 2


def test_locate_refuses_an_unsettled_arena(ctx, bams):
    bam = bams["synthetic"]
    hdr = capi.bam_header(bam.bam)
    a = capi.TextArena(ctx, len(bam.data) + 65536)
    a.append_bgzf(bam.bam[hdr["first_block"]:])
    with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_locate"):
        a.bam_locate(5)
    a.close()


# ---- rfx_bam_fetch ----------------------------------------------------------------------------------------------------
CUT = 1024


@pytest.fixture(scope="module")
def sparse(bams):
    """The stream of synthetic() re-cut into blocks of 1024 bytes; the arena's blocks are every third one plus the
    successors a chosen record (one that starts in an every-third block) runs into.  -> (compressed bytes of the subset,
    inflated bytes of the subset, [(arena offset, bytes, the record's bytes)] of the chosen records, the blocks)."""
    bam = bams["synthetic"]
    blocks = B.split(B.write(bam.data, cut=CUT))[:-1]  # (without the EOF marker)
    ends = bam.starts[1:] + [len(bam.data)]
    chosen = [(s, e) for s, e in zip(bam.starts, ends) if (s // CUT) % 3 == 0]
    take = set(range(0, len(blocks), 3))
    for s, e in chosen:
        take.update(range(s // CUT, (e - 1) // CUT + 1))
    order = sorted(take)
    arena_off, at = {}, 0
    for i in order:
        arena_off[i] = at
        at += len(bam.data[i * CUT:(i + 1) * CUT])
    inflated = b"".join(bam.data[i * CUT:(i + 1) * CUT] for i in order)
    recs = [(arena_off[s // CUT] + s % CUT, e - s, bam.data[s:e]) for s, e in chosen]
    for off, n, raw in recs:
        assert inflated[off:off + n] == raw  # (a chosen record's blocks are adjacent in the arena)
    assert len(order) < len(blocks) and any((e - 1) // CUT - s // CUT >= 2 for s, e in chosen)
    return b"".join(blocks[i] for i in order), inflated, recs, [blocks[i] for i in order]


def _residue_list(recs):
    """The chosen records in an order whose (source residue, destination residue) pairs are all 16: while a pair is missing,
    the next record is one that adds a pair at the current destination residue, else the shortest record that moves the
    residue; then the rest in file order."""
    missing = {(s, d) for s in range(4) for d in range(4)}
    order, used, dst = [], set(), 0
    by_len = sorted(range(len(recs)), key=lambda i: recs[i][1])
    while missing and len(order) < 400:
        pick = next((i for i in range(len(recs)) if i not in used and (recs[i][0] % 4, dst % 4) in missing), None)
        if pick is None:
            pick = next(i for i in by_len if recs[i][1] % 4 and i not in used)
        used.add(pick)
        missing.discard((recs[pick][0] % 4, dst % 4))
        order.append(pick)
        dst += recs[pick][1]
    assert not missing
    return order + [i for i in range(len(recs)) if i not in used]


def _fetch(a, recs, idx, cap_delta=0, start=None, nbytes=None):
    """(rc, bytes reported, the buffer between the guards, guards untouched)."""
    st = np.array([recs[i][0] for i in idx], np.uint32) if start is None else start
    nb = np.array([recs[i][1] for i in idx], np.uint32) if nbytes is None else nbytes
    total = int(np.array([recs[i][1] for i in idx], np.int64).sum())
    buf = np.full(GUARD + max(total, 1) + GUARD, FILL, np.uint8)
    rc, got = a.bam_fetch_into(st, nb, buf[GUARD:GUARD + max(total, 1)], cap=total + cap_delta)
    guards = bool((buf[:GUARD] == FILL).all() and (buf[GUARD + total:] == FILL).all())
    return rc, got, buf[GUARD:GUARD + total].tobytes(), guards


def test_fetch_out_of_blocks_inflated_out_of_context(ctx, sparse):
    comp, inflated, recs, _ = sparse
    assert {r[0] % 4 for r in recs} == {0, 1, 2, 3}
    a = capi.TextArena(ctx, len(inflated) + 65536)
    a.append_bgzf(comp)  # never settled: the subset is no BAM stream
    order = _residue_list(recs)
    assert a.bytes == len(inflated)
    lists = {"0": [], "1": order[:1], "64": order[:64], "65": order[:65], "all": order,
             "duplicates": [order[0], order[0], order[1], order[0]] + order[:10] + order[:10],
             "descending": sorted(range(len(recs)), reverse=True)}
    for key, idx in lists.items():
        want = b"".join(recs[i][2] for i in idx)
        rc, got, out, guards = _fetch(a, recs, idx)
        assert (rc, got) == (0, len(want)) and out == want and guards, key
        if idx:  # one byte short: the need, nothing written
            rc, got, out, guards = _fetch(a, recs, idx, cap_delta=-1)
            assert (rc, got) == (capi.E_RANGE, len(want)) and out == bytes([FILL]) * len(want) and guards, key
    assert a.bam_fetch(np.array([recs[i][0] for i in order[:5]]), np.array([recs[i][1] for i in order[:5]])) == \
        b"".join(recs[i][2] for i in order[:5])
    # an entry that is no record: the lowest failing index is named, nothing is written
    idx = order[:70]
    st0 = np.array([recs[i][0] for i in idx], np.uint32)
    nb0 = np.array([recs[i][1] for i in idx], np.uint32)
    for what, at, edit in (("bytes + 1", (7, 66), lambda s, n, i: n.__setitem__(i, n[i] + 1)),
                           ("bytes - 1", (65, 69), lambda s, n, i: n.__setitem__(i, n[i] - 1)),
                           ("bytes = 35", (0, 3), lambda s, n, i: n.__setitem__(i, 35)),
                           ("one byte beyond the arena", (64, 68), lambda s, n, i: s.__setitem__(i, a.bytes - int(n[i]) + 1)),
                           ("the start beyond the arena", (5,), lambda s, n, i: s.__setitem__(i, a.bytes + 1))):
        st, nb = st0.copy(), nb0.copy()
        for i in at:
            edit(st, nb, i)
        rc, _, out, guards = _fetch(a, recs, idx, start=st, nbytes=nb)
        msg = capi.lib().rfx_last_error().decode()
        assert rc == capi.E_FORMAT and msg.startswith("rfx_bam_fetch: entry %d " % min(at)), (what, rc, msg)
        assert out == bytes([FILL]) * len(out) and guards, what
    a.close()


def test_fetch_a_record_at_the_arenas_first_byte_wherever_it_stands_in_the_list(ctx):
    """A block that begins with a record: its arena offset is 0, and it follows other records in the list."""
    rng = np.random.default_rng(5)
    raws = [R.record(b"n%d" % i, 0, -1, i, [], "ACGT"[:1 + i % 4] * (3 + i), bytes(rng.integers(0, 40, (1 + i % 4) * (3 + i), dtype=np.uint8)))
            for i in range(9)]
    data = b"".join(raws)
    offs = np.cumsum([0] + [len(r) for r in raws])
    recs = [(int(offs[i]), len(raws[i]), raws[i]) for i in range(len(raws))]
    a = capi.TextArena(ctx, 1 << 20)
    a.append_bgzf(B.write(data, cut=300, eof=False))
    for idx in ([0], [1, 0], [2, 0, 0, 3, 0], [8, 7, 6, 5, 4, 3, 2, 1, 0], [0] * 5):
        want = b"".join(recs[i][2] for i in idx)
        rc, got, out, guards = _fetch(a, recs, idx)
        assert (rc, got) == (0, len(want)) and out == want and guards, idx
    a.close()


def test_fetch_reports_a_block_that_did_not_inflate(ctx, sparse):
    _, inflated, recs, blocks = sparse
    bad = bytearray(blocks[1])
    bad[18 + len(B.parts(blocks[1])[1]) // 2] ^= 0x5A  # a payload byte
    a = capi.TextArena(ctx, len(inflated) + 65536)
    a.append_bgzf(blocks[0] + bytes(bad) + b"".join(blocks[2:]))
    buf = np.full(recs[0][1], FILL, np.uint8)
    rc, _ = a.bam_fetch_into(np.array([recs[0][0]], np.uint32), np.array([recs[0][1]], np.uint32), buf)
    assert rc == capi.E_FORMAT and "rfx_bgzf: block 1" in capi.lib().rfx_last_error().decode()
    assert (buf == FILL).all()
    a.close()


# ---- rfx_nameset_mark -------------------------------------------------------------------------------------------------
def _mask_of(hashes, members):
    m = np.zeros((len(hashes) + 63) // 64, np.uint64)
    hit = np.flatnonzero(np.isin(hashes, np.array(sorted(members), np.uint64)))
    np.bitwise_or.at(m, hit >> 6, np.uint64(1) << (hit & 63).astype(np.uint64))
    return m, len(hit)


@pytest.mark.parametrize("piece", [None, "64", "4096"])
def test_nameset_mark_equals_set_membership(ctx, monkeypatch, piece):
    if piece:
        monkeypatch.setenv("RFX_NAMESET_PIECE", piece)
    rng = np.random.default_rng(11)
    top = np.uint64(2**64 - 1)
    pool = rng.integers(1, 2**63, 6000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    sets = {"one": pool[:1], "5000": pool[:5000], "5000 with 0 and 2^64 - 1": np.concatenate([pool[:4998], [np.uint64(0), top]]),
            "only 0": np.zeros(1, np.uint64), "empty": pool[:0]}
    for key, members in sets.items():
        ns = capi.NameSet(ctx, members)
        want_set = set(members.tolist())
        for n in (0, 1, 63, 64, 65, 70000):
            hashes = pool[rng.integers(0, len(pool), n)] if n else pool[:0]
            if n >= 63:  # the two extreme values as queries, at the piece's and the word's edges
                hashes[[0, n // 2, n - 1]] = np.array([0, 2**64 - 1, 0], np.uint64)
                hashes[62] = top
            elif n == 1:
                hashes[0] = members[0] if len(members) else 0
            mask, marked = ns.mark(hashes)
            want, n_want = _mask_of(hashes, want_set)
            assert marked == n_want and np.array_equal(mask, want), (key, n)
        ns.free()
