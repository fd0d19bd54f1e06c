"""GPU: the text of selected records gathered on the device (rfx_text_gather: k_gather_sizes / _table / _copy,
rufus_amd/csrc/rfx_gather.hip), the record count and the cut at a given record of a text arena (rfx_text_records,
rfx_text_settle_records), and two mates' arenas kept in lock step with them -- all through rufus_amd.capi.TextArena.

Ground truth is Python: a join of the selected records, slices of the text, the host packer."""
import numpy as np
import pytest

from rufus_amd import capi
from tests import bgzf_ref as B
from tests import filter_bgzf_ref as F
from tests.test_bgzf_gpu import _fastq, _records

pytestmark = pytest.mark.gpu
GUARD = 0xA5


def ragged_records(rng, n):
    """Four lines per record and nothing else: header 2 .. 40 bytes, sequence 0 .. 300, some lines end in \\r\\n; with five
    records or more, one of 70 000 bases and one of four empty lines."""
    out = []
    for i in range(n):
        head = b"@" + bytes(rng.integers(48, 123, int(rng.integers(1, 40)), dtype=np.uint8))
        L = int(rng.integers(0, 301))
        seq = bytes(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)])
        qual = bytes(rng.integers(33, 75, L, dtype=np.uint8))
        eol = b"\r\n" if rng.random() < 0.2 else b"\n"
        out.append(head + eol + seq + eol + b"+" + eol + qual + eol)
    if n >= 5:
        out[2] = b"@long\n" + b"ACGT" * 17500 + b"\n+\n" + b"I" * 70000 + b"\n"
        out[4] = b"\n\n\n\n"
    return out


def mask_of(bits, n, garbage=False):
    w = np.zeros((n + 63) // 64, np.uint64)
    for r in np.flatnonzero(bits):
        w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    if garbage and n & 63:
        w[-1] |= ~((np.uint64(1) << np.uint64(n & 63)) - np.uint64(1))
    return w


def residues(recs, bits):
    """{(source start mod 4, destination start mod 4)} of the selected records."""
    src = np.concatenate([[0], np.cumsum([len(r) for r in recs])])[:-1]
    seen, dst = set(), 0
    for r in np.flatnonzero(bits):
        seen.add((int(src[r]) & 3, dst & 3))
        dst += len(recs[r])
    return seen


def gather_checked(arena, recs, bits, garbage=False):
    """One gather against the join; guard bytes behind the result, and a buffer one byte short."""
    n = len(recs)
    want = b"".join(recs[r] for r in np.flatnonzero(bits))
    mask = mask_of(bits, n, garbage)
    out = np.full(len(want) + 64, GUARD, np.uint8)
    rc, nb, ns = arena.gather_into(mask, n, out)
    assert (rc, nb, ns) == (0, len(want), int(np.count_nonzero(bits)))
    assert out[:nb].tobytes() == want
    assert (out[nb:] == GUARD).all()
    if want:
        out[:] = GUARD
        rc, nb, _ = arena.gather_into(mask, n, out, cap=len(want) - 1)
        assert (rc, nb) == (capi.E_RANGE, len(want)) and (out == GUARD).all()
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4000])
def test_gather_equals_a_join_of_the_selected_records(ctx, n):
    rng = np.random.default_rng(100 + n)
    recs = ragged_records(rng, n)
    text = b"".join(recs)
    arena = capi.TextArena(ctx, len(text) + 4096)
    arena.append(text[:len(text) // 2])
    arena.append(text[len(text) // 2:])
    assert arena.records() == n
    masks = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": np.arange(n) == 0, "last": np.arange(n) == n - 1,
             "alternating": np.arange(n) % 2 == 1, "random": rng.random(n) < 0.01, "half": rng.random(n) < 0.5}
    seen, lengths = set(), set()
    for name, bits in masks.items():
        want = gather_checked(arena, recs, bits)
        seen |= residues(recs, bits)
        lengths.add(len(want) & 3)
    gather_checked(arena, recs, np.ones(n, bool), garbage=True)  # all ones, and ones at and above n
    assert lengths - {0}  # an output that is no whole number of dwords
    if n >= 129:
        assert len(seen) == 16, sorted(seen)  # every source residue against every destination residue
    assert arena.gather(mask_of(masks["half"], n), n) == b"".join(recs[r] for r in np.flatnonzero(masks["half"]))
    assert arena.fetch() == text  # the arena is as it was
    # the record count must be the arena's
    out = np.full(64, GUARD, np.uint8)
    for wrong in (n - 1, n + 1):
        rc, _, _ = arena.gather_into(mask_of(np.ones(max(wrong, 1), bool), max(wrong, 1)), wrong, out)
        assert rc == capi.E_INVAL and (out == GUARD).all()
    # an arena that ends inside a record: three more lines, then a fourth without its newline
    arena.append(b"@x\nAC\n+\n")
    rc, _, _ = arena.gather_into(mask_of(np.ones(n, bool), n), n, out)
    assert rc == capi.E_INVAL
    arena.append(b"II")
    rc, _, _ = arena.gather_into(mask_of(np.ones(n + 1, bool), n + 1), n + 1, out)
    assert rc == capi.E_INVAL and (out == GUARD).all()
    arena.append(b"\n")
    assert arena.gather(mask_of(np.arange(n + 1) == n, n + 1), n + 1) == b"@x\nAC\n+\nII\n"
    arena.close()


def test_gather_after_a_parse_equals_gather_without(ctx):
    rng = np.random.default_rng(7)
    names, seqs, quals = _records(rng, 3000)
    recs = _fastq(names, seqs, quals)
    bits = rng.random(len(recs)) < 0.05
    mask = mask_of(bits, len(recs))
    arena = capi.TextArena(ctx, sum(map(len, recs)) + 64)
    arena.append_bgzf(B.write(b"".join(recs), 1))
    before = arena.gather(mask, len(recs))
    blk = arena.parse(capi.PACK_FILTER, 15)
    assert blk is not None and blk.n == len(recs)
    after = arena.gather(mask, len(recs))
    blk.free()
    assert before == after == b"".join(recs[r] for r in np.flatnonzero(bits))
    arena.reset()
    assert arena.gather(np.zeros(1, np.uint64), 0) == b""  # an empty arena holds no record
    arena.close()


def _parses_like_the_host_packer(arena, seqs, quals, flags=capi.PACK_FILTER):  # (the comparison of tests/test_bgzf_gpu.py)
    blk = arena.parse(flags, 15)
    assert blk is not None and blk.n == len(seqs)
    ref = capi.PackedReads.from_reads(seqs, quals, 15, flags)
    got = blk.get(want_good=flags == capi.PACK_FILTER, want_acgt=flags == capi.PACK_COUNT)
    nw = int(ref.word_off[-1])
    assert np.array_equal(got["word_off"], ref.word_off) and np.array_equal(got["len"][:blk.n], ref.len[:blk.n])
    assert np.array_equal(got["codes"][:nw], ref.codes[:nw])
    key = "acgt" if flags == capi.PACK_COUNT else "good"
    assert np.array_equal(got[key][:nw], getattr(ref, key)[:nw])
    blk.free()


@pytest.fixture(scope="module")
def straddling():
    """(records, their sequences and qualities, text = R whole records and a piece of the next, the text's BGZF blocks)"""
    rng = np.random.default_rng(11)
    names, seqs, quals = _records(rng, 1501)
    recs = _fastq(names, seqs, quals)
    text = b"".join(recs)[:-(len(recs[-1]) // 2)]
    blocks = B.split(B.write(text, 1, eof=False))
    assert len(blocks) >= 3
    return recs, seqs, quals, text, blocks


@pytest.mark.parametrize("max_records", [0, 1, 1499, 1500, 1505])
def test_records_and_the_cut_at_a_given_record(ctx, straddling, max_records):
    recs, seqs, quals, text, blocks = straddling
    R = len(recs) - 1
    a, b = capi.TextArena(ctx, len(text) + 4096), capi.TextArena(ctx, len(text) + 4096)
    third = len(blocks) // 3
    for piece in (blocks[:third], blocks[third:2 * third], blocks[2 * third:]):
        a.append_bgzf(b"".join(piece))
    assert a.records() == R and a.fetch() == text and b.records() == 0
    kept = min(R, max_records)
    head = b"".join(recs[:kept])
    assert a.settle_records(b, max_records) == (kept, len(text) - len(head))
    assert a.fetch() == head and b.fetch() == text[len(head):]
    assert a.records() == kept and b.records() == R - kept
    if kept:
        _parses_like_the_host_packer(a, seqs[:kept], quals[:kept])
    else:
        assert a.bytes == 0
    b.append(b"".join(recs)[len(text):])  # the rest of the last record
    _parses_like_the_host_packer(b, seqs[kept:], quals[kept:], capi.PACK_COUNT)
    with pytest.raises(capi.RufusError, match=r"\(-2\)"):  # `next` must be empty
        a.settle_records(b, 1)
    a.close(), b.close()


def test_settle_is_what_it_was(ctx, straddling):
    recs, seqs, quals, text, blocks = straddling
    R = len(recs) - 1
    a, b = capi.TextArena(ctx, len(text) + 4096), capi.TextArena(ctx, len(text) + 4096)
    a.append_bgzf(b"".join(blocks))
    head = b"".join(recs[:R])
    assert a.settle(b) == len(text) - len(head) and a.fetch() == head and b.fetch() == text[len(head):]
    with pytest.raises(capi.RufusError, match=r"\(-8\).*inside a record"):
        b.settle(None)
    with pytest.raises(capi.RufusError, match=r"\(-8\).*inside a record"):
        b.settle_records(None, 5)
    _parses_like_the_host_packer(a, seqs[:R], quals[:R])
    a.close(), b.close()


def test_two_mates_in_lock_step_equal_one_arena_per_mate(ctx):
    """The step of the executable's BGZF route, at the API: arenas of 256 KiB, mates whose records differ in length (mate 1's
    are the longer ones in the first half of the files, mate 2's in the second), so every step but the
    last cuts at the smaller count."""
    genome, m1, m2 = F.ragged_pairs(6000, seed=9)
    half = len(m1) // 2
    m1 = [r.replace(b"/1\n", b"/1 " + b"x" * 200 + b"\n", 1) if i < half else r for i, r in enumerate(m1)]
    texts = [b"".join(m1), b"".join(m2)]
    keys = capi.hashlist_keys(F.hash_list(genome, 12), F.K)
    mset = capi.MutantSet(ctx, keys, F.K)

    def hit_mask(arena, n):
        blk = arena.parse(capi.PACK_FILTER, F.MIN_Q)
        assert blk is not None and blk.n == n
        _, mask, _ = mset.filter(blk, F.THRESH, True, want_hits=False)
        blk.free()
        return mask[:(n + 63) // 64].copy()

    # ground truth: each mate whole in one arena
    whole, truth_mask = [], None
    for t in texts:
        a = capi.TextArena(ctx, len(t) + 4096)
        a.append(t)
        whole.append(a)
        m = hit_mask(a, len(m1))
        truth_mask = m if truth_mask is None else truth_mask | m
    truth_bits = np.unpackbits(truth_mask.view(np.uint8), bitorder="little")[:len(m1)].astype(bool)
    truth = [a.gather(truth_mask, len(m1)) for a in whole]
    assert 3 <= truth_bits.sum() <= 150
    assert truth == [b"".join(m[r] for r in np.flatnonzero(truth_bits)) for m in (m1, m2)]
    for a in whole:
        a.close()

    cap = 256 << 10
    blocks = [B.split(B.write(t, 1)) for t in texts]
    at = [0, 0]
    arenas = [[capi.TextArena(ctx, cap), capi.TextArena(ctx, cap)] for _ in range(2)]

    def fill(m, arena):
        while at[m] < len(blocks[m]) and B.parts(blocks[m][at[m]])[3] <= cap - arena.bytes:
            arena.append_bgzf(blocks[m][at[m]])
            at[m] += 1

    cur, pairs, got, bits, smaller = 0, 0, [b"", b""], [], set()
    for m in range(2):
        fill(m, arenas[m][cur])
    while True:
        r = [arenas[m][cur].records() for m in range(2)]
        n = min(r)
        if n == 0:
            break
        if at != [len(blocks[0]), len(blocks[1])]:  # (with both files loaded to their ends, the two hold what is left of both)
            assert r[0] != r[1]
            smaller.add(int(r[1] < r[0]))
        for m in range(2):
            assert arenas[m][cur].settle_records(arenas[m][cur ^ 1], n)[0] == n
            fill(m, arenas[m][cur ^ 1])
        mask = hit_mask(arenas[0][cur], n) | hit_mask(arenas[1][cur], n)
        for m in range(2):
            got[m] += arenas[m][cur].gather(mask, n)
            arenas[m][cur].reset()
        bits.append(np.unpackbits(mask.view(np.uint8), bitorder="little")[:n].astype(bool))
        pairs += n
        cur ^= 1
    assert at == [len(blocks[0]), len(blocks[1])] and arenas[0][cur].bytes == 0 and arenas[1][cur].bytes == 0
    assert pairs == len(m1) and len(bits) >= 5 and smaller == {0, 1}
    assert np.array_equal(np.concatenate(bits), truth_bits) and got == truth
    for pair in arenas:
        for a in pair:
            a.close()
