"""GPU, C-ABI through capi: the device side of `RUFUS.Filter --bam` -- the stranded filter pack (rfx_bam_parse_filter), the
QNAME hashes (rfx_bam_name_hashes), the mark against a set of hashes (rfx_nameset_build, rfx_bam_mark_names) and the gather
of the marked records (rfx_bam_gather) -- on bam_ref.synthetic(), bam_ref.adversarial(), the crafted file of
tests/filter_bam_ref.py and the Child fixture, with the whole file in one arena and cut into arenas of 1 MiB.  The reference
is plain Python over tests/bam_ref.py's reader: the host packer's arrays of the printed forms, the Python name hash, set
membership, slices of the inflated bytes.  tests/test_filter_bam_host.py runs the same per-base statements under the
sanitizers on the host.  Fails without the feature: the entry points do not exist."""
import numpy as np
import pytest

from rufus_amd import capi, tools
from tests import bam_ref as R
from tests import filter_bam_ref as FB

pytestmark = pytest.mark.gpu
ARENAS = {"one": 64 << 20, "1MiB": 1 << 20}
MIN_QS = (0, 15, 42)


@pytest.fixture(scope="module")
def files():
    """name -> (Bam, {MinQ: host-packed reference}, name hashes of the kept records, their raw bytes): made once, shared."""
    out = {}
    for name, blob in (("synthetic", R.synthetic()), ("crafted", FB.crafted()[0]), ("adversarial", R.adversarial()),
                       ("Child", R.fixture("Child"))):
        bam = R.Bam(blob)
        out[name] = (bam, {q: FB.packed(bam, q) for q in MIN_QS}, np.array([FB.name_hash(FB.qname(r)) for r in bam.kept()], np.uint64),
                     FB.record_slices(bam))
    return out


def _bits(idx, n):
    m = np.zeros((n + 63) // 64 or 1, np.uint64)
    for i in idx:
        m[i >> 6] |= np.uint64(1 << (i & 63))
    return m


NAMES = ["synthetic", "crafted", "adversarial", "Child"]


@pytest.mark.parametrize("arena", sorted(ARENAS))
@pytest.mark.parametrize("name", NAMES)
def test_parse_filter_equals_the_host_packer_of_the_printed_forms(ctx, files, name, arena):
    bam, packed, _, _ = files[name]
    L = capi.lib()
    for min_q in MIN_QS:
        want = packed[min_q]
        n, nw = len(bam.kept()), int(want.word_off[-1])
        lens, codes, good, runs, n_arenas = [], [], [], [], 0
        for a, _, _ in tools._bam_arenas(ctx, bam.bam, ARENAS[arena]):
            blk, r = a.bam_parse_filter(min_q)
            got = blk.get(want_good=True, want_acgt=False)
            assert np.array_equal(got["word_off"], np.concatenate([[0], np.cumsum((got["len"].astype(np.int64) + 31) // 32)]))
            assert int(L.rfx_reads_bases(blk._h)) == int(got["len"].sum()) and int(L.rfx_reads_words(blk._h)) == len(got["codes"])
            for l in range(32):
                assert int(L.rfx_reads_of_length(blk._h, l)) == int((got["len"] == l).sum())
            for first, ref in r.tolist():
                if not runs or runs[-1][1] != ref:
                    runs.append((len(np.concatenate(lens)) + first if lens else first, ref))
            lens.append(got["len"]), codes.append(got["codes"]), good.append(got["good"])
            blk.free()
            n_arenas += 1
        assert (n_arenas == 1) if arena == "one" or len(bam.data) < ARENAS[arena] else (n_arenas >= 2)
        assert np.array_equal(np.concatenate(lens), want.len[:n])
        assert np.array_equal(np.concatenate(codes), want.codes[:nw]) and np.array_equal(np.concatenate(good), want.good[:nw])
        assert runs == bam.runs()


@pytest.mark.parametrize("arena", sorted(ARENAS))
@pytest.mark.parametrize("name", NAMES)
def test_name_hashes_marks_and_gathers(ctx, files, name, arena):
    bam, _, hashes, slices = files[name]
    n_all = len(hashes)
    rng = np.random.default_rng(3)
    sets = {0: hashes[:0], 1: hashes[n_all // 2:n_all // 2 + 1], 37: hashes[rng.choice(n_all, 37, replace=False)], "all": hashes}
    nsets = {k: capi.NameSet(ctx, v) for k, v in sets.items()}
    assert len(nsets[0]) == 0 and len(nsets["all"]) == len(set(hashes.tolist()))
    base = 0
    for a, _, _ in tools._bam_arenas(ctx, bam.bam, ARENAS[arena]):
        m_all, n, marked = a.bam_mark_names(nsets["all"])
        assert marked == n and np.array_equal(m_all, _bits(range(n), n)[:len(m_all)])
        mine = hashes[base:base + n]
        assert np.array_equal(a.bam_name_hashes(n), mine)
        for sel in (range(0), range(0, n, 7), (0, n - 1)):
            assert np.array_equal(a.bam_name_hashes(n, _bits(sel, n)), mine[list(sel)])
        for key, hs in sets.items():
            members = set(hs.tolist())
            want = [i for i in range(n) if int(mine[i]) in members]
            mask, n_kept, marked = a.bam_mark_names(nsets[key])
            assert (n_kept, marked) == (n, len(want)) and np.array_equal(mask, _bits(want, n)[:len(mask)]), key
        for sel in (range(0), range(n), range(0, n, 7), (0, n - 1)):
            want = b"".join(slices[base + i] for i in sel)
            assert a.bam_gather(_bits(sel, n), n) == want
        # bits at and above the kept count are ignored; a buffer one byte short is refused with the need set
        junk = _bits((0, n - 1), n)
        if n & 63:
            junk[-1] |= np.uint64(1 << 63)
        want = slices[base] + (slices[base + n - 1] if n > 1 else b"")
        out = np.zeros(len(want), np.uint8)
        assert a.bam_gather_into(junk, n, out, cap=len(want) - 1) == (capi.E_RANGE, len(want), 1 + (n > 1)) and not out.any()
        assert a.bam_gather_into(junk, n, out) == (0, len(want), 1 + (n > 1)) and out.tobytes() == want
        base += n
    assert base == n_all
    for s in nsets.values():
        s.free()


def test_refusals_on_an_unsettled_arena_and_a_wrong_kept_count(ctx, files):
    bam = files["synthetic"][0]
    hdr = capi.bam_header(bam.bam)
    a = capi.TextArena(ctx, len(bam.data) + 65536)
    a.append_bgzf(bam.bam[hdr["first_block"]:])
    ns = capi.NameSet(ctx, np.array([1, 2, 3], np.uint64))
    with pytest.raises(capi.RufusError, match="rfx_bam_parse_filter: RFX_E_INVAL"):
        a.bam_parse_filter(15)
    for call, who in ((lambda: a.bam_name_hashes(5), "rfx_bam_name_hashes"), (lambda: a.bam_mark_names(ns), "rfx_bam_mark_names"),
                      (lambda: a.bam_gather(_bits((0,), 5), 5), "rfx_bam_gather")):
        with pytest.raises(capi.RufusError, match=r"\(-2\) " + who):
            call()
    n, _ = a.bam_settle(None, hdr["skip"], hdr["n_ref"])
    kept = len(bam.kept())
    assert n == len(bam.records) and kept < n
    with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_gather"):
        a.bam_gather(_bits((0,), n), n)  # the records, not the kept records
    with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_name_hashes"):
        a.bam_name_hashes(kept + 1)
    assert len(a.bam_name_hashes(kept)) == kept
    a.reset()
    with pytest.raises(capi.RufusError, match=r"\(-2\) rfx_bam_gather"):
        a.bam_gather(_bits((0,), kept), kept)  # reset: not settled any more
    # an arena none of whose records is kept, and an empty arena: valid, empty
    for recs in ([R.record(b"x%d" % i, 1024, 0, i, [("M", 4)], "ACGT", bytes([30] * 4)) for i in range(3)], []):
        a.reset()
        small = R.write(R.REFS, recs)
        hdr = capi.bam_header(small)
        a.append_bgzf(small[hdr["first_block"]:])
        assert a.bam_settle(None, hdr["skip"], hdr["n_ref"]) == (len(recs), 0)
        blk, runs = a.bam_parse_filter(15)
        assert blk.n == 0 and len(runs) == 0
        blk.free()
        assert a.bam_mark_names(ns)[1:] == (0, 0) and len(a.bam_name_hashes(0)) == 0
        assert a.bam_gather(np.zeros(1, np.uint64), 0) == b""
    ns.free()
    a.close()


def test_tools_filter_bam_equals_the_feeder_and_the_oracle(ctx):
    blob, hl, _ = FB.crafted()
    bam = R.Bam(blob)
    e1, e2, log, idx = FB.expected(bam, hl)
    assert len(idx) >= 20
    for arena in (64 << 20, 1 << 20):
        assert tools.filter_bam(ctx, blob, hl, FB.K, FB.MIN_Q, FB.THRESH, arena_bytes=arena) == (e1, e2, log)
    # a hash list that hits nothing: empty files, the log all the same
    absent = b"".join(b"ACGT"[i % 4:i % 4 + 1] * 25 + b" 7\n" for i in range(4))
    assert tools.filter_bam(ctx, blob, absent, FB.K, FB.MIN_Q, FB.THRESH, arena_bytes=1 << 20) == (b"", b"", log)
