"""GPU: the Python mirrors of the two commands with `region=` (rufus_amd/tools.py bam_read_blocks, filter_bam) on Child.bam,
without an index, with a fine and with a coarse one, in one arena and in arenas of 1 MiB: the count blocks must be the host
packer's of the SEQs of exactly the kept records of the region, and the filter's three outputs the oracle's pull over the
feeder's pairs of those records (tests/filter_bam_ref.py).  Fails without the feature: neither function takes `region`."""
import copy

import numpy as np
import pytest

from rufus_amd import capi, tools
from tests import bai_ref as X
from tests import bam_ref as R
from tests import filter_bam_ref as FB

pytestmark = pytest.mark.gpu
HL = R.GOLDEN + "/Child.k25_c5.HashList"


@pytest.fixture(scope="module")
def child():
    bam = R.Bam(R.fixture("Child"))
    return bam, {None: None, "fine": X.build(bam, "fine"), "coarse": X.build(bam, "coarse", "same")}


def _subset(bam, text):
    region = X.parse_region(text, [n for n, _ in bam.refs])
    sub = copy.copy(bam)
    sub.records = [r for r in bam.records if X.in_region(r, *region)]
    return sub


@pytest.mark.parametrize("arena", [256 << 20, 1 << 20])
@pytest.mark.parametrize("index", [None, "fine", "coarse"])
def test_read_blocks_of_a_region(ctx, child, index, arena):
    bam, indexes = child
    text = "5:177640001-177645000"
    seqs = _subset(bam, text).kept_seqs()
    assert len(seqs) == 1307
    assert capi.bam_region_parse(text, [n for n, _ in bam.refs]) == X.parse_region(text, [n for n, _ in bam.refs])
    done = 0
    for blk, _, _ in tools.bam_read_blocks(ctx, bam.bam, arena_bytes=arena, region=text, index=indexes[index]):
        try:
            part = seqs[done:done + blk.n]
            packed = capi.PackedReads.from_reads(part, flags=capi.PACK_COUNT)
            got = blk.get(want_good=False, want_acgt=True)
            nw = int(packed.word_off[-1])
            assert np.array_equal(got["word_off"], packed.word_off) and np.array_equal(got["codes"], packed.codes[:nw])
            done += blk.n
        finally:
            blk.free()
    assert done == len(seqs)


def test_bai_query_equals_the_reference(child):
    bam, indexes = child
    names = [n for n, _ in bam.refs]
    for text in ("5:177640001-177645000", "5", "5:1-1000", "1"):
        region = X.parse_region(text, names)
        for kind in ("fine", "coarse"):
            assert capi.bai_query(indexes[kind], len(bam.refs), len(bam.bam), *region) == X.query(X.parse(indexes[kind]), *region)
    with pytest.raises(capi.RufusError, match="n_ref"):
        capi.bai_query(indexes["fine"], len(bam.refs) + 1, len(bam.bam), 4, 0, 1000)
    with pytest.raises(capi.RufusError, match="region '7:1-2'"):
        capi.bam_region_parse("7:1-2", [b"5"])


@pytest.mark.parametrize("index", [None, "fine"])
def test_filter_bam_of_a_region(ctx, child, index):
    bam, indexes = child
    text = "5:177642801-177643000"
    hl = open(HL, "rb").read()
    e1, e2, log, idx = FB.expected(_subset(bam, text), hl)
    assert len(idx) >= 5 and len(idx) < len(FB.expected(bam, hl)[3])
    m1, m2, got_log = tools.filter_bam(ctx, bam.bam, hl, FB.K, FB.MIN_Q, FB.THRESH, arena_bytes=1 << 20, region=text, index=indexes[index])
    assert (m1, m2, got_log) == (e1, e2, log)
