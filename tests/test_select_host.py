"""CPU: the numpy statement of ``rfx_reads_select`` (tests/select_ref.py) against the host packer over the selected reads'
TEXT, brute force; its pair rule against the driver's ``wgs.pulled_pairs``; the three new names in the symbol table."""
import ctypes as C
import os

import numpy as np
import pytest

from rufus_amd import capi, tools, wgs
from tests import select_ref as ref
from tests.conftest import ROOT

MIN_Q = 15
FLAGS = capi.PACK_COUNT | capi.PACK_FILTER


@pytest.mark.parametrize("n", ref.READ_COUNTS)
def test_reference_selection_equals_the_packer_over_the_selected_text(n):
    rng = np.random.default_rng(1000 + n)
    seqs, quals = ref.ragged_reads(rng, n)
    whole = ref.packed_dict(capi.PackedReads.from_reads(seqs, quals, MIN_Q, FLAGS), n)
    if n >= 12:
        assert {len(s) for s in seqs} == set(ref.LENGTHS)
    for name, mask in ref.masks_for(rng, n).items():
        for pairs in (False, True):
            what = (n, name, pairs)
            got, origin = ref.select_packed(whole, n, mask, pairs)
            # which reads: from the definition, read by read
            bit = [bool((int(mask[r // 64]) >> (r % 64)) & 1) for r in range(n)]
            want_idx = [r for r in range(n) if bit[r] or (pairs and (r ^ 1) < n and bit[r ^ 1])]
            assert origin.tolist() == want_idx, what
            sel_s, sel_q = [seqs[r] for r in want_idx], [quals[r] for r in want_idx]
            want = ref.packed_dict(capi.PackedReads.from_reads(sel_s, sel_q, MIN_Q, FLAGS), len(want_idx))
            for key in ("codes", "acgt", "good", "word_off", "len"):
                assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)
            # and back to text: N where the ACGT bit is clear
            assert tools.decode_reads(got) == sel_s, what


def test_reference_selection_without_good_or_acgt():
    rng = np.random.default_rng(5)
    seqs, quals = ref.ragged_reads(rng, 65)
    mask = ref.masks_for(rng, 65)["random"]
    for flags, missing in ((capi.PACK_COUNT, "good"), (capi.PACK_FILTER, "acgt")):
        whole = ref.packed_dict(capi.PackedReads.from_reads(seqs, quals, MIN_Q, flags), 65)
        got, origin = ref.select_packed(whole, 65, mask, True)
        want = ref.packed_dict(capi.PackedReads.from_reads([seqs[r] for r in origin], [quals[r] for r in origin], MIN_Q, flags),
                               len(origin))
        assert got[missing] is None and want[missing] is None
        for key in ("codes", "acgt", "good", "word_off", "len"):
            if key != missing:
                assert got[key].tobytes() == want[key].tobytes(), (flags, key)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129, 1000, 1001])
def test_pair_rule_is_the_drivers(n):
    """popcount(effective mask) = 2 * pulled_pairs - (1 if the lone last read of an odd block is selected)."""
    rng = np.random.default_rng(n)
    for name, mask in ref.masks_for(rng, n).items():
        if "garbage" in name:
            continue                    # (pulled_pairs takes the mask as the filter leaves it, bit n included)
        eff = ref.effective_mask(mask, n, True)
        lone = n % 2 == 1 and bool((int(mask[(n - 1) // 64]) >> ((n - 1) % 64)) & 1)
        assert int(np.bitwise_count(eff).sum()) == 2 * wgs.pulled_pairs(mask, n) - (1 if lone else 0), (n, name)
        assert len(ref.selected_reads(mask, n, True)) == int(np.bitwise_count(eff).sum())


def test_the_three_entry_points_are_declared_and_exported():
    L = C.CDLL(capi.LIB_PATH)
    for name in ("rfx_reads_select", "rfx_reads_origin", "rfx_filter_pull"):
        assert name in capi.SIGNATURES, name
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "rufus_hip.h")).read()
    assert "RFX_SELECT_READS 0" in header and "RFX_SELECT_PAIRS 1" in header
    assert (capi.SELECT_READS, capi.SELECT_PAIRS) == (0, 1)
