"""CPU-only: the tile plan (``rfx_tile_plan`` / ``capi.tile_plan``) against a brute force.

A sequence of ``length`` bases is cut into tiles of at most L bases that start every step = L - k + 1 bases.  The count
kernels are exact on the tiled block only if every k-mer window of the sequence lies in exactly one tile, so that is what
is checked here, window by window, for every length of the grid."""
import numpy as np
import pytest

from rufus_amd import capi

KS = (1, 2, 5, 15, 25, 31, 32)
LENGTHS = tuple(range(700)) + (5000, 5003)


def tiles_of(length, k, L):
    """[(start, len)] of the plan, from the library's (n_tiles, step) and the stated tile geometry."""
    n, step = capi.tile_plan(length, k, L)
    assert step == L - k + 1
    if length <= L:
        assert n == 1
        return [(0, length)]
    return [(t * step, min(L, length - t * step)) for t in range(n)]


@pytest.mark.parametrize("k", KS)
def test_every_window_in_exactly_one_tile(k):
    for L in (k, k + 1, 33, 64, 150, 160):
        if L < k:
            continue
        for length in LENGTHS:
            tiles = tiles_of(length, k, L)
            n_win = max(0, length - k + 1)
            cover = np.zeros(n_win, np.int32)
            for start, tl in tiles:
                assert 0 <= tl <= L and start + tl <= length, (k, L, length, start, tl)
                if len(tiles) > 1:
                    assert tl >= k, (k, L, length, start, tl)
                if tl >= k:
                    cover[start:start + tl - k + 1] += 1
            assert (cover == 1).all(), (k, L, length)
            if length > L:       # the closed form of the plan
                assert len(tiles) == -(-(length - k + 1) // (L - k + 1))


def test_short_and_empty_sequences_are_one_tile():
    for k, L in ((25, 150), (32, 32), (5, 33)):
        for length in (0, 1, k - 1, k, L):
            assert capi.tile_plan(length, k, L) == (1, L - k + 1)


def test_overhead_at_the_default_geometry():
    # step 126 of 150: the tiled block of a long sequence holds 150 / 126 = 1.19 x the bases
    n, step = capi.tile_plan(10_000_000, 25, 150)
    assert step == 126
    assert abs(n * 150 / 10_000_000 - 150 / 126) < 1e-3


@pytest.mark.parametrize("k,L", [(0, 150), (-1, 150), (33, 150), (25, 24), (32, 31), (2, 1), (1, 0)])
def test_refusals(k, L):
    with pytest.raises(capi.RufusError):
        capi.tile_plan(1000, k, L)
    nt, step = capi.C.c_uint64(7), capi.C.c_uint32(7)
    assert capi.lib().rfx_tile_plan(1000, k, L, capi.C.byref(nt), capi.C.byref(step)) == capi.E_INVAL


def test_null_outputs_are_allowed():
    assert capi.lib().rfx_tile_plan(1000, 25, 150, None, None) == 0
