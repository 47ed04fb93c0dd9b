"""The model of the connected components (tests/component_checkers.py) pinned on any host: the flood fill against the transitive
closure of the adjacency matrix, the symmetry of the move masks the rule relies on, and the CPU facts the GPU tests build on (the
components of the golden maps, the checkerboard, the split wall)."""
import itertools

import numpy as np
import pytest

import component_checkers as cc
import field_checkers as fc
import golden_io as gio
import thin_maps

GOLDEN = {   # name -> (components per policy in fc.POLICIES order, the sizes under (1, 1) from the largest down)
    "fig7": ((1, 1, 1, 1), [290]),
    "fig13": ((1, 1, 1, 1), [254]),
    "img1": ((2, 1, 2, 2), [281, 17]),
    "g128crop": ((3, 3, 3, 3), [11005, 152, 1]),
    "g256": ((10, 9, 10, 10), [46880, 603, 19, 14]),
}


def test_flood_fill_against_the_closure_on_every_small_grid():
    """Every 3 x 4 grid with at most 5 obstacles, the four policies: 1586 grids."""
    n = 0
    for k in range(6):
        for cells in itertools.combinations(range(12), k):
            g = np.zeros(12, np.uint8)
            g[list(cells)] = 1
            g = g.reshape(3, 4)
            for ad, rs in fc.POLICIES:
                lab, sizes, first = cc.flood_fill(g, ad, rs)
                assert np.array_equal(lab, cc.closure_labels(g, ad, rs)), (cells, ad, rs)
                assert np.array_equal(sizes, np.bincount(lab[lab >= 0], minlength=len(sizes))), (cells, ad, rs)
                assert all(first[l] == np.flatnonzero(lab.reshape(-1) == l)[0] for l in range(len(sizes))), (cells, ad, rs)
                assert np.all(np.diff(first) > 0)
            n += 1
    assert n == 1586


def all_test_maps():
    maps = [gio.grid(name)[0] for name in GOLDEN]
    maps += [thin_maps.thin_map(R, C, ob)[0] for R, C, ob in thin_maps.all_maps()]
    maps += [cc.checkerboard(30, 51), cc.row_serpentine(30, 51), cc.col_serpentine(30, 51), cc.rings(30, 51), cc.seeded_random(30, 51, 0.41, 3),
             cc.shifted_copy(cc.rings(30, 51)), cc.split_wall(40, 37, 11, 17)]
    return maps


def test_move_masks_are_symmetric_on_every_test_map():
    for g in all_test_maps():
        for ad, rs in fc.POLICIES:
            assert cc.masks_symmetric(g, ad, rs), (g.shape, ad, rs)


@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_map_components(name):
    g = gio.grid(name)[0]
    counts, sizes11 = GOLDEN[name]
    got = [cc.flood_fill(g, ad, rs) for ad, rs in fc.POLICIES]
    assert tuple(len(r[1]) for r in got) == counts
    top = sorted(got[0][1].tolist(), reverse=True)
    assert top[:len(sizes11)] == sizes11
    if name == "g256":
        assert top.count(1) == 4 and sorted(got[1][1].tolist()).count(1) == 3
        assert int(got[0][1].sum()) == int((g != 1).sum())
    for lab, sizes, first in got:
        assert np.array_equal(cc.info_of(sizes), [len(sizes), (g != 1).sum(), sizes.max(), np.argmax(sizes)])


def test_checkerboard():
    """Free where r + c is even: one component under (1, 0); under the other three every free cell is its own component."""
    for R, C in ((6, 9), (31, 64), (64, 65)):
        g = cc.checkerboard(R, C)
        nfree = int((g != 1).sum())
        assert g[0, 0] == 0 and nfree == (R * C + 1) // 2
        for ad, rs in fc.POLICIES:
            lab, sizes, first = cc.flood_fill(g, ad, rs)
            if ad and not rs:
                assert len(sizes) == 1 and sizes[0] == nfree
            else:
                assert len(sizes) == nfree and np.all(sizes == 1)
                assert np.array_equal(first, np.flatnonzero(g.reshape(-1) != 1))


def test_serpentines_and_rings():
    for g in (cc.row_serpentine(30, 51), cc.col_serpentine(30, 51), cc.shifted_copy(cc.row_serpentine(30, 51))):
        for ad, rs in fc.POLICIES:
            assert len(cc.flood_fill(g, ad, rs)[1]) == 1
    g = cc.rings(30, 51)
    for ad, rs in fc.POLICIES:
        assert len(cc.flood_fill(g, ad, rs)[1]) == 5                  # walls at d = 2, 5, 8, 11, 14: the outer band and one band inside each but the last
    assert len(cc.flood_fill(cc.seeded_random(300, 517, 0.41, 1), 1, 1)[1]) > 300


@pytest.mark.parametrize("shape", [(40, 37, 11, 17), (64, 300, 255, 33)])
def test_split_wall_labels_are_the_flood_fills(shape):
    R, C, w, g = shape
    m = cc.split_wall(R, C, w, g)
    for ad, rs in fc.POLICIES:
        got, want = cc.flood_fill(m, ad, rs), cc.split_wall_labels(R, C, w, g, ad, rs)
        assert len(want[1]) == (1 if ad and not rs else 2)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (ad, rs)
