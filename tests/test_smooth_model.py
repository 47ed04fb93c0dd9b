"""The model of any-angle smoothing (tests/smooth_model.py) pinned on any host: the integer rule against exact rational clipping, the
corner rule of the move policies on single steps, and the properties and case tables the GPU assertions of tests/test_gpu_smooth.py
rest on."""
from fractions import Fraction as F

import numpy as np
import pytest

import golden_io as gio
import smooth_model as sm

HALF = F(1, 2)


def clip(a, b, cell, closed):
    """The parameter interval [lo, hi] of the segment a -> b (centres) inside the cell's square, open or closed, by exact rational
    Liang-Barsky clipping; None when they do not meet."""
    lo, hi = F(0), F(1)
    for p0, p1, m in ((a[0], b[0], cell[0]), (a[1], b[1], cell[1])):
        d, e0, e1 = p1 - p0, m - HALF, m + HALF
        if d == 0:
            if not ((e0 <= p0 <= e1) if closed else (e0 < p0 < e1)):
                return None
            continue
        t0, t1 = sorted(((e0 - p0) / d, (e1 - p0) / d))
        lo, hi = max(lo, t0), min(hi, t1)
    if closed:
        return (lo, hi) if lo <= hi else None
    # the open square: some t of [0, 1] strictly between the bounds of every axis.  lo / hi were clamped to [0, 1]: a proper
    # interval is enough, a single point is never inside an open set's preimage unless the interval is proper
    return (lo, hi) if lo < hi else None


def test_rule_equals_exact_clipping_on_6x6():
    cells = [(r, c) for r in range(6) for c in range(6)]
    pairs = 0
    for a in cells:
        for b in cells:
            if a == b:
                assert sm.segment_cells(a, b) == ([a], [])
                continue
            crossed = [p for p in cells if clip(a, b, p, False)]
            meets = [p for p in cells if clip(a, b, p, True)]
            touched = [p for p in meets if p not in crossed]
            for p in touched:                                       # a touch is one point, and that point is a corner of the square
                lo, hi = clip(a, b, p, True)
                assert lo == hi
                pt = (a[0] + lo * (b[0] - a[0]), a[1] + lo * (b[1] - a[1]))
                assert abs(pt[0] - p[0]) == HALF and abs(pt[1] - p[1]) == HALF
            assert sm.segment_cells(a, b) == (crossed, touched), (a, b)
            assert a in crossed and b in crossed
            pairs += 1
    assert pairs == 36 * 35


def test_single_steps_are_the_corner_rule_on_fig7():
    g, _, _ = gio.grid("fig7")
    occ = sm.occ_of(g)
    R, C = occ.shape
    free = lambda r, c: occ[r, c] != 1                              # noqa: E731
    steps = diag_cut = 0
    for r in range(R):
        for c in range(C):
            for dr, dc in ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
                nr, nc = r + dr, c + dc
                if not (0 <= nr < R and 0 <= nc < C):
                    continue
                loose = free(r, c) and free(nr, nc)
                strict = loose and (dr == 0 or dc == 0 or (free(nr, c) and free(r, nc)))     # helper.py:46-49
                assert sm.visible(occ, (r, c), (nr, nc), 1) == strict
                assert sm.visible(occ, (r, c), (nr, nc), 0) == loose
                steps += 1
                diag_cut += loose and not strict
    assert steps == 8 * R * C - 6 * (R + C) + 4 and diag_cut > 50


@pytest.mark.parametrize("name", sm.MAPS20)
def test_visibility_is_symmetric_and_the_table_is_the_scalar_rule(name):
    g, _, _ = gio.grid(name)
    occ = sm.occ_of(g)
    C = occ.shape[1]
    rnd = np.random.default_rng(3)
    tab = {s: sm.all_pairs(occ, s) for s in ((0, 1) if name == "fig7" else ())}
    for a, b in rnd.integers(0, occ.size, (1500, 2)):
        pa, pb = (int(a) // C, int(a) % C), (int(b) // C, int(b) % C)
        for s in (0, 1):
            v = sm.visible(occ, pa, pb, s)
            assert v == sm.visible(occ, pb, pa, s)
            assert (sm.first_block(occ, pa, pb, s) < 0) == v
            if s in tab:
                assert tab[s][0][a, b] == v and tab[s][1][a, b] == sm.first_block(occ, pa, pb, s)
    if tab:
        assert np.array_equal(tab[0][0], tab[0][0].T) and np.array_equal(tab[1][0], tab[1][0].T)
        assert (tab[0][0] & ~tab[1][0]).sum() > 1000 and not (tab[1][0] & ~tab[0][0]).any()     # strict sees less, never more


def test_first_block_rule():
    """Hand-made cases: the nearest major index wins over a smaller cell id, and within one index the smaller id."""
    occ = np.zeros((7, 9), np.uint8)
    occ[2, 6] = occ[3, 3] = 1
    assert sm.first_block(occ, (3, 0), (2, 8), 0) == 3 * 9 + 3       # column 3 is nearer (3, 0) than column 6
    assert sm.first_block(occ, (2, 8), (3, 0), 0) == 2 * 9 + 6       # and from the other end column 6
    occ[:] = 0
    occ[0, 1] = occ[1, 0] = 1
    assert sm.first_block(occ, (0, 0), (1, 1), 1) == 9 and sm.first_block(occ, (0, 0), (1, 1), 0) == -1   # column 0 holds (1, 0)
    assert sm.first_block(occ, (1, 1), (0, 0), 1) == 1               # and from the other end column 1 holds (0, 1)
    occ[:] = 0
    occ[4, 4] = 1
    assert sm.first_block(occ, (4, 4), (4, 4), 0) == 4 * 9 + 4 and sm.first_block(occ, (0, 0), (0, 0), 1) == -1


def path_facts(occ, p, C):
    """Smooth one path in both modes and check what holds for every input -> (strict positions, loose positions, log of strict)."""
    pp = [(int(x) // C, int(x) % C) for x in p]
    res = []
    for s in (1, 0):
        log = []
        out = sm.smooth(occ, p, s, log)
        assert len(log) == max(len(p) - 2, 0)                        # L - 2 tests
        assert out[0] == 0 and out[-1] == len(p) - 1 and all(x < y for x, y in zip(out, out[1:]))   # a subsequence with both ends
        for x, y in zip(out, out[1:]):                              # every segment is an input step or visible
            assert y == x + 1 or sm.visible(occ, pp[x], pp[y], s), (x, y, s)
        assert sm.stats(p[out], C)[0] <= sm.input_length(p, C) * (1 + 1e-12)
        res.append((out, log))
    return res[0][0], res[1][0], res[0][1]


@pytest.mark.parametrize("name", sm.MAPS20 + ("g128crop",))
def test_case_table_of_a_map(name):
    g, paths = sm.astar_cases(name)
    occ = sm.occ_of(g)
    C = occ.shape[1]
    assert len(paths) == sm.PATHS_PER_MAP
    three = later = differ = 0
    for p in paths:
        strict, loose, log = path_facts(occ, p, C)
        pp = [(int(x) // C, int(x) % C) for x in p]
        three += len(strict) >= 3
        differ += strict != loose
        later += any(not v and any(sm.visible(occ, pp[a], pp[m], 1) for m in range(j + 1, len(pp))) for a, j, v in log)
    assert three >= 40 and later >= 10 and differ >= 30, (three, later, differ)


def test_case_table_of_the_thin_maps():
    cases = sm.thin_cases()
    assert len(cases) >= 25 and sum(len(p) >= 3 for _, _, p in cases) >= 15
    bends = long_runs = 0
    for name, g, p in cases:
        if len(p) == 0:
            continue
        strict, _, _ = path_facts(sm.occ_of(g), p, g.shape[1])
        bends += len(strict) >= 3
        long_runs += len(strict) == 2 and len(p) > 130               # one segment of more than two 64-lane passes, in a box < 3 wide
    assert bends >= 1 and long_runs >= 6, (bends, long_runs)


def test_rows_the_device_rejects():
    occ = np.zeros((4, 5), np.uint8)
    assert sm.smooth_row(occ, [], 1)[0] == 1 and sm.smooth_row(occ, [0, 20, 1], 1)[0] == 1 and sm.smooth_row(occ, [0, -1], 1)[0] == 1
    occ[1, 2] = 1
    st, way, idx, length, turns = sm.smooth_row(occ, [0, 1, 2, 3, 8, 13, 12, 11], 1)
    assert st == 0 and list(idx) == sm.smooth(occ, [0, 1, 2, 3, 8, 13, 12, 11], 1) and list(way) == [[0, 1, 2, 3, 8, 13, 12, 11][i] for i in idx]
    assert sm.smooth_row(occ, [0, 1, 2, 3, 8, 13, 12, 11], 1, way_cap=len(idx) - 1)[0] == 3
    assert sm.smooth_row(occ, [0, 1, 2, 3, 8, 13, 12, 11], 1, way_cap=len(idx))[0] == 0
    st, way, idx, _, _ = sm.smooth_row(occ, [7], 1)
    assert st == 0 and list(way) == [7] and list(idx) == [0]
    assert sm.stats([0, 3, 13, 11], 5) == (float(np.float64(3.0) + np.sqrt(np.float64(4.0)) + np.float64(2.0)), 2)
    assert sm.stats([0, 2, 4], 5)[1] == 0 and sm.stats([0, 2, 0], 5)[1] == 1 and sm.stats([0, 0, 2], 5)[1] == 0
