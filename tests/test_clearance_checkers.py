"""The models of tests/clearance_checkers.py, pinned: the brute force against an independently written separable transform, the margin
rule against hand-computed values, the path and segment models on a map small enough to read, and the field against the reference's
own safety term (tests/golden/decode_cases.npz).  No device."""
import math

import numpy as np
import pytest

import clearance_checkers as ck
import golden_io as gio


def separable(grid, border):
    """Row pass (the left obstacle wins an equal |dc|), then column pass (the lowest row wins an equal sum), in plain loops."""
    g = np.asarray(grid)
    R, C = g.shape
    col_of = [[None] * C for _ in range(R)]
    for r in range(R):
        here = [c for c in range(C) if g[r, c] == 1]
        for c in range(C):
            pick = None
            for o in here:                                            # (increasing columns: `<` keeps the left one)
                if pick is None or abs(o - c) < abs(pick - c):
                    pick = o
            col_of[r][c] = pick
    d2 = np.full((R, C), ck.NONE, np.int64)
    near = np.full((R, C), -1, np.int64)
    for c in range(C):
        for r in range(R):
            for q in range(R):                                        # (increasing rows: `<` keeps the lowest one)
                o = col_of[q][c]
                if o is not None and (q - r) ** 2 + (o - c) ** 2 < d2[r, c]:
                    d2[r, c] = (q - r) ** 2 + (o - c) ** 2
                    near[r, c] = q * C + o
            if border:
                d2[r, c] = min(d2[r, c], min(r + 1, R - r, c + 1, C - c) ** 2)
    return d2, near


def check(g):
    for border in (False, True):
        d2, near, info = ck.brute_force(g, border)
        want = separable(g, border)
        assert np.array_equal(d2, want[0]) and np.array_equal(near, want[1]), (g, border)
        assert np.array_equal(info, ck.info_of(g, want[0]))


def test_every_3x4_grid():
    for bits in range(4096):
        check(np.array([(bits >> i) & 1 for i in range(12)], np.uint8).reshape(3, 4))


def test_seeded_maps_up_to_12x13():
    rnd = np.random.default_rng(1213)
    for i in range(120):
        R, C = int(rnd.integers(1, 13)), int(rnd.integers(1, 14))
        g = (rnd.random((R, C)) < (0.03, 0.15, 0.4, 0.8)[i % 4]).astype(np.uint8)
        g[rnd.integers(0, R), rnd.integers(0, C)] = (0, 2, 3)[i % 3]     # markers are free cells
        check(g)
    check(np.zeros((12, 13), np.uint8))
    check(np.ones((12, 13), np.uint8))
    for g in ck.tie_maps():
        check(g)


def test_window_form_equals_list_form():
    rnd = np.random.default_rng(8)
    for i in range(40):
        g = ck.seeded(int(rnd.integers(1, 30)), int(rnd.integers(1, 30)), (0.01, 0.05, 0.3)[i % 3], 100 + i)
        for border in (False, True):
            a, b = ck.brute_force(g, border), ck.brute_force(g, border, window=(1, 2, 5)[i % 3])
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), i
    g = ck.seeded(60, 70, 0.3, 9)
    assert g.sum() * g.size <= ck.LIST_BUDGET                        # (the list form)
    a, b = ck.brute_force(g), ck.brute_force(g, window=8)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_info_and_special_maps():
    d2, near, info = ck.brute_force(np.zeros((3, 4), np.uint8))
    assert np.all(d2 == ck.NONE) and np.all(near == -1) and list(info) == [0, 12, ck.NONE, 0]
    d2, near, info = ck.brute_force(np.zeros((3, 4), np.uint8), True)
    assert d2.tolist() == [[1, 1, 1, 1], [1, 4, 4, 1], [1, 1, 1, 1]] and np.all(near == -1) and list(info) == [0, 12, 4, 5]
    d2, near, info = ck.brute_force(np.ones((3, 4), np.uint8), True)
    assert np.all(d2 == 0) and np.array_equal(near.reshape(-1), np.arange(12)) and list(info) == [12, 0, -1, -1]
    g = np.zeros((3, 5), np.uint8)
    g[1, 1] = g[1, 3] = 1
    d2, near, info = ck.brute_force(g)
    assert d2.tolist() == [[2, 1, 2, 1, 2], [1, 0, 1, 0, 1], [2, 1, 2, 1, 2]]
    assert near[:, 2].tolist() == [6, 6, 6] and near[0].tolist() == [6, 6, 6, 8, 8]      # the left one of two equally near
    assert list(info) == [2, 13, 2, 0]


def test_margin_sq():
    want = {1.5: 3, 1.8: 4, math.sqrt(2.0): 2, 2.0: 4, math.nextafter(2.0, 3.0): 5, 15.9: 253}
    from pathfit.clearance import margin_to_sq
    for m, n in want.items():
        assert ck.margin_sq(m) == n and margin_to_sq(m) == n, m
        assert math.sqrt(n) >= m and math.sqrt(n - 1) < m
    for m in np.random.default_rng(3).uniform(0.01, 300.0, 2000):
        assert margin_to_sq(float(m)) == ck.margin_sq(float(m)), m
    for k in range(1, 400):                                           # whole numbers and exact roots
        assert margin_to_sq(float(k)) == k * k and margin_to_sq(math.sqrt(k)) == ck.margin_sq(math.sqrt(k))


def test_path_and_segment_models():
    g = np.zeros((5, 6), np.uint8)
    g[2, 2] = 1
    d2 = ck.brute_force(g)[0]
    cells = [0, 7, 14, 15, 10, 5]                                     # (0,0) (1,1) (2,2) (2,3) (1,4) (0,5)
    st, out, prof = ck.path_row(d2, cells, 8, 2)
    assert st == 0 and prof.tolist() == [8, 2, 0, 1, 5, 13] and out.tolist() == [0, 2, 2, 2]
    assert ck.path_row(d2, cells, 8, 0)[1].tolist() == [0, 2, 0, -1]
    assert ck.path_row(d2, [7, 13, 7], 8, 3)[1].tolist() == [1, 1, 3, 0]
    assert ck.path_row(d2, [7, 8, 7], 8, 3)[1].tolist() == [1, 1, 3, 0] and ck.path_row(d2, [7, 13, 8], 8, 1)[1].tolist() == [1, 1, 0, -1]
    for bad in ([], [0] * 9, [0, -1], [0, 30]):
        st, out, prof = ck.path_row(d2, bad, 8, 5)
        assert st == 1 and out.tolist() == [ck.NONE, -1, 0, -1] and prof is None
    assert ck.segment(d2, (0, 0), (4, 4), False) == (0, 14)          # through the obstacle
    assert ck.segment(d2, (1, 2), (2, 3), False) == (1, 8) and ck.segment(d2, (1, 2), (2, 3), True) == (0, 14)   # the corner touch
    assert ck.segment(d2, (3, 3), (3, 3), True) == (2, 21) and ck.segment(d2, (0, 0), (0, 6), False) == (ck.NONE, -1)
    assert ck.segment(d2, (-1, 0), (0, 0), False) == (ck.NONE, -1)
    assert ck.segment(d2, (0, 0), (0, 5), False) == (4, 2)           # the smallest id of the minimum


def test_field_reproduces_the_reference_safety_term():
    """helper.py:67-80 does not treat the grid edge as an obstacle: border=False.  The safety term of every golden row, recomputed
    from the brute-force field, equals the captured stats[:, 2] bit for bit, and the cells below margin_sq(min_safe) are exactly the
    cells that paid."""
    z = gio.load("decode_cases")
    names = [str(s) for s in z["grid_names"]]
    fields = {n: ck.brute_force(gio.grid(n)[0], False)[0] for n in names}
    nonzero = 0
    for i in range(len(z["kind"])):
        w = z["main_w"] if str(z["weights"][i]) == "main" else z["def_w"]
        min_safe = float(w[2])
        d2 = fields[names[int(z["grid_id"][i])]]
        cells = gio.csr_get(z["path_off"], z["path"], i)
        term, paid = ck.safety_term(d2, cells, min_safe)
        want = float(z["stats"][i, 2])
        assert term == want or (len(cells) == 0 and want == 0.0), (i, term, want)
        if len(cells):
            assert ck.path_row(d2, cells, len(cells), ck.margin_sq(min_safe))[1][2] == paid, i
        nonzero += want != 0.0
    assert nonzero >= 1
