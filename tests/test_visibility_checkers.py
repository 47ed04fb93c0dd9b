"""The CPU model of the visibility fields (tests/visibility_checkers.py) against the pinned rule of tests/smooth_model.py, and the CPU
facts tests/test_gpu_visibility.py leans on.  Runs on any host."""

import numpy as np
import pytest

import golden_io as gio
import smooth_model as sm
import visibility_checkers as vc


def every_3x4():
    for bits in range(1 << 12):
        yield np.array([(bits >> i) & 1 for i in range(12)], np.uint8).reshape(3, 4)


@pytest.mark.parametrize("strict", [False, True])
def test_seen_equals_the_rows_of_all_pairs_on_every_3x4_grid(strict):
    for n, occ in enumerate(every_3x4()):
        vis, _ = sm.all_pairs(occ, strict)
        # all_pairs says "no blocker between a and b"; a target on an obstacle blocks itself, a viewpoint on one blocks every line
        for a in range(12):
            want = vis[a].reshape(3, 4)
            got = vc.seen_map(occ, (a // 4, a % 4), strict)
            assert np.array_equal(got, want), (n, a, strict)
            if n % 64 == 5:
                assert np.array_equal(vc.seen(occ, (a // 4, a % 4), strict), want), (n, a, strict)


@pytest.mark.parametrize("strict", [False, True])
def test_symmetry_on_every_3x4_grid_and_a_golden_map(strict):
    for occ in every_3x4():
        vis, _ = sm.all_pairs(occ, strict)
        assert np.array_equal(vis, vis.T)
    occ = vc.occ_of(gio.grid("img2")[0])
    m = np.stack([vc.seen_map(occ, (a // 20, a % 20), strict).reshape(-1) for a in range(400)])
    assert np.array_equal(m, m.T)
    assert not m[occ.reshape(-1) == 1].any() and not m[:, occ.reshape(-1) == 1].any()


@pytest.mark.parametrize("strict", [False, True])
def test_seen_map_equals_the_definition_on_seeded_maps(strict):
    rnd = np.random.default_rng(3)
    for R, C, p in ((9, 14, 0.15), (5, 33, 0.08), (17, 6, 0.25), (1, 40, 0.05), (12, 12, 0.0)):
        occ = (rnd.random((R, C)) < p).astype(np.uint8)
        for a in [(0, 0), (R // 2, C // 2), (R - 1, C - 1), (R - 1, 0)]:
            for rsq in (-1, 25):
                assert np.array_equal(vc.seen_map(occ, a, strict, rsq), vc.seen(occ, a, strict, rsq)), (R, C, a, rsq)


@pytest.mark.parametrize("rsq, cells", [(0, 1), (1, 5), (2, 9), (25, 81), (-1, 21 * 23)])
def test_the_range_disc(rsq, cells):
    occ = np.zeros((21, 23), np.uint8)
    got = vc.seen_map(occ, (10, 11), True, rsq)
    assert int(got.sum()) == cells
    rr, cc = np.mgrid[0:21, 0:23]
    d2 = (rr - 10) ** 2 + (cc - 11) ** 2
    assert np.array_equal(got, (d2 <= rsq) if rsq >= 0 else np.ones_like(got))
    assert np.array_equal(got, vc.seen(occ, (10, 11), True, rsq))
    assert vc.field_info(got, (10, 11))[:2] == [cells, int(d2[got].max())]


# ---- walkers the model must reject
def bresenham_sees(occ, a, b):
    """A thin-line walker: one cell per major index."""
    (r0, c0), (r1, c1) = a, b
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr, sc = (1 if r1 > r0 else -1), (1 if c1 > c0 else -1)
    err, r, c = dc - dr, r0, c0
    while True:
        if occ[r, c] == 1:
            return False
        if (r, c) == (r1, c1):
            return True
        e2 = 2 * err
        if e2 > -dr:
            err -= dr
            c += sc
        if e2 < dc:
            err += dc
            r += sr


def test_the_model_rejects_a_thin_line_walker():
    # (0, 0) -> (2, 5): the segment crosses two cells in some columns; a thin line visits one cell per column
    crossed, _ = sm.segment_cells((0, 0), (2, 5))
    assert len(crossed) > 6
    differ = 0
    for ob in crossed[1:-1]:
        occ = np.zeros((3, 6), np.uint8)
        occ[ob] = 1
        assert not vc.seen(occ, (0, 0), False)[2, 5], ob
        differ += bresenham_sees(occ, (0, 0), (2, 5))
    assert differ >= 1
    rnd = np.random.default_rng(11)
    occ = (rnd.random((12, 15)) < 0.12).astype(np.uint8)
    occ[6, 7] = 0
    thin = np.array([[occ[r, c] != 1 and bresenham_sees(occ, (6, 7), (r, c)) for c in range(15)] for r in range(12)])
    assert not np.array_equal(thin, vc.seen(occ, (6, 7), False))


def test_the_model_rejects_a_walker_that_ignores_touched_cells():
    g, a, b = vc.diagonal_gap_map()
    occ = vc.occ_of(g)
    loose, strict = vc.seen(occ, a, False), vc.seen(occ, a, True)
    assert loose[b] and not strict[b]                                  # the gap: open under the loose rule only
    assert np.array_equal(vc.seen_map(occ, a, False), loose) and np.array_equal(vc.seen_map(occ, a, True), strict)
    # a "strict" walker that forgets the touched cells is the loose rule: it differs here and on every golden map
    for name in sm.MAPS20:
        o = vc.occ_of(gio.grid(name)[0])
        v0, _ = sm.all_pairs(o, False)
        v1, _ = sm.all_pairs(o, True)
        assert (v0 != v1).sum() > 0 and not (v1 & ~v0).any(), name


def test_the_large_sample_holds_seen_and_hidden_targets_at_spans_above_64():
    for strict in (False, True):
        far_seen = far_hidden = 0
        for a, targets, want in vc.large_sample(False, strict):
            span = np.array([max(abs(t[0] - a[0]), abs(t[1] - a[1])) for t in targets])
            far_seen += int((want & (span > 64)).sum())
            far_hidden += int((~want & (span > 64)).sum())
        assert far_seen >= 20 and far_hidden >= 20, (strict, far_seen, far_hidden)
    for a, targets, want in vc.large_sample(True, True):
        assert want.all()


@pytest.mark.parametrize("strict", [False, True])
def test_corner_lines_equal_the_definition(strict):
    rnd = np.random.default_rng(8)
    hits = 0
    for trial in range(30):
        occ = (rnd.random((11, 13)) < 0.06).astype(np.uint8)
        occ[0, 0] = trial == 7
        want = vc.seen(occ, (0, 0), strict)
        diag, row, col = vc.corner_lines(occ, strict)
        d = np.arange(11)
        assert np.array_equal(diag, want[d, d]) and np.array_equal(row, want[0, :]) and np.array_equal(col, want[:, 0]), trial
        hits += int((~diag).any()) + int((~row).any())
    assert hits > 10


def test_exposure_counts_duplicates_twice_and_path_exposure():
    occ = vc.occ_of(gio.grid("fig7")[0])
    free = [tuple(int(x) for x in v) for v in np.argwhere(occ != 1)[:3]]
    one, two = vc.exposure(occ, free[:1], True), vc.exposure(occ, [free[0], free[0]], True)
    assert np.array_equal(two, 2 * one) and one.max() == 1
    counts = vc.exposure(occ, free, True)
    assert vc.count_info(occ, counts)[1] == int((occ != 1).sum())
    out, st, prof = vc.path_exposure(counts, [[0, 1, 2], [], [400], [5]], 3)
    assert list(st) == [0, 1, 1, 0] and list(out[1]) == [0, -1, -1, 0] and prof[1] is None
    assert out[0, 0] == counts.reshape(-1)[:3].sum() and out[3, 2] == 0
