"""Visibility fields on the device (pf_visibility_field, pf_visibility_count, pf_visibility_paths, pathfit.Visibility) against the
models of tests/visibility_checkers.py (pinned by tests/test_visibility_checkers.py) and against pf_line_of_sight_batch.  Every
comparison is exact equality; every output buffer lies between canary words."""
import functools

import numpy as np
import pytest

import golden_io as gio
import smooth_model as sm
import visibility_checkers as vc

pytestmark = pytest.mark.gpu

CANARY = -77
BYTE = 0xB3                                                          # the canary of the byte masks
PAD = 64                                                             # canary words in front of and behind every output


def between_canaries(e, n, dtype):
    return e.put(np.full(n + 2 * PAD, BYTE if np.dtype(dtype) == np.uint8 else CANARY, dtype))


def inner(buf, tag):
    a = buf.download()
    can = BYTE if a.dtype == np.uint8 else CANARY
    assert np.all(a[:PAD] == can) and np.all(a[len(a) - PAD:] == can), tag
    return a[PAD:len(a) - PAD]


def ids_of(e, views):
    return np.array([r * e.C + c for r, c in views], np.int32)


def run_field(e, views, strict, rsq=-1, want_info=True):
    """One raw Engine call, every output between canaries -> (masks uint8 [K, R, C], info int64 [K, 4] or None)."""
    from pathfit.engine import _View
    K, RC = len(views), e.R * e.C
    sb, ib = between_canaries(e, K * RC, np.uint8), between_canaries(e, 4 * K, np.int64)
    try:
        e.visibility_field(ids_of(e, views), _View(e, sb.at(PAD), K * RC, np.uint8), strict, rsq, _View(e, ib.at(PAD), 4 * K, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        m, info = inner(sb, "seen").reshape(K, e.R, e.C), inner(ib, "info").reshape(K, 4)
        assert m.max() <= 1
        if not want_info:
            assert np.all(info == CANARY)
        return m, info if want_info else None
    finally:
        sb.free()
        ib.free()


def run_count(e, views, strict, rsq=-1, want_info=True):
    """-> (counts int32 [R, C], info int64 [4] or None)"""
    from pathfit.engine import _View
    RC = e.R * e.C
    cb, ib = between_canaries(e, RC, np.int32), between_canaries(e, 4, np.int64)
    try:
        e.visibility_count(ids_of(e, views), _View(e, cb.at(PAD), RC, np.int32), strict, rsq, _View(e, ib.at(PAD), 4, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        n, info = inner(cb, "count").reshape(e.R, e.C), inner(ib, "info")
        if not want_info:
            assert np.all(info == CANARY)
        return n, info if want_info else None
    finally:
        cb.free()
        ib.free()


def check_views(e, g, views, strict, rsq=-1, tag=None):
    """The masks and the info words of `views` against seen_map."""
    occ = vc.occ_of(g)
    m, info = run_field(e, views, strict, rsq)
    for k, a in enumerate(views):
        want = vc.seen_map(occ, a, strict, rsq)
        assert np.array_equal(m[k] != 0, want), (tag, g.shape, a, strict, rsq)
        assert list(info[k]) == vc.field_info(want, a), (tag, g.shape, a, strict, rsq, info[k])
    return m


def seeded(R, C, p, seed, keep=()):
    g = (np.random.default_rng(seed).random((R, C)) < p).astype(np.uint8)
    for a in keep:
        g[a] = 0
    return g


# ---- 1. pf_visibility_field against the model
@functools.lru_cache(maxsize=None)
def pairs_of(name, strict):
    return sm.all_pairs(vc.occ_of(gio.grid(name)[0]), strict)[0]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", sm.MAPS20)
def test_every_cell_of_the_golden_maps_as_a_viewpoint(name, strict):
    from pathfit.engine import Engine
    g = gio.grid(name)[0]
    want = pairs_of(name, strict)
    e = Engine(g)
    try:
        views = [(v // 20, v % 20) for v in range(400)]              # free and obstacle cells alike
        m, info = run_field(e, views, strict)
        assert np.array_equal(m.reshape(400, 400) != 0, want)
        for k in range(400):
            assert list(info[k]) == vc.field_info(want[k].reshape(20, 20), views[k]), k
        assert any(list(i) == [0, -1, -1, 0] for i in info) and np.array_equal(want, want.T)
    finally:
        e.close()
    assert (pairs_of(name, False) != pairs_of(name, True)).sum() > 0   # the two rules disagree on this map


@pytest.mark.parametrize("W, N", [(1, 4096), (2, 4096), (3, 4096), (1, 65), (3, 129), (2, 1000)])
@pytest.mark.parametrize("tall", [False, True])
def test_thin_maps(W, N, tall):
    from pathfit.engine import Engine
    g = np.zeros((W, N), np.uint8)
    rnd = np.random.default_rng(W * 7 + N)
    for c in rnd.choice(np.arange(N // 8, N), 5, replace=False):     # a few obstacles far out: sight lines of many 64-cell spans
        g[rnd.integers(0, W), c] = 1
    views = [(0, 0), (W - 1, N // 16), (W // 2, N - 1)]
    for a in views:
        g[a] = 0
    if tall:
        g, views = np.ascontiguousarray(g.T), [(c, r) for r, c in views]
    e = Engine(g)
    try:
        for strict in (False, True):
            m = check_views(e, g, views, strict)
            assert 0 < m[0].sum() <= g.size - 5                       # the end viewpoint's lines reach the obstacles, and stop there
    finally:
        e.close()


@pytest.mark.parametrize("C", [63, 64, 65, 128, 129, 255, 256, 257])
@pytest.mark.parametrize("R", [15, 16, 17])
def test_sizes_about_the_64_lane_and_256_thread_groups(R, C):
    """Column counts about the wavefront's 64 cells and the workgroup's 256, with copies shifted by one row and one column."""
    from pathfit.engine import Engine
    views = [(0, 0), (R // 2, C // 2), (R - 1, C - 1), (R - 1, 62)]
    g = seeded(R, C, 0.05, R * 1000 + C, views)
    sh = np.zeros_like(g)
    sh[1:, 1:] = g[:-1, :-1]
    shviews = [(min(r + 1, R - 1), min(c + 1, C - 1)) for r, c in views]
    for a in shviews:
        sh[a] = 0
    e = Engine(g)
    try:
        for strict in (False, True):
            check_views(e, g, views, strict, tag="base")
        e.update_grid(sh)
        for strict in (False, True):
            check_views(e, sh, shviews, strict, tag="shifted")
    finally:
        e.close()


def test_a_single_obstacle_on_every_cell_of_5x70():
    from pathfit.engine import Engine
    a = (2, 3)
    e = Engine(np.zeros((5, 70), np.uint8))
    differ = 0
    try:
        for v in range(5 * 70):
            g = np.zeros((5, 70), np.uint8)
            g.reshape(-1)[v] = 1
            e.update_grid(g)
            occ = vc.occ_of(g)
            got = [run_field(e, [a], s, want_info=False)[0][0] != 0 for s in (False, True)]
            want = [vc.seen_map(occ, a, s) for s in (False, True)]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), v
            differ += int(not np.array_equal(want[0], want[1]))
    finally:
        e.close()
    assert differ > 50                                                # a lone obstacle has corners that sight lines graze


def test_the_diagonal_gap_differs_between_the_rules():
    from pathfit.engine import Engine
    g, a, b = vc.diagonal_gap_map()
    e = Engine(g)
    try:
        loose, strict = check_views(e, g, [a, b], False), check_views(e, g, [a, b], True)
        assert loose[0][b] == 1 and strict[0][b] == 0 and loose[1][a] == 1 and strict[1][a] == 0
    finally:
        e.close()


def test_pure_lines_of_4095_cells():
    """A 4095 x 4095 map, free on the band |r - c| <= 1 and on row 0 and column 0 only (every other target is an obstacle and costs
    no walk): the pure diagonal, the pure row and the pure column from (0, 0), 64 passes of 64 cells each."""
    from pathfit.engine import Engine
    n = 4095
    g = np.ones((n, n), np.uint8)
    d = np.arange(n)
    g[d, d] = 0
    g[d[:-1], d[:-1] + 1] = 0
    g[d[:-1] + 1, d[:-1]] = 0
    g[0, :] = 0
    g[:, 0] = 0
    e = Engine(g)
    try:
        for step, obstacles in enumerate([(), ((2001, 2000),), ((3000, 3000), (0, 3500), (3900, 0)), ((4094, 4094),)]):
            for ob in obstacles:
                g[ob] = 1
            if step:
                e.update_grid(g)
            for strict in (False, True):
                m, info = run_field(e, [(0, 0)], strict)
                diag, row, col = vc.corner_lines(g, strict)
                assert np.array_equal(m[0][d, d] != 0, diag) and np.array_equal(m[0][0, :] != 0, row) and np.array_equal(m[0][:, 0] != 0, col), (step, strict)
                assert info[0][0] == int(m[0].sum())
                if step == 0:
                    assert diag.all() and list(info[0][1:]) == [2 * 4094 ** 2, n * n - 1, 0]
                if step == 1:
                    assert diag[2001:].any() != strict and diag[:2001].all()       # a touched cell: the strict rule alone stops there
    finally:
        e.close()


# ---- 2. sets and ranges
@pytest.fixture(scope="module")
def m4050():
    from pathfit.engine import Engine
    g = seeded(40, 50, 0.08, 77, [(20, 25), (0, 0), (39, 49)])
    e = Engine(g)
    yield e, g
    e.close()


def views_of(g, n, seed, free_only=True):
    ids = np.flatnonzero(g.reshape(-1) != 1) if free_only else np.arange(g.size)
    pick = np.random.default_rng(seed).choice(ids, n, replace=n > len(ids))
    return [(int(v) // g.shape[1], int(v) % g.shape[1]) for v in pick]


@pytest.mark.parametrize("K", [1, 3, 70])
def test_sets_of_1_3_and_70_viewpoints(m4050, K):
    e, g = m4050
    for strict in (False, True):
        check_views(e, g, views_of(g, K, K, free_only=False), strict)


def test_duplicates_and_a_viewpoint_on_an_obstacle(m4050):
    e, g = m4050
    wall = tuple(int(v) for v in np.argwhere(g == 1)[3])
    views = [(20, 25), wall, (20, 25), (0, 0), wall]
    m, info = run_field(e, views, True)
    check_views(e, g, views, True)
    assert np.array_equal(m[0], m[2]) and not m[1].any() and not m[4].any()
    assert list(info[1]) == [0, -1, -1, 0] and list(info[4]) == [0, -1, -1, 0] and list(info[0]) == list(info[2])
    assert not m[:, g == 1].any()                                     # an obstacle is never seen


def test_a_map_without_obstacles_and_a_sealed_room():
    from pathfit.engine import Engine
    g = np.zeros((33, 70), np.uint8)
    e = Engine(g)
    try:
        m = check_views(e, g, [(0, 0), (16, 35), (32, 69)], True)
        assert m.all()
        room = g.copy()
        room[10, 20:31] = room[20, 20:31] = 1
        room[10:21, 20] = room[10:21, 30] = 1
        e.update_grid(room)
        for strict in (False, True):
            m = check_views(e, room, [(15, 25), (0, 0), (11, 21)], strict)
            assert m[0].sum() == 81 and not m[1][11:20, 21:30].any() and m[2].sum() == 81
    finally:
        e.close()


@pytest.mark.parametrize("rsq", [0, 1, 2, 25, 40 * 40 + 50 * 50, -1])
def test_ranges(m4050, rsq):
    e, g = m4050
    views = [(20, 25), (0, 0), (39, 49), tuple(int(v) for v in np.argwhere(g == 1)[0])]
    for strict in (False, True):
        m = check_views(e, g, views, strict, rsq)
        if rsq == 0:
            assert m[0].sum() == 1 and m[0][20, 25] == 1 and m[3].sum() == 0
    if rsq > 100:
        assert np.array_equal(run_field(e, views, True, rsq)[0], run_field(e, views, True, -1)[0])
    n, info = run_count(e, views, True, rsq)
    want = vc.exposure(vc.occ_of(g), views, True, rsq)
    assert np.array_equal(n, want) and list(info) == vc.count_info(vc.occ_of(g), want)


# ---- 3. a 300 x 517 seeded map and an open one, K = 3
@pytest.mark.parametrize("open_map", [False, True])
def test_300x517_against_the_pair_kernel_and_the_model(open_map):
    from pathfit.engine import Engine
    g = vc.large_map(open_map)
    R, C = g.shape
    RC = R * C
    e = Engine(g)
    bufs = []
    try:
        dto, dvis = e.put(np.arange(RC, dtype=np.int32)), e.buf(RC, np.int32)
        bufs += [dto, dvis]
        for strict in (False, True):
            m, info = run_field(e, vc.LARGE_VIEWS, strict)
            for k, (a, targets, want) in enumerate(vc.large_sample(open_map, strict)):
                assert a == vc.LARGE_VIEWS[k]
                dfrom = e.put(np.full(RC, a[0] * C + a[1], np.int32))
                bufs.append(dfrom)
                e.line_of_sight_batch(dfrom, dto, RC, dvis, None, strict)           # another kernel: one wavefront per pair
                pair = dvis.download().reshape(R, C)
                assert np.array_equal(m[k], pair), (open_map, strict, a)
                got = np.array([m[k][t] != 0 for t in targets])
                assert np.array_equal(got, want), (open_map, strict, a)
                assert list(info[k]) == vc.field_info(pair != 0, a)
                if open_map:
                    assert m[k].all()
                else:
                    assert 0 < m[k].sum() < (g != 1).sum()
    finally:
        for b in bufs:
            b.free()
        e.close()


# ---- 4. pf_visibility_count
@pytest.mark.parametrize("K", [1, 70])
def test_count_equals_the_column_sums_of_the_masks(m4050, K):
    e, g = m4050
    occ = vc.occ_of(g)
    views = views_of(g, K, 5 + K, free_only=False)
    for strict in (False, True):
        m, _ = run_field(e, views, strict)
        n, info = run_count(e, views, strict)
        assert n.dtype == np.int32 and np.array_equal(n, m.sum(axis=0, dtype=np.int32))
        assert list(info) == vc.count_info(occ, n)
        assert run_count(e, views, strict, want_info=False)[1] is None
    if K == 70:                                                      # by symmetry: what v sees, read at the viewpoints
        n, _ = run_count(e, views, True)
        for v in vc.sample_targets(40, 50, 9, 200):
            assert n[v] == int(vc.seen(occ, v, True, -1, views).sum()), v


def test_count_of_1000_viewpoints_on_130x200():
    """No mask is materialised by the call under test; the reference masks come from pf_visibility_field in slices."""
    from pathfit.engine import Engine
    g = seeded(130, 200, 0.03, 130200)
    views = views_of(g, 1000, 1)
    e = Engine(g)
    try:
        for strict in (False, True):
            want = np.zeros((130, 200), np.int32)
            for i in range(0, 1000, 250):
                want += run_field(e, views[i:i + 250], strict, want_info=False)[0].sum(axis=0, dtype=np.int32)
            n, info = run_count(e, views, strict)
            assert np.array_equal(n, want) and list(info) == vc.count_info(vc.occ_of(g), want)
            assert want.max() > 100 and info[0] == ((want > 0) & (g != 1)).sum()
    finally:
        e.close()


def test_duplicates_count_twice(m4050):
    e, g = m4050
    a, b = (20, 25), (0, 0)
    one, _ = run_count(e, [a, b], True)
    two, info = run_count(e, [a, b, a, b], True)
    assert np.array_equal(two, 2 * one) and info[2] == 2 * one.max() and one.max() >= 1 and one[20, 25] >= 1


# ---- 5. other behaviour
def test_five_runs_are_identical(m4050):
    e, g = m4050
    views = views_of(g, 70, 3)
    first = (run_field(e, views, True), run_count(e, views, True))
    for _ in range(4):
        again = (run_field(e, views, True), run_count(e, views, True))
        for x, y in zip(first, again):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_a_door_opened_by_update_grid_is_seen_by_the_next_call():
    import pathfit
    g = np.zeros((9, 30), np.uint8)
    g[:, 15] = 1
    v = pathfit.Visibility(g)
    try:
        before = v.seen([(4, 2)])[0]
        assert not before[:, 16:].any() and v.exposure([(4, 2)])[4, 20] == 0 and v.coverage < 0.6
        g[4, 15] = 0
        v.engine.update_grid(g)
        after = v.seen([(4, 2)])[0]
        assert np.array_equal(after, vc.seen_map(vc.occ_of(g), (4, 2), True)) and after[4, 16:].all()
        assert v.exposure([(4, 2)])[4, 20] == 1 and v.kernel_ms > 0
        assert np.array_equal(v.cost_map([(4, 2)], 3.0), np.where(after, 4.0, 1.0))
    finally:
        v.close()


# ---- 6. pf_visibility_paths
def run_paths(e, dcount, cells, lens, cap, n=None, want_profile=True):
    from pathfit.engine import _View
    rows = len(lens)
    n = rows if n is None else n
    dc, dl = e.put(np.asarray(cells, np.int32).reshape(rows, cap)), e.put(np.asarray(lens, np.int32))
    ob, sb, pb = between_canaries(e, 4 * rows, np.int64), between_canaries(e, rows, np.int32), between_canaries(e, rows * cap, np.int32)
    try:
        e.visibility_paths(dcount, n, cap, dc, dl, _View(e, ob.at(PAD), 4 * rows, np.int64), _View(e, sb.at(PAD), rows, np.int32),
                           _View(e, pb.at(PAD), rows * cap, np.int32) if want_profile else None)
        return inner(ob, "out").reshape(rows, 4), inner(sb, "status"), inner(pb, "profile").reshape(rows, cap)
    finally:
        for b in (dc, dl, ob, sb, pb):
            b.free()


def check_paths(e, dcount, counts, rows, cap, want_profile=True):
    cells = np.full((len(rows), cap), 2 ** 31 - 1, np.int32)          # words beyond the length are never read
    for i, r in enumerate(rows):
        cells[i, :min(len(r), cap)] = r[:cap]
    out, st, prof = run_paths(e, dcount, cells, [len(r) for r in rows], cap, want_profile=want_profile)
    wout, wst, wprof = vc.path_exposure(counts, rows, cap)
    assert np.array_equal(out, wout) and np.array_equal(st, wst)
    for i, r in enumerate(rows):
        if want_profile and wprof[i] is not None:
            assert np.array_equal(prof[i, :len(r)], wprof[i]) and np.all(prof[i, len(r):] == CANARY), i
        else:
            assert np.all(prof[i] == CANARY), i
    return out, st


@pytest.fixture(scope="module")
def g256_counts():
    from pathfit.engine import Engine
    g = gio.grid("g256")[0]
    e = Engine(g)
    views = views_of(g, 40, 21)
    dcount = e.buf(g.size, np.int32)
    e.visibility_count(ids_of(e, views), dcount, True, -1, None)
    yield e, g, dcount, dcount.download().reshape(g.shape), views
    dcount.free()
    e.close()


def test_path_rows_against_the_model(g256_counts):
    e, g, dcount, counts = g256_counts[:4]
    flat = counts.reshape(-1)
    rnd = np.random.default_rng(31)
    some, top = np.flatnonzero((flat > 0) & (flat < flat.max())), np.flatnonzero(flat == flat.max())
    cap = 129                                                         # L = cap and L - 1 = cap - 1 lie between other rows
    rows = [rnd.choice(some, L).astype(np.int32) for L in (1, 63, 64, 65, 129, 128, 129, 2)]
    first, last, twice, edge = (rnd.choice(some, L).astype(np.int32) for L in (100, 100, 100, 129))
    first[0] = last[-1] = twice[17] = twice[80] = edge[64] = top[0]   # the peak first, last, twice (the first wins), on a lane's second trip
    rows += [first, last, twice, edge, np.flatnonzero(flat == 0)[:7].astype(np.int32)]
    rows += [np.zeros(0, np.int32), rnd.choice(some, cap + 1).astype(np.int32), np.array([5, -1, 7], np.int32), np.array([5, 6, g.size], np.int32),
             np.array([2 ** 31 - 1], np.int32), np.array([-2 ** 31, 4], np.int32)]
    out, st = check_paths(e, dcount, counts, rows, cap)
    assert list(st[-6:]) == [1] * 6 and np.all(st[:-6] == 0) and np.all(out[-6:] == [0, -1, -1, 0])
    assert out[8][2] == 0 and out[9][2] == 99 and out[10][2] == 17 and out[11][2] == 64 and list(out[12]) == [0, 0, 0, 0]
    check_paths(e, dcount, counts, rows, cap, want_profile=False)
    out, st, _ = run_paths(e, dcount, np.zeros((2, 4), np.int32), [1, 1], 4, n=0)
    assert np.all(out == CANARY) and np.all(st == CANARY)            # n == 0 launches nothing
    out, st, prof = run_paths(e, dcount, np.zeros((2, 4), np.int32), [1, 1], 4, n=1)
    assert st[0] == 0 and st[1] == CANARY and np.all(out[1] == CANARY) and prof[0, 0] == flat[0] and np.all(prof.reshape(-1)[1:] == CANARY)


def test_solver_rows_where_they_lie_in_hbm(g256_counts):
    """A* rows from pf_astar_batch's own buffers, and the same rows through the class."""
    import pathfit
    e, g, dcount, counts, views = g256_counts
    rnd = np.random.default_rng(12)
    free = np.flatnonzero(g.reshape(-1) != 1)
    n, cap = 48, e.default_path_cap()
    ds, dt = e.put(rnd.choice(free, n).astype(np.int32)), e.put(rnd.choice(free, n).astype(np.int32))
    dc, dl, dst = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
    do, dstat = e.buf((n, 4), np.int64), e.buf(n, np.int32)
    v = pathfit.Visibility(g, engine=e)
    try:
        e.astar_batch(0, ds, dt, n, cap, dc, dl, dst)
        cells, lens = dc.download().reshape(n, cap), dl.download()
        assert (dst.download() == 0).sum() >= 24
        e.visibility_paths(dcount, n, cap, dc, dl, do, dstat)
        rows = [cells[i, :max(lens[i], 0)] for i in range(n)]
        wout, wst, _ = vc.path_exposure(counts, rows, cap)
        assert np.array_equal(do.download(), wout) and np.array_equal(dstat.download(), wst) and (wst == 1).sum() == (lens < 1).sum()
        assert np.array_equal(v.exposure(views), counts) and v.counts_device is v.exposure_device(views)
        for got in (v.path_exposure(rows), v.path_exposure(rows, counts), v.path_exposure(rows, dcount),
                    v.path_exposure([pathfit.CellPath(r, 256) for r in rows])):
            assert np.array_equal(np.stack(got, axis=1), wout) and np.array_equal(v.status, wst)
        patrol = pathfit.CellPath(rows[int(np.argmax(lens))][:40], 256)   # a patrol route as the viewpoint list
        got = v.exposure(patrol, max_range=4.5)                        # floor(4.5^2) = 20
        masks = v.seen([(int(c) // 256, int(c) % 256) for c in patrol.cells], max_range=4.5)
        assert np.array_equal(got, masks.sum(axis=0, dtype=np.int32)) and got.max() >= 2 and 0 < v.coverage < 1
        rr, cc = np.mgrid[0:256, 0:256]
        a = (int(patrol.cells[0]) // 256, int(patrol.cells[0]) % 256)
        assert not masks[0][(rr - a[0]) ** 2 + (cc - a[1]) ** 2 > 20].any() and v.info[0, 1] <= 20
    finally:
        v.close()
        for b in (ds, dt, dc, dl, dst, do, dstat):
            b.free()


# ---- 7. end to end on g256: a route that stays out of sight where it can
def test_stealth_route_on_g256():
    import cost_checkers as ck
    import field_checkers as fc
    import pathfit
    g, s, t = gio.grid("g256")
    R, C = g.shape
    e = pathfit.Engine(g)
    v = pathfit.Visibility(g, engine=e)
    cf = None
    try:
        short, length = pathfit.DijkstraSolver(g, engine=e).solve()[:2]
        short = [tuple(int(x) for x in p) for p in short]
        assert short[0] == (s // C, s % C) and short[-1] == (t // C, t % C)
        watchers = [short[len(short) // 3], short[len(short) // 2], short[2 * len(short) // 3]]   # they stand on the shortest route
        cost = v.cost_map(watchers, 4.0)
        assert cost.dtype == np.float64 and cost.min() == 1.0 and cost.max() == 1.0 + 4.0 * v.info[2] and 0 < v.coverage < 1
        cf = pathfit.CostField(g, cost, [short[0]], engine=e)
        want, _ = ck.dijkstra(g, fc.move_masks(g, 1, 1), cost, [s])
        assert np.array_equal(cf.fields[0].view(np.uint64), want.view(np.uint64))                  # bit for bit
        route = cf.paths([short[-1]])[0]
        tot, bad = cf.path_costs([route, pathfit.CellPath(np.array([r * C + c for r, c in short], np.int32), C)])
        assert np.all(bad == -1) and tot[0] == want.reshape(-1)[t] and tot[0] <= tot[1]
        # on the CPU: the watchers make the two routes differ, and the stealth route is the less exposed one
        assert [(int(c) // C, int(c) % C) for c in route.cells] != short and ck.path_cost(cost, route.cells.tolist(), C) < ck.path_cost(cost, [r * C + c for r, c in short], C)
        totals = v.path_exposure([route, short])[0]
        assert totals[0] < totals[1]
    finally:
        if cf is not None:
            cf.close()
        v.close()
        e.close()


# ---- 8. argument errors of the raw ABI
def test_argument_errors_leave_every_output_untouched(m4050):
    from pathfit._lib import PathfitError
    from pathfit.engine import _View
    e, g = m4050
    RC = g.size
    L = e.L
    sb, cb, ib = between_canaries(e, RC, np.uint8), between_canaries(e, RC, np.int32), between_canaries(e, 4, np.int64)
    ob, stb, pb = between_canaries(e, 4, np.int64), between_canaries(e, 1, np.int32), between_canaries(e, 4, np.int32)
    dcells, dlen = e.put(np.zeros(4, np.int32)), e.put(np.ones(1, np.int32))
    ok = np.array([5], np.int32)
    seen, cnt, info = sb.at(PAD), cb.at(PAD), ib.at(PAD)
    try:
        for fn, out in ((L.pf_visibility_field, seen), (L.pf_visibility_count, cnt)):
            assert fn(None, 1, -1, 1, ok.ctypes.data, out, info) == -2
            for args, msg in [((1, -1, 0, ok.ctypes.data, out, info), "K = 0"), ((1, -1, -3, ok.ctypes.data, out, info), "K = -3"),
                              ((1, -2, 1, ok.ctypes.data, out, info), "max_range_sq = -2"), ((1, -1, 1, None, out, info), "must not be null"),
                              ((1, -1, 1, ok.ctypes.data, None, info), "must not be null"),
                              ((1, -1, 3, np.array([5, RC, 7], np.int32).ctypes.data, out, info), "viewpoint 1 = 2000 lies outside the grid"),
                              ((1, -1, 2, np.array([5, -1], np.int32).ctypes.data, out, info), "viewpoint 1 = -1 lies outside the grid")]:
                assert fn(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode(), (fn, msg, L.pf_last_error(e.h))
        paths = L.pf_visibility_paths
        assert paths(None, cnt, 1, 4, dcells.ptr, dlen.ptr, ob.at(PAD), pb.at(PAD), stb.at(PAD)) == -2
        for args in [(cnt, -1, 4, dcells.ptr, dlen.ptr, ob.at(PAD), pb.at(PAD), stb.at(PAD)), (cnt, 1, 0, dcells.ptr, dlen.ptr, ob.at(PAD), pb.at(PAD), stb.at(PAD)),
                     (None, 1, 4, dcells.ptr, dlen.ptr, ob.at(PAD), pb.at(PAD), stb.at(PAD)), (cnt, 1, 4, None, dlen.ptr, ob.at(PAD), pb.at(PAD), stb.at(PAD)),
                     (cnt, 1, 4, dcells.ptr, None, ob.at(PAD), pb.at(PAD), stb.at(PAD)), (cnt, 1, 4, dcells.ptr, dlen.ptr, None, pb.at(PAD), stb.at(PAD)),
                     (cnt, 1, 4, dcells.ptr, dlen.ptr, ob.at(PAD), pb.at(PAD), None)]:
            assert paths(e.h, *args) == -1 and "pf_visibility_paths: bad arguments" in L.pf_last_error(e.h).decode(), args
        assert paths(e.h, cnt, 0, 4, dcells.ptr, dlen.ptr, ob.at(PAD), pb.at(PAD), stb.at(PAD)) == 0
        with pytest.raises(PathfitError, match="pf_visibility_field: bad arguments"):
            e.visibility_field([], _View(e, seen, RC, np.uint8))
        for b in (sb, cb, ib, ob, stb, pb):
            a = b.download()
            assert np.all(a == (BYTE if a.dtype == np.uint8 else CANARY))
    finally:
        for b in (sb, cb, ib, ob, stb, pb, dcells, dlen):
            b.free()
