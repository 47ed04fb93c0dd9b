"""Any-angle smoothing on the device (pf_line_of_sight_batch, pf_smooth_batch, pathfit.PathSmoother) against the model of
tests/smooth_model.py, which tests/test_smooth_model.py pins on any host.  Every comparison is exact: flags, cells, positions,
statuses, and the fp64 stats as bit patterns."""
import numpy as np
import pytest

import golden_io as gio
import smooth_model as sm
from pathfit import PathSmoother
from pathfit.engine import Engine

pytestmark = pytest.mark.gpu

CANARY = -77
CANARY_F = -77.5


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def los(e, frm, to, strict, want_fb=True):
    """One raw launch -> (visible int32[n], first_block int32[n])."""
    n = len(frm)
    bufs = [e.put(np.asarray(frm, np.int32)), e.put(np.asarray(to, np.int32)), e.buf(n, np.int32), e.buf(n, np.int32)]
    try:
        bufs[3].upload(np.full(n, CANARY, np.int32))
        e.line_of_sight_batch(bufs[0], bufs[1], n, bufs[2], bufs[3] if want_fb else None, strict)
        return bufs[2].download(), bufs[3].download()
    finally:
        for b in bufs:
            b.free()


def run_rows(e, rows, strict, path_cap=None, way_cap=None, want_idx=True, want_stats=True):
    """One raw pf_smooth_batch launch over `rows` (int arrays; a row may hold anything), every output between canary rows
    -> (way [n, way_cap], idx, way_len, stats [n, 2], status); the canary rows on both sides are checked here."""
    n = len(rows)
    cap = int(path_cap or max([len(r) for r in rows] + [1]))
    wcap = int(way_cap or cap)
    cells, lens = np.full((n, cap), CANARY, np.int32), np.zeros(n, np.int32)
    for i, r in enumerate(rows):
        cells[i, :len(r)] = np.asarray(r, np.int64).astype(np.int32)
        lens[i] = len(r)
    dc, dl = e.put(cells), e.put(lens)
    dw, di = e.put(np.full((n + 2, wcap), CANARY, np.int32)), e.put(np.full((n + 2, wcap), CANARY, np.int32))
    dwl, dss = e.put(np.full(n + 2, CANARY, np.int32)), e.put(np.full(n + 2, CANARY, np.int32))
    dst = e.put(np.full((n + 2, 2), CANARY_F, np.float64))
    try:
        rc = e.L.pf_smooth_batch(e.h, int(strict), n, cap, dc.ptr, dl.ptr, wcap, dw.at(wcap), di.at(wcap) if want_idx else None, dwl.at(1),
                                 dst.at(2) if want_stats else None, dss.at(1))
        assert rc == 0, e.L.pf_last_error(e.h)
        way, idx, wl, stats, status = dw.download(), di.download(), dwl.download(), dst.download(), dss.download()
    finally:
        for b in (dc, dl, dw, di, dwl, dss, dst):
            b.free()
    for a in (way, idx, wl, stats, status):
        assert (a[0] == a.dtype.type(CANARY if a.dtype != np.float64 else CANARY_F)).all()
        assert (a[-1] == a.dtype.type(CANARY if a.dtype != np.float64 else CANARY_F)).all()
    if not want_idx:
        assert (idx == CANARY).all()
    if not want_stats:
        assert (stats == CANARY_F).all()
    return way[1:-1], idx[1:-1], wl[1:-1], stats[1:-1], status[1:-1]


def check_rows(e, occ, rows, strict, path_cap=None, way_cap=None, want_idx=True, want_stats=True):
    """run_rows against the model, row by row -> the statuses."""
    way, idx, wl, stats, status = run_rows(e, rows, strict, path_cap, way_cap, want_idx, want_stats)
    wcap = way.shape[1]
    for i, r in enumerate(rows):
        st, mway, midx, mlen, mturns = sm.smooth_row(occ, r, strict, wcap)
        assert status[i] == st, (i, status[i], st)
        assert wl[i] == len(mway), (i, wl[i], len(mway))
        if st == 3:
            continue                                                 # (the row's contents are unspecified; its neighbours are checked)
        assert np.array_equal(way[i, :wl[i]], mway), (i, way[i, :wl[i]], mway)
        assert (way[i, wl[i]:] == CANARY).all()                      # nothing behind the waypoints; a status-1 row is untouched
        if want_idx:
            assert np.array_equal(idx[i, :wl[i]], midx) and (idx[i, wl[i]:] == CANARY).all()
        if want_stats:
            assert np.array_equal(bits(stats[i]), bits([mlen, float(mturns)])), (i, stats[i], mlen, mturns)
    return status


@pytest.fixture(scope="module")
def fig7():
    g, _, _ = gio.grid("fig7")
    e = Engine(g)
    yield e, sm.occ_of(g)
    e.close()


# ---- 1. every ordered pair of fig7's 400 cells, both modes, one launch each
@pytest.mark.parametrize("strict", [1, 0])
def test_every_pair_of_fig7(fig7, strict):
    e, occ = fig7
    a, b = (v.reshape(-1) for v in np.mgrid[0:400, 0:400])
    vis, fb = los(e, a, b, strict)
    mvis, mfb = sm.all_pairs(occ, strict)
    assert np.array_equal(vis.reshape(400, 400) != 0, mvis)
    assert np.array_equal(fb.reshape(400, 400), mfb)
    assert set(np.unique(vis)) == {0, 1}
    vis2, fb2 = los(e, a[:1000], b[:1000], strict, want_fb=False)    # first_block is optional
    assert np.array_equal(vis2, vis[:1000]) and (fb2 == CANARY).all()


# ---- 2. the rule, cell by cell: one obstacle on each cell of the bounding box in turn
DELTAS = [(0, 6), (6, 0), (5, 5), (3, 7), (7, 3), (2, 4), (1, 64), (64, 1), (65, 64), (63, 64), (129, 128)]
LARGE = {(65, 64), (63, 64), (129, 128)}


@pytest.mark.parametrize("dr, dc", DELTAS)
def test_rule_cell_by_cell(dr, dc):
    N = 140
    g = np.zeros((N, N), np.uint8)
    e = Engine(g)
    dfrom, dto, dvis, dfb = e.buf(2, np.int32), e.buf(2, np.int32), e.buf(2, np.int32), e.buf(2, np.int32)
    rnd = np.random.default_rng(1000 * dr + dc)
    grazes = placements = 0
    try:
        for sr, sc in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            a = (5 if sr > 0 else N - 6, 5 if sc > 0 else N - 6)
            b = (a[0] + sr * dr, a[1] + sc * dc)
            crossed, touched = sm.segment_cells(a, b)
            assert a in crossed and b in crossed
            box = [(r, c) for r in range(min(a[0], b[0]), max(a[0], b[0]) + 1) for c in range(min(a[1], b[1]), max(a[1], b[1]) + 1)]
            if (dr, dc) in LARGE:
                pick = rnd.choice(len(box), 400, replace=False)
                box = sorted(set(box[i] for i in pick) | set(crossed) | set(touched))
            ia, ib = a[0] * N + a[1], b[0] * N + b[1]
            dfrom.upload(np.array([ia, ib], np.int32))
            dto.upload(np.array([ib, ia], np.int32))
            for strict in (1, 0):                                    # the open map: everything sees everything
                e.line_of_sight_batch(dfrom, dto, 2, dvis, dfb, strict)
                assert list(dvis.download()) == [1, 1] and list(dfb.download()) == [-1, -1]
            cset, tset = set(crossed), set(touched)
            grazes += len(tset)
            for cell in box:
                g[cell] = 1
                e.update_grid(g)
                g[cell] = 0
                placements += 1
                for strict in (1, 0):
                    blocked = cell in cset or (strict and cell in tset)
                    e.line_of_sight_batch(dfrom, dto, 2, dvis, dfb, strict)
                    want = -1 if not blocked else cell[0] * N + cell[1]
                    assert list(dvis.download()) == [int(not blocked)] * 2, (a, b, cell, strict)
                    assert list(dfb.download()) == [want, want], (a, b, cell, strict)
    finally:
        for buf in (dfrom, dto, dvis, dfb):
            buf.free()
        e.close()
    assert placements >= 4 * (min(400, (dr + 1) * (dc + 1)))
    if (dr, dc) in ((5, 5), (3, 7), (7, 3)):                        # (|2k| == s needs an even s)
        assert grazes > 0                                            # vertex grazes: strict and loose differ


# ---- 3. thin maps: a box narrower than the run of three minor indices, spans of 64 passes
@pytest.mark.parametrize("R, C", [(1, 4095), (4095, 1), (2, 4095), (4095, 2), (3, 4095), (4095, 3)])
def test_thin_maps(R, C):
    N, W = max(R, C), min(R, C)
    tall = R > C
    g = np.zeros((R, C), np.uint8)
    e = Engine(g)
    cell = (lambda major, minor: (major, minor)) if tall else (lambda major, minor: (minor, major))     # noqa: E731
    ends = [(cell(0, u), cell(N - 1, v)) for u in range(W) for v in range(W)]
    pairs = ends + [(b, a) for a, b in ends]
    frm = [a[0] * C + a[1] for a, _ in pairs]
    to = [b[0] * C + b[1] for _, b in pairs]
    blocked_some = 0
    try:
        for m in (None, 0, 1, 63, 64, 65, N - 2, N - 1):
            for u in range(W if m is not None else 1):
                g[:] = 0
                if m is not None:
                    g[cell(m, u)] = 1
                e.update_grid(g)
                occ = sm.occ_of(g)
                for strict in (1, 0):
                    vis, fb = los(e, frm, to, strict)
                    want = [sm.first_block(occ, a, b, strict) for a, b in pairs]
                    assert list(fb) == want, (m, u, strict)
                    assert list(vis) == [int(w < 0) for w in want]
                    if m is None:
                        assert all(w < 0 for w in want)
                    else:
                        blocked_some += sum(w >= 0 for w in want)
                        if W == 1:                                   # the corridor: the blocker is seen from both ends
                            assert want == [m, m]
    finally:
        e.close()
    assert blocked_some >= 2 * 7


# ---- 4. smoothing
@pytest.mark.parametrize("name", sm.MAPS20 + ("g128crop",))
def test_smooth_case_table(name):
    g, paths = sm.astar_cases(name)
    e = Engine(g)
    try:
        for strict in (1, 0):
            st = check_rows(e, sm.occ_of(g), paths, strict)
            assert (st == 0).all()
    finally:
        e.close()


def test_smooth_thin_case_table():
    for name, g, p in sm.thin_cases():
        e = Engine(g)
        try:
            for strict in (1, 0):
                check_rows(e, sm.occ_of(g), [p], strict)
        finally:
            e.close()


def test_smooth_g256_corner_to_corner():
    import pf_oracle as po
    g, s, t = gio.grid("g256")
    p, _ = po.Oracle(g).astar(s, t, None, 0)
    assert len(p) == 335
    e = Engine(g)
    try:
        for strict in (1, 0):
            check_rows(e, sm.occ_of(g), [p], strict)
    finally:
        e.close()


def test_smooth_the_engines_own_paths():
    """One path per search variant straight from Engine.astar_host, and the facade on top of the same engine."""
    g, cases = sm.astar_cases("g128crop")
    occ = sm.occ_of(g)
    e = Engine(g)
    try:
        rows = []
        for variant in (0, 1, 2):
            far = max(cases[variant::3], key=len)                   # (the table's paths of this variant: a feasible pair, far apart)
            paths, st = e.astar_host(variant, [int(far[0])], [int(far[-1])], path_cap=g.size)
            assert st[0] == 0 and len(paths[0]) > 20
            rows.append(paths[0])
        for strict in (1, 0):
            check_rows(e, occ, rows, strict)
        s = PathSmoother(g, engine=e)
        out = s.smooth(rows)
        for i, r in enumerate(rows):
            st, way, idx, length, turns = sm.smooth_row(occ, r, 1)
            assert np.array_equal(out[i].cells, way) and np.array_equal(s.indices[i], idx) and s.status[i] == 0
            assert bits(s.lengths[i]) == bits(length) and s.turns[i] == turns
            assert out[i].tolist() == [(int(x) // 128, int(x) % 128) for x in way]
        assert s.kernel_ms > 0
        vis = s.visible([((int(r[0]) // 128, int(r[0]) % 128), (int(r[-1]) // 128, int(r[-1]) % 128)) for r in rows] + [((0, 0), (0, 500))])
        want = [sm.first_block(occ, (int(r[0]) // 128, int(r[0]) % 128), (int(r[-1]) // 128, int(r[-1]) % 128), 1) for r in rows]
        assert list(vis) == [w < 0 for w in want] + [False]
        assert s.first_block == [None if w < 0 else (w // 128, w % 128) for w in want] + [None]
        s.close()
        assert e.h                                                   # a passed engine stays open
    finally:
        e.close()


def device_rows_check(s, occ, dc, dl, n, cap):
    """smooth_device on rows in HBM, then everything downloaded for the comparison."""
    dw, dwl, dst, dss, wcap = s.smooth_device(dc, dl, n, cap)
    try:
        assert wcap == cap
        cells, lens = dc.download().reshape(n, cap), dl.download()
        way, wl, stats, status = dw.download(), dwl.download(), dst.download().reshape(n, 2), dss.download()
    finally:
        for b in (dw, dwl, dst, dss):
            b.free()
    kept = 0
    for i in range(n):
        st, mway, _, mlen, mturns = sm.smooth_row(occ, cells[i, :max(lens[i], 0)], int(s.restrict_diagonal_near_obstacle))
        assert status[i] == st and wl[i] == len(mway) and np.array_equal(way[i, :wl[i]], mway), i
        assert np.array_equal(bits(stats[i]), bits([mlen, float(mturns)])), i
        kept += len(mway) >= 4
    return kept


def test_smooth_device_rows_of_a_maaco_walk_and_a_ga_decode():
    import pathfit
    g, s0, t0 = gio.grid("fig13")
    occ = sm.occ_of(g)
    m = pathfit.MAACO(g, 96, 4, 1.0, 7.0, 0.1, 2.5, 1.0, 0.9, 0.2, 0.9, 0.5, 0.1, seed=4)
    e = m.engine
    try:
        n = m.walk_iteration_dev(0)
        dc, dl = m.walk_bufs()[:2]
        for strict in (True, False):
            s = PathSmoother(g, strict, engine=e)
            assert device_rows_check(s, occ, dc, dl, n, m.path_cap) >= 20     # wiggly walks keep many waypoints
        W, n = 2, 80                                               # (a decode never revisits a cell: more waypoints, fewer feasible rows)
        free = np.flatnonzero(g.reshape(-1) != 1)
        wps = np.random.default_rng(9).choice(free, (n, W)).astype(np.int32)
        cap = e.default_path_cap(W)
        dw, dc, dl, dst = e.put(wps), e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
        e.decode_batch(n, W, s0, t0, cap, dc, dl, dst, d_wp_cells=dw)
        assert (dst.download() == 0).sum() >= 40
        for strict in (True, False):
            s = PathSmoother(g, strict, engine=e)
            assert device_rows_check(s, occ, dc, dl, n, cap) >= 20
    finally:
        e.close()


# ---- 5. rows and edges
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(fig7, n):
    e, occ = fig7
    _, paths = sm.astar_cases("fig7")
    rows = [paths[i % len(paths)] for i in range(n)]
    check_rows(e, occ, rows, 1)
    check_rows(e, occ, rows, 0, want_idx=False, want_stats=False)


def test_short_rows_and_exact_fit(fig7):
    e, occ = fig7
    _, paths = sm.astar_cases("fig7")
    p = max(paths, key=len)
    L = len(p)
    rows = [[], [int(p[0])], p[:2], p[:3], p, p[:L - 1], [], p[:3]]
    st = check_rows(e, occ, rows, 1, path_cap=L)                      # a row filled exactly, and one of path_cap - 1
    assert list(st) == [1, 0, 0, 0, 0, 0, 1, 0]
    check_rows(e, occ, rows, 0, path_cap=L)


def test_way_cap_exact_and_one_less(fig7):
    e, occ = fig7
    _, paths = sm.astar_cases("fig7")
    for strict in (1, 0):
        k = [len(sm.smooth(occ, p, strict)) for p in paths]
        top = max(k)
        assert top >= 5
        st = check_rows(e, occ, paths, strict, way_cap=top)          # the longest waypoint list fits exactly
        assert (st == 0).all()
        st = check_rows(e, occ, paths, strict, way_cap=top - 1)      # and no longer: status 3, length 0, the neighbours intact
        assert [int(v) for v in st] == [3 if x == top else 0 for x in k]
        st = check_rows(e, occ, paths, strict, way_cap=1)
        assert (st == 3).all()


def test_cells_outside_the_grid_and_illegal_paths(fig7):
    e, occ = fig7
    _, paths = sm.astar_cases("fig7")
    good = [p for p in paths if len(p) >= 8][:4]
    bad1, bad2, bad3 = good[0].copy(), good[1].copy(), good[2].copy()
    bad1[3] = -1
    bad2[len(bad2) - 1] = 400
    bad3[0] = 2 ** 31 - 1
    rows = [good[0], bad1, good[1], bad2, bad3, good[3]]
    for strict in (1, 0):
        st = check_rows(e, occ, rows, strict)
        assert list(st) == [0, 1, 0, 1, 1, 0]
    ob = int(np.flatnonzero(occ.reshape(-1) == 1)[7])
    free = np.flatnonzero(occ.reshape(-1) != 1)
    wild = [np.array([free[0], free[0], free[5], ob, free[-1], free[2], free[2], free[-3], ob, ob, free[40]], np.int32),   # jumps, repeats, obstacles
            np.array([ob, ob, ob], np.int32), np.array([free[9]] * 70, np.int32),
            np.concatenate([good[0], good[0][::-1], good[1]]).astype(np.int32)]
    for strict in (1, 0):
        st = check_rows(e, occ, wild, strict)
        assert (st == 0).all()


# ---- 6. dynamic map
def test_update_grid_is_seen_by_the_next_call():
    g, paths = sm.astar_cases("fig13")
    occ = sm.occ_of(g)
    s = PathSmoother(g)
    try:
        p = next(p for p in paths if (np.diff(sm.smooth(occ, p, 1))[:1] >= 4).any())      # its first segment skips at least 3 cells
        first = s.smooth([p])[0]
        assert np.array_equal(first.cells, sm.smooth_row(occ, p, 1)[1])
        a, b = first[0], first[1]
        crossed, _ = sm.segment_cells(a, b)
        wall = [c for c in crossed if c not in (a, b)]
        assert wall
        g2 = np.array(g)
        g2[wall[len(wall) // 2]] = 1                                 # a wall across the first long segment
        s.engine.update_grid(g2)
        second = s.smooth([p])[0]
        assert np.array_equal(second.cells, sm.smooth_row(sm.occ_of(g2), p, 1)[1])
        assert not np.array_equal(second.cells, first.cells)
        assert not s.visible([(a, b)])[0] and s.first_block[0] == wall[len(wall) // 2]
    finally:
        s.close()
    with pytest.raises(ValueError, match="closed"):
        s.smooth([p])


# ---- 7. the square roots of segment lengths
def test_square_roots_up_to_two_times_4095_squared(fig7):
    e, _ = fig7
    rnd = np.random.default_rng(12)
    d = rnd.integers(-4095, 4096, (1 << 20, 2)).astype(np.int64)
    arr = np.concatenate([(d * d).sum(axis=1), np.array([0, 1, 2, 3, 4095 ** 2, 4095 ** 2 + 1, 2 * 4095 ** 2 - 1, 2 * 4095 ** 2], np.int64)])
    assert arr.max() == 2 * 4095 ** 2 and (arr > 1 << 21).sum() > 1 << 19       # beyond the earlier self-test's range
    d_in, d_out = e.put(arr), e.buf(arr.size, np.float64)
    try:
        e._ck(e.L.pf_selftest_sqrt(e.h, arr.size, d_in.ptr, d_out.ptr))
        assert np.array_equal(bits(d_out.download()), bits(np.sqrt(arr.astype(np.float64))))
    finally:
        d_in.free()
        d_out.free()


# ---- 8. ABI errors
def test_abi_errors(fig7):
    e, _ = fig7
    L, h = e.L, e.h
    b, b2 = e.put(np.zeros(64, np.int32)), e.buf(64, np.int32)
    d = e.buf(16, np.float64)
    p = b.ptr
    try:
        def failed(rc, word):
            msg = L.pf_last_error(h).decode()
            assert rc < 0 and word in msg, (rc, msg)
        failed(L.pf_line_of_sight_batch(h, 1, -1, p, p, p, p), "pf_line_of_sight_batch")
        failed(L.pf_line_of_sight_batch(h, 1, 4, None, p, p, p), "pf_line_of_sight_batch")
        failed(L.pf_line_of_sight_batch(h, 1, 4, p, None, p, p), "pf_line_of_sight_batch")
        failed(L.pf_line_of_sight_batch(h, 1, 4, p, p, None, p), "pf_line_of_sight_batch")
        assert L.pf_line_of_sight_batch(h, 1, 0, p, p, p, None) == 0
        assert L.pf_line_of_sight_batch(h, 1, 4, p, b.at(8), b2.ptr, None) == 0
        ok = dict(strict=1, n=2, cap=8, cells=p, lens=p, wcap=8, way=p, idx=p, wl=p, st=d.ptr, status=p)

        def smooth(**kw):
            a = dict(ok, **kw)
            return L.pf_smooth_batch(h, a["strict"], a["n"], a["cap"], a["cells"], a["lens"], a["wcap"], a["way"], a["idx"], a["wl"], a["st"], a["status"])
        for kw in (dict(n=-1), dict(cap=0), dict(wcap=0), dict(cells=None), dict(lens=None), dict(way=None), dict(wl=None), dict(status=None)):
            failed(smooth(**kw), "pf_smooth_batch")
        assert smooth(n=0) == 0
        assert smooth(n=0, cells=p) == 0
        assert L.pf_smooth_batch(None, 1, 1, 1, p, p, 1, p, p, p, None, p) < 0 and L.pf_line_of_sight_batch(None, 1, 1, p, p, p, p) < 0
    finally:
        b.free()
        b2.free()
        d.free()
