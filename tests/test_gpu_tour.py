"""Tours on the device (pf_tour_matrix, pf_tour_solve, pathfit.Tour) against the models of tests/tour_checkers.py (pinned by
tests/test_tour_checkers.py).  Every comparison is exact equality, doubles as 64-bit words; every output buffer lies between canary
words.  The table lies in LDS up to m = 9 and in HBM from m = 10 on: both sides of the switch are run."""
import functools

import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import tour_checkers as tc

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64                                                             # canary words in front of and behind every output
LDS_M = 9                                                            # the largest m whose table lies in LDS


def between_canaries(e, n, dtype):
    return e.put(np.full(n + 2 * PAD, CANARY, dtype))


def inner(buf, tag):
    a = buf.download()
    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), tag
    return a[PAD:len(a) - PAD]


@pytest.fixture(scope="module")
def eng():
    from pathfit import Engine
    e = Engine(gio.grid("fig7")[0])
    yield e
    e.close()


def n_of(m, mode):
    return m + (2 if mode == 2 else 1)


@functools.lru_cache(maxsize=None)
def _model(key, mode, need):
    d = np.frombuffer(key, np.float64)
    n = int(round(len(d) ** 0.5))
    d = d.reshape(n, n)
    nd = None if need is None else list(need)
    m = len(tc.middle(n, mode))
    return tc.held_karp_layers(d, mode, nd) if m >= 8 else tc.held_karp(d, mode, nd)


def model(d, mode, need=None):
    return _model(np.ascontiguousarray(d, np.float64).tobytes(), mode, None if need is None else tuple(int(v) for v in need))


def run_solve(e, mats, mode, need=None, want_info=True):
    """One raw Engine call, every output between canaries -> (total [B], order [B, n], status [B], info [B, 4] or None)."""
    from pathfit.engine import _View
    mats = np.ascontiguousarray(mats, np.float64)
    B, n = mats.shape[0], mats.shape[1]
    dm = e.put(mats.reshape(-1))
    tb, ob, sb, ib = between_canaries(e, B, np.float64), between_canaries(e, B * n, np.int32), between_canaries(e, B, np.int32), between_canaries(e, 4 * B, np.int64)
    try:
        e.tour_solve(mode, n, B, dm, _View(e, tb.at(PAD), B, np.float64), _View(e, ob.at(PAD), B * n, np.int32), _View(e, sb.at(PAD), B, np.int32), need,
                     _View(e, ib.at(PAD), 4 * B, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        info = inner(ib, "info").reshape(B, 4)
        if not want_info:
            assert np.all(info == CANARY)
        return inner(tb, "total"), inner(ob, "order").reshape(B, n), inner(sb, "status"), info if want_info else None
    finally:
        for b in (dm, tb, ob, sb, ib):
            b.free()


def check(e, mats, mode, need=None, tag=None):
    mats = np.ascontiguousarray(mats, np.float64)
    tot, order, status, info = run_solve(e, mats, mode, need)
    for b, d in enumerate(mats):
        want = model(d, mode, need)
        got = (tc.bits(tot[b]), list(order[b]), int(info[b, 0]), int(info[b, 1]))
        assert got == (tc.bits(want[0]), list(want[1]), want[2], want[3]), (tag, mode, mats.shape, b, need, tot[b], want[0])
        assert status[b] == (0 if want[0] < tc.INF else 1) and list(info[b, 2:]) == [0, 0]
        if want[0] < tc.INF:
            assert tc.bits(tc.route_cost(d, order[b], mode)) == tc.bits(tot[b])
    return tot, order, status, info


def pair_need(n, mode):
    mid = tc.middle(n, mode)
    need = [0] * n
    if len(mid) >= 2:
        need[mid[0]] |= 1 << mid[-1]
    if len(mid) >= 4:
        need[mid[1]] |= 1 << mid[2]
    return need


# ---- 1. the layer loop's edges, the wavefront, the workgroup, the LDS / HBM switch
@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_small_shapes(eng, m, mode):
    n = n_of(m, mode)
    mats = [tc.matrix(kind, n, seed) for kind in tc.KINDS for seed in (0, 1)]
    check(eng, mats, mode, None, "small")
    check(eng, mats, mode, pair_need(n, mode), "small, need")
    if mode == 2:                                                     # the leg 0 -> end may be missing
        d = tc.matrix("asym", n, 2)
        d[0, n - 1] = tc.INF
        check(eng, [d], mode, None, "small, no direct leg")


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("m", [5, 6, 7, 8, LDS_M, LDS_M + 1])
def test_lane_workgroup_and_switch_borders(eng, m, mode):
    n = n_of(m, mode)
    mats = [tc.matrix(kind, n, 5) for kind in tc.KINDS]
    check(eng, mats, mode, None, "borders")
    check(eng, mats[2:5], mode, pair_need(n, mode), "borders, need")


def test_m_16_with_two_problems(eng):
    mats = [tc.matrix("euclid", 17, 1), tc.matrix("holes", 17, 2)]
    tot, order, status, info = check(eng, mats, 0, None, "m16")
    assert info[0, 0] == 16 << 15                                     # every state of a complete matrix is finite
    check(eng, [tc.matrix("ints", 18, 3)], 2, pair_need(18, 2), "m16 last")


@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_batch_sizes_at_m_6(eng, B):
    mats = [tc.matrix(tc.KINDS[b % 5], 7, b) for b in range(B)]
    check(eng, mats, 1, None if B % 2 else pair_need(7, 1), "batch")


def test_tour_tables_1_2_and_0_give_equal_outputs(eng):
    mats = [tc.matrix(tc.KINDS[b], 12, 7) for b in range(5)]
    need = pair_need(12, 0)
    outs = []
    try:
        for tables in (1, 2, 0):
            eng.set_option("tour_tables", tables)
            outs.append(check(eng, mats, 0, need, f"tables {tables}"))
    finally:
        eng.set_option("tour_tables", 0)
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert a.tobytes() == b.tobytes()


# ---- 2. what the matrices hold
@pytest.mark.parametrize("m", [4, LDS_M + 1])
def test_matrix_content(eng, m):
    for mode in tc.MODES:
        n = n_of(m, mode)
        base = tc.matrix("asym", n, 11)
        zeros, equal = np.zeros((n, n)), np.full((n, n), 2.75)
        row, col, none = base.copy(), base.copy(), np.full((n, n), tc.INF)
        row[2, :] = tc.INF
        col[:, 2] = tc.INF
        dup = base.copy()                                             # stops 1 and 3 are one place
        dup[3, :], dup[:, 3] = dup[1, :], dup[:, 1]
        dup[1, 3] = dup[3, 1] = 0.0
        tot, order, status, info = check(eng, [zeros, equal, row, col, none, dup, base, base.T.copy()], mode, None, "content")
        # a node without a way out can still be the last of an open tour; one without a way in is never reached
        assert list(status[2:5]) == [0 if mode == 0 else 1, 1, 1] and status[0] == 0 and info[4, 0] == 0
        assert np.all(order[3:5] == -1) and (mode != 0 or order[2][-1] == 2)
        if mode != 2:                                                 # ties everywhere: the smallest index is the LAST node, and so on back
            assert list(order[0]) == [0] + list(range(m, 0, -1))
        # one admissible order; a cycle; a middle node that needs the end
        perm = tc.middle(n, mode)[::-1]
        tot, order, status, info = check(eng, [base, equal], mode, tc.chain_need(n, mode, perm), "chain")
        assert list(order[0][1:1 + m]) == perm and info[0, 0] == m
        cyc = [0] * n
        cyc[1], cyc[2] = 1 << 2, 1 << 1
        tot, order, status, info = check(eng, [base], mode, cyc, "cycle")
        assert status[0] == 1 and tot[0] == tc.INF
        if mode == 2:
            blocked = [0] * n
            blocked[2] = 1 << (n - 1)
            assert check(eng, [base], mode, blocked, "needs the end")[2][0] == 1
            ends = [0] * n
            ends[n - 1] = 1 << 1                                      # the end's own needs are always met
            assert check(eng, [base], mode, ends, "the end's needs")[2][0] == 0


def test_info_null_and_five_identical_runs(eng):
    for m in (7, 11):
        mats = [tc.matrix(k, m + 1, 13) for k in tc.KINDS]
        first = run_solve(eng, mats, 0, None, want_info=False)
        assert first[3] is None
        ref = check(eng, mats, 0, None, "identical")
        for _ in range(5):
            again = run_solve(eng, mats, 0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ref))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], ref[:3]))


# ---- 3. pf_tour_matrix
def gather(e, ids, fields_buf):
    from pathfit.engine import _View
    n = len(ids)
    mb = between_canaries(e, n * n, np.float64)
    try:
        e.tour_matrix(ids, fields_buf, _View(e, mb.at(PAD), n * n, np.float64))
        return inner(mb, "matrix").reshape(n, n)
    finally:
        mb.free()


@pytest.mark.parametrize("name,n", [("fig7", 1), ("fig7", 18), ("g256", 7)])
def test_matrix_against_the_downloaded_fields(name, n):
    from pathfit import DistanceField
    g = gio.grid(name)[0]
    stops = tc.free_cells(g, n, 21)
    df = DistanceField(g, sources=stops)
    try:
        ids = np.array([r * g.shape[1] + c for r, c in stops], np.int32)
        got = gather(df.engine, ids, df.buf)
        want = df.fields.reshape(n, -1)[:, ids]
        assert got.tobytes() == want.tobytes()
        assert np.all(np.diag(got) == 0.0)
    finally:
        df.close()


def test_matrix_on_a_thin_map():
    from pathfit import DistanceField
    g = np.zeros((1, 4096), np.uint8)
    g[0, 3000] = 1
    stops = [(0, 0), (0, 4095), (0, 2999), (0, 3001), (0, 64)]
    df = DistanceField(g, sources=stops)
    try:
        ids = np.array([c for _, c in stops], np.int32)
        got = gather(df.engine, ids, df.buf)
        assert got.tobytes() == df.fields.reshape(5, -1)[:, ids].tobytes()
        assert got[0, 2] == 2999.0 and got[0, 1] == tc.INF and got[1, 3] == 1094.0
    finally:
        df.close()


# ---- 4. Tour end to end
def walk_is_legal(g, cells):
    mm = fc.move_masks(g, 1, 1).reshape(-1)
    C = g.shape[1]
    steps = {fc.DR[k] * C + fc.DC[k]: k for k in range(8)}
    for u, v in zip(cells[:-1], cells[1:]):
        k = steps.get(int(v) - int(u))
        if k is None or not (mm[int(u)] >> k) & 1:
            return False
    return True


@pytest.mark.parametrize("name,n,end", [("fig7", 8, "open"), ("fig7", 8, "return"), ("g256", 9, "last")])
def test_tour_end_to_end(name, n, end):
    from pathfit import DistanceField, Engine, Tour
    g = gio.grid(name)[0]
    stops = tc.NN_STOPS if name == "fig7" else tc.free_cells(g, n, 5)
    mode = {"open": 0, "return": 1, "last": 2}[end]
    e = Engine(g)
    t = df = None
    try:
        before = [(3, 1)]
        t = Tour(g, stops, end=end, before=before, engine=e)
        df = DistanceField(g, sources=stops, engine=e)
        ids = [r * g.shape[1] + c for r, c in stops]
        assert t.matrix.tobytes() == df.fields.reshape(n, -1)[:, ids].tobytes()
        need = [0] * n
        need[1] = 1 << 3
        want = tc.held_karp(t.matrix, mode, need)
        assert t.feasible and (tc.bits(t.total), list(t.order), int(t.info[0]), int(t.info[1])) == (tc.bits(want[0]), want[1], want[2], want[3])
        assert tc.bits(t.route_cost(t.order)) == tc.bits(t.total) and t.kernel_ms > 0
        seq = list(t.order) + ([0] if end == "return" else [])
        legs = t.legs()
        rows = df.paths([stops[b] for b in seq[1:]], k=seq[:-1])
        assert len(legs) == len(rows) == len(seq) - 1
        for leg, row in zip(legs, rows):
            assert len(row) > 0 and np.array_equal(leg.cells, row.cells)
        p = t.path()
        assert walk_is_legal(g, p.cells) and len(p) == sum(len(leg) for leg in legs) - (len(legs) - 1)
        at, cells = 0, list(p.cells)
        for s in seq:                                                 # the stops, in order
            at = cells.index(ids[s], at)
    finally:
        for o in (t, df):
            if o is not None:
                o.close()
        e.close()


def test_the_greedy_order_is_dearer_than_the_device_optimum(eng):
    from pathfit import Tour
    t = Tour(gio.grid(tc.NN_MAP)[0], tc.NN_STOPS, engine=eng)
    try:
        greedy = tc.nearest_neighbour(t.matrix, 0)
        assert t.total == 49.62741699796952 and t.route_cost(greedy) == 61.45584412271571 > t.total
    finally:
        t.close()


def two_rooms():
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    g[1, 10] = g[7, 10] = 0
    return g, [(4, 2), (0, 18), (8, 18), (8, 3)]


def test_a_sealed_room_is_infeasible():
    from pathfit import Tour
    g, stops = two_rooms()
    g[1, 10] = g[7, 10] = 1
    t = Tour(g, stops, end="return")
    try:
        assert not t.feasible and t.total == tc.INF and list(t.order) == [-1] * 4 and t.info[1] == -1
        assert t.legs() == [] and len(t.path()) == 0
        assert t.matrix[0, 1] == tc.INF and t.matrix[0, 3] < tc.INF
    finally:
        t.close()


def test_a_door_closed_by_update_grid_changes_the_order():
    from pathfit import DistanceField, Tour
    g, stops = two_rooms()
    t = Tour(g, stops)
    try:
        first = list(t.order)
        assert first == tc.held_karp(t.matrix, 0)[1] == [0, 3, 2, 1]
        g2 = g.copy()
        g2[7, 10] = 1
        t.engine.update_grid(g2)
        t.refresh()
        df = DistanceField(g2, sources=stops, engine=t.engine)
        ids = [r * 21 + c for r, c in stops]
        assert t.matrix.tobytes() == df.fields.reshape(4, -1)[:, ids].tobytes()
        df.close()
        want = tc.held_karp(t.matrix, 0)
        assert (tc.bits(t.total), list(t.order)) == (tc.bits(want[0]), want[1]) and list(t.order) == [0, 3, 1, 2]
        assert walk_is_legal(g2, t.path().cells)
    finally:
        t.close()


def test_cost_map_legs_on_g256():
    from pathfit import Clearance, CostField, Engine, Tour
    g = gio.grid("g256")[0]
    stops = tc.free_cells(g, 6, 9)
    e = Engine(g)
    t = cf = cl = None
    try:
        cl = Clearance(g, engine=e)
        cost = cl.cost_map(margin=4)
        t = Tour(g, stops, end="return", cost=cost, engine=e)
        cf = CostField(g, cost, [[s] for s in stops], engine=e)
        ids = [r * 256 + c for r, c in stops]
        assert t.matrix.tobytes() == cf.fields.reshape(6, -1)[:, ids].tobytes()
        want = tc.held_karp(t.matrix, 1)
        assert (tc.bits(t.total), list(t.order)) == (tc.bits(want[0]), want[1])
        seq = list(t.order) + [0]
        for leg, a, b in zip(t.legs(), seq[:-1], seq[1:]):
            assert len(leg) > 0 and np.array_equal(leg.cells, cf.paths([stops[b]], b=a)[0].cells)
    finally:
        for o in (t, cf, cl):
            if o is not None:
                o.close()
        e.close()


def test_two_tours_and_a_distance_field_take_turns(eng):
    from pathfit import DistanceField, Tour
    from pathfit.tour import join_legs
    g = gio.grid("fig7")[0]
    a = Tour(g, tc.NN_STOPS, engine=eng)
    b = Tour(g, tc.NN_STOPS[::-1], end="last", before=[(2, 5)], engine=eng)
    df = DistanceField(g, sources=tc.NN_STOPS[:3], engine=eng)
    try:
        la, lb = a.legs(), b.legs()
        route = df.paths([tc.NN_STOPS[5]], k=0)[0]
        assert [list(x.cells) for x in a.legs()] == [list(x.cells) for x in la]
        b.refresh()
        assert [list(x.cells) for x in b.legs()] == [list(x.cells) for x in lb] and b.order[-1] == 7
        assert list(b.order).index(2) < list(b.order).index(5)
        a.refresh()
        assert list(a.order) == tc.held_karp(a.matrix, 0)[1] and a.total == 49.62741699796952
        assert df.paths([tc.NN_STOPS[5]], k=0)[0] == route
        assert list(a.path().cells) == list(join_legs(la, 20).cells)
    finally:
        for o in (a, b, df):
            o.close()


# ---- 5. argument errors of the raw ABI
def test_argument_errors_leave_every_output_untouched(eng):
    e, L = eng, eng.L
    RC = e.R * e.C
    n = 5
    tb, ob, sb, ib = between_canaries(e, 4, np.float64), between_canaries(e, 4 * 18, np.int32), between_canaries(e, 4, np.int32), between_canaries(e, 16, np.int64)
    mb = between_canaries(e, 18 * 18, np.float64)
    good = np.array([tc.matrix("asym", n, b) for b in range(3)])
    dm, dbig = e.put(good.reshape(-1)), e.put(np.zeros(19 * 19))
    fields = e.put(np.zeros(2 * RC))
    tot, order, status, info, mat = tb.at(PAD), ob.at(PAD), sb.at(PAD), ib.at(PAD), mb.at(PAD)

    try:
        solve = L.pf_tour_solve
        assert solve(None, 0, n, None, 3, dm.ptr, tot, order, status, info) == -2
        keep = [np.array(w, np.uint32) for w in ([1, 0, 0, 0, 0], [0, 2, 0, 0, 0], [0, 0, 1 << 5, 0, 0])]
        for args, msg in [((0, 0, None, 3, dm.ptr, tot, order, status, info), "n = 0"), ((2, 1, None, 3, dm.ptr, tot, order, status, info), "n = 1"),
                          ((0, 18, None, 1, dbig.ptr, tot, order, status, info), "17 middle nodes"), ((2, 19, None, 1, dbig.ptr, tot, order, status, info), "17 middle nodes"),
                          ((3, n, None, 3, dm.ptr, tot, order, status, info), "mode = 3"), ((-1, n, None, 3, dm.ptr, tot, order, status, info), "mode = -1"),
                          ((0, n, None, 0, dm.ptr, tot, order, status, info), "B = 0"),
                          ((0, n, keep[0].ctypes.data, 3, dm.ptr, tot, order, status, info), "need[0] = 1"),
                          ((0, n, keep[1].ctypes.data, 3, dm.ptr, tot, order, status, info), "node 1 needs itself"),
                          ((0, n, keep[2].ctypes.data, 3, dm.ptr, tot, order, status, info), "names a node >= n = 5"),
                          ((0, n, None, 3, None, tot, order, status, info), "must not be null"), ((0, n, None, 3, dm.ptr, None, order, status, info), "must not be null"),
                          ((0, n, None, 3, dm.ptr, tot, None, status, info), "must not be null"), ((0, n, None, 3, dm.ptr, tot, order, None, info), "must not be null")]:
            assert solve(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode(), (msg, L.pf_last_error(e.h))
        # a NaN and a negative entry: found before anything is written, the smallest (b, i, j) named; the diagonal is never read
        bad = good.copy()
        bad[2, 1, 3], bad[1, 4, 0] = -1.0, np.nan
        bad[0, 2, 2] = np.nan
        dm.upload(bad.reshape(-1))
        assert solve(e.h, 0, n, None, 3, dm.ptr, tot, order, status, info) == -1 and "(b, i, j) = (1, 4, 0)" in L.pf_last_error(e.h).decode()
        bad[1, 4, 0] = 1.0
        dm.upload(bad.reshape(-1))
        assert solve(e.h, 0, n, None, 3, dm.ptr, tot, order, status, info) == -1 and "(b, i, j) = (2, 1, 3)" in L.pf_last_error(e.h).decode()
        bad[2, 1, 3] = -tc.INF
        dm.upload(bad.reshape(-1))
        assert solve(e.h, 0, n, None, 3, dm.ptr, tot, order, status, info) == -1 and "(b, i, j) = (2, 1, 3)" in L.pf_last_error(e.h).decode()
        matrix = L.pf_tour_matrix
        ok, beyond, below = np.array([5, 9], np.int32), np.array([5, RC], np.int32), np.array([-1, 5], np.int32)      # (held: the calls take their addresses)
        assert matrix(None, 2, ok.ctypes.data, fields.ptr, mat) == -2
        for args, msg in [((0, ok.ctypes.data, fields.ptr, mat), "n = 0"), ((2, None, fields.ptr, mat), "must not be null"), ((2, ok.ctypes.data, None, mat), "must not be null"),
                          ((2, ok.ctypes.data, fields.ptr, None), "must not be null"),
                          ((2, beyond.ctypes.data, fields.ptr, mat), f"stop 1 = {RC} lies outside the grid"),
                          ((2, below.ctypes.data, fields.ptr, mat), "stop 0 = -1 lies outside the grid")]:
            assert matrix(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode(), (msg, L.pf_last_error(e.h))
        for b in (tb, ob, sb, ib, mb):
            assert np.all(b.download() == CANARY)
        # the handle still works, and the diagonal may hold anything
        bad[2, 1, 3] = 1.0
        dm.upload(bad.reshape(-1))
        assert solve(e.h, 0, n, None, 3, dm.ptr, tot, order, status, info) == 0
        assert tc.bits(tb.download()[PAD]) == tc.bits(tc.held_karp(bad[0], 0)[0])
    finally:
        for b in (tb, ob, sb, ib, mb, dm, dbig, fields):
            b.free()
