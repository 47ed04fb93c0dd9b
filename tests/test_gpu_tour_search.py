"""The tour search on the device (pf_tour_improve, pathfit.TourSearch) against the numpy model of tests/tour_search_checkers.py
(pinned by tests/test_tour_search_checkers.py).  Every comparison is exact equality, doubles as 64-bit words; every output buffer
lies between canary words.  A workgroup of 1024 threads searches a start, four pairs a thread in flight: the sizes lie about the
multiples of the wavefront, the workgroup and the unrolled step, and reach the largest n."""
import functools

import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import tour_checkers as tc
import tour_search_checkers as ts

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64                                                             # canary words in front of and behind every output
MID_N = 128                                                          # a size with a few pairs per thread and sweep
BIG = 2.0 ** 1000


def between_canaries(e, n, dtype, inside=None):
    a = np.full(n + 2 * PAD, CANARY, dtype)
    if inside is not None:
        a[PAD:PAD + n] = inside
    return e.put(a)


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


@functools.lru_cache(maxsize=None)
def _model(key, n, start, mode, cap):
    return ts.two_opt_numpy(np.frombuffer(key, np.float64).reshape(n, n), list(start), mode, cap)


def model(d, start, mode, cap):
    d = np.ascontiguousarray(d, np.float64)
    return _model(d.tobytes(), d.shape[0], tuple(int(v) for v in start), mode, cap)


def words(order, value, status, info):
    return [int(v) for v in order], tuple(tc.bits(x) for x in value), int(status), tuple(int(v) for v in info)


def run(e, mats, starts, mode, shared, cap, want_info=True):
    """One raw Engine call, every output between canaries -> (order [B, n], value [B, 2], status [B], info [B, 4])."""
    from pathfit.engine import _View
    mats = np.ascontiguousarray(mats, np.float64)
    starts = np.ascontiguousarray(starts, np.int32)
    B, n = starts.shape
    assert mats.shape == ((n, n) if shared else (B, n, n))
    dm = e.put(mats.reshape(-1))
    ob = between_canaries(e, B * n, np.int32, starts.reshape(-1))
    vb, sb, ib = between_canaries(e, 2 * B, np.float64), between_canaries(e, B, np.int32), between_canaries(e, 4 * B, np.int64)
    try:
        e.tour_improve(mode, n, B, shared, dm, cap, _View(e, ob.at(PAD), B * n, np.int32), _View(e, vb.at(PAD), 2 * B, np.float64),
                       _View(e, sb.at(PAD), B, np.int32), _View(e, ib.at(PAD), 4 * B, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        info = inner(ib, "info").reshape(B, 4)
        assert want_info or np.all(info == CANARY)
        return inner(ob, "order").reshape(B, n), inner(vb, "value").reshape(B, 2), inner(sb, "status"), info
    finally:
        for b in (dm, ob, vb, sb, ib):
            b.free()


def check(e, mats, starts, mode, shared=False, cap=None, tag=None):
    mats = np.ascontiguousarray(mats, np.float64)
    starts = np.ascontiguousarray(starts, np.int32)
    B, n = starts.shape
    cap = 16 * n if cap is None else cap
    order, value, status, info = run(e, mats, starts, mode, shared, cap)
    for b in range(B):
        want = model(mats if shared else mats[b], starts[b], mode, cap)
        assert words(order[b], value[b], status[b], info[b]) == words(*want), (tag, mode, n, B, b)
    return order, value, status, info


def identity(n):
    return list(range(n))


def reversed_middle(n, mode):
    return [0] + list(range(ts.hi_of(n, mode), 0, -1)) + ([n - 1] if mode == 2 and n > 1 else [])


def shuffled(n, mode, seed):
    hi = ts.hi_of(n, mode)
    mid = np.random.default_rng([seed, n, mode]).permutation(np.arange(1, hi + 1))
    return [0] + [int(v) for v in mid] + ([n - 1] if mode == 2 and n > 1 else [])


def nn(d, mode):
    return tc.nearest_neighbour(ts.mirror(d), mode)[:len(d)]          # (n = 1 in mode 2: node 0 is the start and the end)


# ---- 1. sizes: the first pairs, the wavefront's and the workgroup's borders
@pytest.mark.parametrize("mode", ts.MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_the_smallest_sizes(eng, n, mode):
    for kind in ("ints", "tenths", "euclid"):
        mats = [ts.matrix(kind, n, s) for s in range(4)]
        for starts in ([nn(d, mode) for d in mats], [reversed_middle(n, mode)] * 4, [shuffled(n, mode, s) for s in range(4)]):
            order, value, status, info = check(eng, mats, starts, mode, tag=kind)
            assert np.all(status == 0) and np.all(info[:, 1] == info[:, 0] + 1)
            if ts.hi_of(n, mode) < 2 or (mode == 1 and n == 3):       # no pair at all; or every delta 0
                assert not info[:, 0].any() and order.tolist() == [list(s) for s in starts]


@pytest.mark.parametrize("mode", ts.MODES)
@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_sizes_about_the_wavefront_and_the_workgroup(eng, n, mode):
    d, t = ts.matrix("euclid", n, 3), ts.matrix("ints", n, 3)
    order, value, status, info = check(eng, [d, d, t], [identity(n), nn(d, mode), identity(n)], mode, tag="sizes")
    assert np.all(status == 0) and info[0, 0] > n // 8 and np.all(value[:, 0] <= value[:, 1])
    for o in order:
        assert tc.admissible(o, n, mode, None)
    assert ts.improving_pairs(d, order[0], mode) == []


def test_the_largest_size_under_a_cap_of_eight_moves(eng):
    n = ts.MAX_N
    d = ts.matrix("euclid", n, 1)
    order, value, status, info = check(eng, d, [identity(n), shuffled(n, 1, 4)], 1, shared=True, cap=8, tag="largest")
    assert list(status) == [2, 2] and info[:, :2].tolist() == [[8, 9], [8, 9]] and np.all(value[:, 0] < value[:, 1])
    assert tc.admissible(order[0], n, 1, None) and tc.admissible(order[1], n, 1, None)


# ---- 2. batches and starts
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_batch_sizes_at_n_12(eng, B, shared):
    n, mode = 12, B % 3
    kinds = ("ints", "uniform", "euclid", "tenths")
    starts = [shuffled(n, mode, b) for b in range(B)]
    if shared:
        check(eng, ts.matrix("euclid", n, 7), starts, mode, shared=True, tag="batch")
        return
    mats = [ts.matrix(kinds[b % 4], n, b) for b in range(B)]
    if B >= 3:
        mats[1][2, 9] = ts.INF                                        # one problem of the batch is not searched
    order, value, status, info = check(eng, mats, starts, mode, tag="batch")
    assert list(status) == [1 if (b == 1 and B >= 3) else 0 for b in range(B)]
    if B >= 3:
        assert np.all(order[1] == -1) and np.all(value[1] == ts.INF) and not info[1].any()


@pytest.mark.parametrize("n", [9, MID_N + 2])
def test_a_local_optimum_its_reversal_and_the_cap(eng, n):
    d = ts.matrix("euclid", n, 5)
    for mode in ts.MODES:
        full = model(d, identity(n), mode, 16 * n)
        best, moves = full[0], full[3][0]
        assert full[2] == 0 and moves >= 3
        back = [0] + best[1:ts.hi_of(n, mode) + 1][::-1] + ([n - 1] if mode == 2 else [])
        order, value, status, info = check(eng, d, [best, back, identity(n)], mode, shared=True, tag="optimum")
        assert info[0].tolist() == [0, 1, 0, 0] and order[0].tolist() == best and tc.bits(value[0, 0]) == tc.bits(value[0, 1])
        caps = (0, 1, moves - 1, moves)
        for cap in caps:
            order, value, status, info = check(eng, d, [identity(n), best], mode, shared=True, cap=cap, tag="cap")
            assert list(status) == [0 if cap == moves else 2, 0] and info[0, :2].tolist() == [cap, cap + 1]
            assert cap or order[0].tolist() == identity(n)


def test_info_null_and_five_identical_runs(eng):
    for n in (11, MID_N + 3):
        mats = [ts.matrix(k, n, 13) for k in ("ints", "uniform", "euclid", "tenths")]
        starts = [shuffled(n, 2, b) for b in range(4)]
        first = run(eng, mats, starts, 2, False, 16 * n, want_info=False)
        ref = check(eng, mats, starts, 2, tag="identical")
        for _ in range(5):
            again = run(eng, mats, starts, 2, False, 16 * n)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ref))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], ref[:3]))


# ---- 3. what the matrices hold
@pytest.mark.parametrize("n", [7, MID_N + 5])
def test_matrix_content(eng, n):
    base = ts.matrix("uniform", n, 11)
    equal = np.full((n, n), 2.75)
    junk = base.copy()
    junk[np.tril_indices(n)] = np.resize([np.nan, -1.0, -ts.INF, 2.0 ** 1010, ts.INF], n * (n + 1) // 2)   # never read
    hole = base.copy()
    hole[0, n - 1] = ts.INF
    big = np.where(ts.matrix("ints", n, 5) == 1.0, BIG, np.where(ts.matrix("ints", n, 6) == 1.0, 0.0, base))
    mats = [ts.matrix("ints", n, 2), equal, ts.matrix("tenths", n, 2), junk, hole, big, base]
    for mode in ts.MODES:
        starts = [shuffled(n, mode, b) for b in range(6)] + [shuffled(n, mode, 3)]
        order, value, status, info = check(eng, mats, starts, mode, tag="content")
        assert list(status) == [0, 0, 0, 0, 1, 0, 0]
        assert not info[1, 0] and order[1].tolist() == starts[1]      # all entries equal: every delta is 0
        assert words(order[3], value[3], status[3], info[3]) == words(order[6], value[6], status[6], info[6])
        assert np.all(order[4] == -1) and np.all(value[4] == ts.INF)
        assert np.isfinite(value[5]).all() and value[5, 1] >= BIG


# ---- 4. TourSearch end to end
def walk_is_legal(g, cells):
    mm = fc.move_masks(g, 1, 1).reshape(-1)
    C = g.shape[1]
    steps = {fc.DR[k] * C + fc.DC[k]: k for k in range(8)}
    for u, v in zip(cells[:-1], cells[1:]):
        k = steps.get(int(v) - int(u))
        if k is None or not (mm[int(u)] >> k) & 1:
            return False
    return True


def reachable_cells(g, count, seed):
    """`count` distinct seeded cells of one connected region of the map (the region of the first seeded free cell)."""
    from pathfit import DistanceField
    df = DistanceField(g, sources=tc.free_cells(g, 1, seed))
    try:
        ids = np.flatnonzero(np.isfinite(df.fields.reshape(-1)))
    finally:
        df.close()
    pick = np.random.default_rng(seed).choice(ids, count, replace=False)
    return [(int(v) // g.shape[1], int(v) % g.shape[1]) for v in pick]


def against_the_model(t, g, stops, fields, search):
    """The matrix against the gathered fields (float64 [n, R * C]); order, total, history and moves against the model."""
    ids = [r * g.shape[1] + c for r, c in stops]
    want_m = np.ascontiguousarray(fields[:, ids])
    assert t.matrix.tobytes() == ts.mirror(want_m).tobytes()
    want = ts.search(want_m, t.mode, max_moves=t.max_moves, **search)
    assert t.feasible == want["feasible"] and list(t.order) == list(want["order"]) and t.moves == want["moves"]
    assert [tc.bits(x) for x in [t.total, t.start_total] + t.history] == [tc.bits(x) for x in [want["total"], want["start_total"]] + want["history"]]
    if t.feasible:
        assert tc.bits(t.route_cost(t.order)) == tc.bits(t.total) and tc.admissible(t.order, len(stops), t.mode, None)
    return want


def legs_against_distance_field(t, df, g, stops):
    ids = [r * g.shape[1] + c for r, c in stops]
    seq = list(t.order) + ([0] if t.mode == 1 else [])
    legs = t.legs()
    rows = df.paths([stops[b] for b in seq[1:]], k=seq[:-1])
    assert len(legs) == len(rows) == len(seq) - 1
    for leg, row in zip(legs, rows):
        assert len(row) > 0 and np.array_equal(leg.cells, row.cells)
    p = t.path()
    assert walk_is_legal(g, p.cells) and len(p) == sum(len(leg) for leg in legs) - (len(legs) - 1)
    at, cells = 0, list(p.cells)
    for s in seq:                                                     # the stops, in order
        at = cells.index(ids[s], at)


@pytest.mark.parametrize("name,end", [("fig7", "open"), ("fig7", "return"), ("g256", "last")])
def test_tour_search_end_to_end(name, end):
    from pathfit import DistanceField, Engine, TourSearch
    g = gio.grid(name)[0]
    stops = ts.MAP_STOPS if name == "fig7" else reachable_cells(g, 40, 5)
    search = ts.MAP_SEARCH if name == "fig7" else dict(starts=5, rounds=2, seed=9)
    e = Engine(g)
    t = df = None
    try:
        t = TourSearch(g, stops, end=end, engine=e, **search)
        df = DistanceField(g, sources=stops, engine=e)
        against_the_model(t, g, stops, df.fields.reshape(len(stops), -1), search)
        assert t.feasible and t.kernel_ms > 0 and len(t.history) == search["rounds"] + 1
        if (name, end) == ("fig7", "open"):
            assert (t.start_total, t.history[0], t.total) == (ts.MAP_NN_TOTAL, ts.MAP_TWO_OPT_TOTAL, ts.MAP_ROUNDS_TOTAL)
        legs_against_distance_field(t, df, g, stops)
    finally:
        for o in (t, df):
            if o is not None:
                o.close()
        e.close()


def test_fields_in_three_chunks_and_a_released_chunk_is_computed_again(monkeypatch):
    from pathfit import DistanceField, TourSearch
    g = gio.grid("fig7")[0]
    stops = ts.MAP_STOPS[:7]
    whole = TourSearch(g, stops, end="return", starts=4, rounds=2)
    monkeypatch.setattr(TourSearch, "CHUNK_BYTES", 3 * 400 * 8)       # three rows of the 20 x 20 map at a time: chunks of 3, 3 and 1
    t = TourSearch(g, stops, end="return", starts=4, rounds=2, engine=whole.engine)
    df = DistanceField(g, sources=stops, engine=whole.engine)
    try:
        assert t.chunk == 3 and whole.chunk == 7
        assert t.matrix.tobytes() == whole.matrix.tobytes() and list(t.order) == list(whole.order) and t.history == whole.history
        for _ in range(2):
            assert [list(p.cells) for p in t.legs()] == [list(p.cells) for p in whole.legs()]
        against_the_model(t, g, stops, df.fields.reshape(7, -1), dict(starts=4, rounds=2, seed=0))
        legs_against_distance_field(t, df, g, stops)
    finally:
        for o in (t, df, whole):
            o.close()


def test_never_below_the_exact_optimum_at_12_stops(eng):
    from pathfit import Tour, TourSearch
    g = gio.grid("fig7")[0]
    for end in ("open", "return", "last"):
        t = TourSearch(g, ts.MAP_STOPS[:12], end=end, engine=eng)
        try:
            exact = Tour.solve_matrices(eng, t.matrix, end=end)[0][0]
            assert t.feasible and t.total >= exact > 0 and t.total <= t.history[0] <= t.start_total
        finally:
            t.close()


def two_rooms():
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    g[1, 10] = g[7, 10] = 0
    return g, [(4, 2), (0, 18), (8, 18), (8, 3), (2, 5), (6, 14)]


def test_a_stop_in_a_sealed_room_is_infeasible():
    from pathfit import TourSearch
    g, stops = two_rooms()
    g[1, 10] = g[7, 10] = 1
    t = TourSearch(g, stops, end="return")
    try:
        assert not t.feasible and t.total == ts.INF and t.start_total == ts.INF and list(t.order) == [-1] * 6 and t.history == [ts.INF] and t.moves == 0
        assert t.legs() == [] and len(t.path()) == 0 and t.matrix[0, 1] == ts.INF and t.matrix[0, 3] < ts.INF
    finally:
        t.close()


def test_refresh_after_update_grid():
    from pathfit import DistanceField, TourSearch
    g, stops = two_rooms()
    search = dict(starts=4, rounds=2, seed=1)
    t = TourSearch(g, stops, **search)
    try:
        first = t.total
        g2 = g.copy()
        g2[7, 10] = 1
        t.engine.update_grid(g2)
        t.refresh()
        df = DistanceField(g2, sources=stops, engine=t.engine)
        try:
            against_the_model(t, g2, stops, df.fields.reshape(6, -1), search)
            legs_against_distance_field(t, df, g2, stops)
        finally:
            df.close()
        assert t.feasible and t.total > first
    finally:
        t.close()


def test_cost_map_legs_on_g256():
    from pathfit import Clearance, CostField, Engine, TourSearch
    g = gio.grid("g256")[0]
    stops = reachable_cells(g, 9, 9)
    search = dict(starts=3, rounds=1, seed=2)
    e = Engine(g)
    t = cf = cl = None
    try:
        cl = Clearance(g, engine=e)
        cost = cl.cost_map(margin=4)
        t = TourSearch(g, stops, end="return", cost=cost, engine=e, **search)
        cf = CostField(g, cost, [[s] for s in stops], engine=e)
        against_the_model(t, g, stops, cf.fields.reshape(9, -1), search)
        seq = list(t.order) + [0]
        for leg, a, b in zip(t.legs(), seq[:-1], seq[1:]):
            assert len(leg) > 0 and np.array_equal(leg.cells, cf.paths([stops[b]], b=a)[0].cells)
    finally:
        for o in (t, cf, cl):
            if o is not None:
                o.close()
        e.close()


def test_a_tour_search_a_tour_and_an_assignment_take_turns(eng):
    import assign_checkers as ac
    from pathfit import Assignment, Tour, TourSearch
    g = gio.grid("fig7")[0]
    s = TourSearch(g, ts.MAP_STOPS, engine=eng, **ts.MAP_SEARCH)
    tour = Tour(g, tc.NN_STOPS, engine=eng)
    a = Assignment(g, ac.GREEDY_ROBOTS, ac.GREEDY_TASKS, engine=eng)
    try:
        ls, lt, pa = s.legs(), tour.legs(), a.paths()
        tour.refresh()
        assert [list(x.cells) for x in s.legs()] == [list(x.cells) for x in ls]
        s.refresh()
        a.refresh()
        assert s.total == ts.MAP_ROUNDS_TOTAL and [list(x.cells) for x in s.legs()] == [list(x.cells) for x in ls]
        assert tour.total == 49.62741699796952 and [list(x.cells) for x in tour.legs()] == [list(x.cells) for x in lt]
        assert a.total == ac.GREEDY_OPTIMUM and [list(p.cells) for p in a.paths()] == [list(p.cells) for p in pa]
    finally:
        for o in (s, tour, a):
            o.close()


def test_solve_matrices(eng):
    from pathfit import TourSearch
    mats = np.array([ts.matrix(k, 10, 2) for k in ("ints", "uniform", "euclid")])
    out = TourSearch.solve_matrices(eng, mats, end="last")
    for b in range(3):
        assert words(out.order[b], out.value[b], out.status[b], out.info[b]) == words(*model(mats[b], nn(mats[b], 2), 2, 160))
    starts = [shuffled(10, 1, b) for b in range(5)]
    out = TourSearch.solve_matrices(eng, mats[2], starts, end="return", shared=True, max_moves=2)
    for b in range(5):
        assert words(out.order[b], out.value[b], out.status[b], out.info[b]) == words(*model(mats[2], starts[b], 1, 2))


# ---- 5. argument errors of the raw ABI
def test_argument_errors_leave_every_output_untouched(eng):
    e, L = eng, eng.L
    n, B = 5, 3
    good = np.array([ts.matrix("uniform", n, b) for b in range(B)])
    rows = np.array([shuffled(n, 2, b) for b in range(B)], np.int32)
    held = np.full(B * n + 2 * PAD, CANARY, np.int32)
    held[PAD:PAD + B * n] = rows.reshape(-1)
    ob, vb, sb, ib = e.put(held), between_canaries(e, 2 * B, np.float64), between_canaries(e, B, np.int32), between_canaries(e, 4 * B, np.int64)
    dm = e.put(good.reshape(-1))
    order, value, status, info = ob.at(PAD), vb.at(PAD), sb.at(PAD), ib.at(PAD)
    try:
        improve = L.pf_tour_improve
        assert improve(None, 0, n, B, 0, dm.ptr, 9, order, value, status, info) == -2
        for args, msg in [((3, n, B, 0, dm.ptr, 9, order, value, status, info), "mode = 3"), ((-1, n, B, 0, dm.ptr, 9, order, value, status, info), "mode = -1"),
                          ((0, 0, B, 0, dm.ptr, 9, order, value, status, info), "n = 0"), ((0, 1025, B, 0, dm.ptr, 9, order, value, status, info), "n = 1025"),
                          ((0, n, 0, 0, dm.ptr, 9, order, value, status, info), "B = 0"), ((0, n, B, 2, dm.ptr, 9, order, value, status, info), "shared = 2"),
                          ((0, n, B, -1, dm.ptr, 9, order, value, status, info), "shared = -1"), ((0, n, B, 0, dm.ptr, -1, order, value, status, info), "max_moves = -1"),
                          ((0, n, B, 0, dm.ptr, (1 << 20) + 1, order, value, status, info), "max_moves = 1048577"),
                          ((0, n, B, 0, None, 9, order, value, status, info), "must not be null"), ((0, n, B, 0, dm.ptr, 9, None, value, status, info), "must not be null"),
                          ((0, n, B, 0, dm.ptr, 9, order, None, status, info), "must not be null"), ((0, n, B, 0, dm.ptr, 9, order, value, None, info), "must not be null")]:
            assert improve(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode(), (msg, L.pf_last_error(e.h))
        # a NaN, a negative entry and an entry beyond 2^1000 in an upper triangle: the smallest (b, i, j) is named
        bad = good.copy()
        bad[2, 1, 3], bad[1, 3, 4], bad[0, 4, 0], bad[0, 2, 2] = -1.0, np.nan, np.nan, -3.0        # (the last two are never read)
        assert ts.first_bad_entry(bad) == (1, 3, 4)
        dm.upload(bad.reshape(-1))
        assert improve(e.h, 2, n, B, 0, dm.ptr, 9, order, value, status, info) == -1 and "(b, i, j) = (1, 3, 4)" in L.pf_last_error(e.h).decode()
        bad[1, 3, 4] = BIG
        dm.upload(bad.reshape(-1))
        assert improve(e.h, 2, n, B, 0, dm.ptr, 9, order, value, status, info) == -1 and "(b, i, j) = (2, 1, 3)" in L.pf_last_error(e.h).decode()
        bad[2, 1, 3], bad[2, 3, 4] = 1.0, 2.0 ** 1001
        dm.upload(bad.reshape(-1))
        assert improve(e.h, 2, n, B, 0, dm.ptr, 9, order, value, status, info) == -1 and "(b, i, j) = (2, 3, 4)" in L.pf_last_error(e.h).decode()
        dm.upload(good.reshape(-1))
        # a bad start row: the smallest (b, position) is named
        r1 = [int(v) for v in rows[1]]
        for change, mode, at in [({(2, 3): int(rows[2, 1])}, 0, (2, 3)), ({(1, 0): r1[2], (1, 2): 0, (2, 3): int(rows[2, 1])}, 0, (1, 0)), ({(1, 2): n}, 1, (1, 2)),
                                 ({(0, 4): -1}, 0, (0, 4)), ({(1, 4): r1[1], (1, 1): n - 1}, 2, (1, 4))]:
            broken = rows.copy()
            for (b, p), v in change.items():
                broken[b, p] = v
            assert ts.first_bad_start(broken, n, mode) == at
            held[PAD:PAD + B * n] = broken.reshape(-1)
            ob.upload(held)
            assert improve(e.h, mode, n, B, 0, dm.ptr, 9, order, value, status, info) == -1
            assert f"(b, position) = ({at[0]}, {at[1]})" in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
            assert np.array_equal(ob.download(), held)
        for b in (vb, sb, ib):
            assert np.all(b.download() == CANARY)
        # the handle still works
        held[PAD:PAD + B * n] = rows.reshape(-1)
        ob.upload(held)
        assert improve(e.h, 2, n, B, 0, dm.ptr, 9, order, value, status, info) == 0
        want = model(good[0], rows[0], 2, 9)
        assert tc.bits(vb.download()[PAD]) == tc.bits(want[1][0]) and list(ob.download()[PAD:PAD + n]) == want[0]
    finally:
        for b in (ob, vb, sb, ib, dm):
            b.free()
