"""The min-max fleet routes on the device (pf_fleet_balance, pathfit.FleetTours(objective="makespan")) against the numpy model of
tests/fleet_balance_checkers.py (pinned by tests/test_fleet_balance_checkers.py).  Every comparison is exact equality, doubles as
64-bit words; every output buffer lies between canary words.  The kernel is pf_fleet_improve's workgroup under another price: the
sizes lie about the multiples of the wavefront, the workgroup and the unrolled step and reach the largest N, the starts hold ties at
the span (the pick among the three largest lengths) and moves that leave the critical route alone.  Where the cap on the moves is
not what a case is about, its inputs end with status 0 in the model."""
import functools

import numpy as np
import pytest

import fleet_balance_checkers as fb
import fleet_checkers as fl
import golden_io as gio
import tour_checkers as tc
from test_gpu_fleet import BIG, CANARY, PAD, all_on, between_canaries, ceil_caps, inner, legs_against_distance_field, reachable_cells, two_rooms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pathfit import Engine
    e = Engine(gio.grid("fig7")[0])
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _model(key, N, start, k, mode, cap, limit):
    return fb.balance_numpy(np.frombuffer(key, np.float64).reshape(N, N), list(start), k, mode, None if cap is None else list(cap), limit)


def model(d, start, k, mode, cap, limit):
    d = np.ascontiguousarray(d, np.float64)
    return _model(d.tobytes(), d.shape[0], tuple(int(v) for v in start), k, mode, None if cap is None else tuple(int(c) for c in cap), limit)


def words(route, lens, value, status, info):
    return [int(v) for v in route], tuple(tc.bits(x) for x in lens), tuple(tc.bits(x) for x in value), int(status), tuple(int(v) for v in info)


def run(e, mats, starts, k, mode, shared, cap, limit, want_info=True):
    """One raw Engine call, every output between canaries -> (route [B, N], len [B, k], value [B, 4], status [B], info [B, 5])."""
    from pathfit.engine import _View
    mats = np.ascontiguousarray(mats, np.float64)
    starts = np.ascontiguousarray(starts, np.int32)
    B, N = starts.shape
    assert mats.shape == ((N, N) if shared else (B, N, N))
    dm = e.put(mats.reshape(-1))
    dc = None if cap is None else e.put(np.array(cap, np.int32))
    ob = between_canaries(e, B * N, np.int32, starts.reshape(-1))
    lb, vb = between_canaries(e, B * k, np.float64), between_canaries(e, 4 * B, np.float64)
    sb, ib = between_canaries(e, B, np.int32), between_canaries(e, 5 * B, np.int64)
    try:
        e.fleet_balance(mode, k, N - k, B, shared, dm, dc, limit, _View(e, ob.at(PAD), B * N, np.int32), _View(e, lb.at(PAD), B * k, np.float64),
                        _View(e, vb.at(PAD), 4 * B, np.float64), _View(e, sb.at(PAD), B, np.int32), _View(e, ib.at(PAD), 5 * B, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        info = inner(ib, "info").reshape(B, 5)
        assert want_info or np.all(info == CANARY)
        return inner(ob, "route").reshape(B, N), inner(lb, "len").reshape(B, k), inner(vb, "value").reshape(B, 4), inner(sb, "status"), info
    finally:
        for b in (dm, dc, ob, lb, vb, sb, ib):
            if b is not None:
                b.free()


def check(e, mats, starts, k, mode, shared=False, cap=None, limit=None, tag=None):
    mats = np.ascontiguousarray(mats, np.float64)
    starts = np.ascontiguousarray(starts, np.int32)
    B, N = starts.shape
    limit = 16 * N if limit is None else limit
    route, lens, value, status, info = run(e, mats, starts, k, mode, shared, cap, limit)
    for b in range(B):
        want = model(mats if shared else mats[b], starts[b], k, mode, cap, limit)
        assert words(route[b], lens[b], value[b], status[b], info[b]) == words(*want), (tag, k, N, mode, B, b)
        assert status[b] == 1 or fl.valid_row(route[b], k, N, cap)
    return route, lens, value, status, info


# ---- 1. sizes, empty routes, ties at the span
@pytest.mark.parametrize("mode", fl.MODES)
@pytest.mark.parametrize("k,n", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (2, 5)])
def test_the_smallest_shapes(eng, k, n, mode):
    N = k + n
    for kind in ("ints", "euclid"):
        mats = [fl.matrix(kind, N, s) for s in range(4)]
        for starts in ([fl.start_row(fl.mirror(d), k) for d in mats], [all_on(k, n, 0)] * 4, [all_on(k, n, k - 1)] * 4, [fl.random_row(k, n, s) for s in range(4)]):
            route, lens, value, status, info = check(eng, mats, starts, k, mode, tag=kind)
            assert np.all(status == 0) and np.all(info[:, 1] == info[:, 0] + 1) and np.all(info[:, 0] == info[:, 2] + info[:, 3]) and np.all(info[:, 4] <= info[:, 0])
            assert np.all(value[:, 0] <= value[:, 2])
            if N == 2:
                assert not info[:, 0].any() and route.tolist() == [list(s) for s in starts]


def test_all_tasks_on_one_robot_and_empty_first_middle_and_last_routes(eng):
    k, n = 4, 9
    starts = [all_on(k, n, r) for r in range(k)] + [fl.row_of([[], [4, 5, 6, 7], [8, 9], [10, 11, 12]]), fl.row_of([[4, 5, 6], [], [], [7, 8, 9, 10, 11, 12]]),
                                                    fl.row_of([[4, 12], [5, 6, 7, 8, 9, 10, 11], [], []]), fl.row_of([[], [4, 5, 6, 7, 8, 9, 10, 11, 12], [], []])]
    for kind in ("euclid", "ints"):
        d = fl.matrix(kind, k + n, 2)
        for mode in fl.MODES:
            route, lens, value, status, info = check(eng, d, starts, k, mode, shared=True, tag="empty")
            assert np.all(status == 0) and np.all(info[:, 3] > 0) and np.all(info[:, 4] > 0) and np.all(value[:4, 0] < value[:4, 2])
            if kind == "ints":
                assert all(fb.improving_candidates(d, route[b], k, mode, None) == [] for b in (0, 5))


def test_two_and_three_routes_tied_at_the_span(eng):
    """Equal weights: a route's length is its number of tasks (one more for the way home), so the starts below hold two, three and
    four routes at the span, and the largest length outside a candidate's routes is the second or third of the top three."""
    moved = 0
    for k, lists in ((3, [[3, 4, 5], [6, 7, 8], []]), (3, [[3, 4], [5, 6], [7, 8]]), (4, [[4, 5, 6], [7, 8, 9], [10, 11, 12], []]), (3, [[3, 4, 5, 6], [7, 8, 9, 10], [11]]),
                     (5, [[5, 6], [7, 8], [9, 10], [11, 12], []]), (2, [[2, 3, 4], [5, 6, 7]])):
        N = k + sum(len(x) for x in lists)
        ones, ints = np.full((N, N), 1.0), fl.matrix("ints", N, 1)
        start = fl.row_of(lists)
        for mode in fl.MODES:
            lens = fl.lengths(fl.mirror(ones), start, k, mode)[0]
            assert lens.count(max(lens)) >= 2
            route, lens, value, status, info = check(eng, [ones, ints], [start, start], k, mode, tag="ties")
            assert np.all(status == 0) and np.all(value[:, 0] <= value[:, 2])
            moved += int(info[:, 0].sum())
            # (one move shortens one of the tied routes: where its delta is not < 0 the rule stops, so the deal need not end even)
    assert moved > 0


@pytest.mark.parametrize("kind,seed", [("ints", 2), ("euclid", 3)])
def test_the_best_move_may_leave_the_critical_route_alone(eng, kind, seed):
    k, n, mode = 4, 8, 1
    d, start = fl.matrix(kind, k + n, seed), fl.random_row(k, n, seed)
    route, lens, value, status, info = check(eng, d, [start], k, mode, shared=True, tag="plateau")
    assert status[0] == 0 and 0 < info[0, 4] < info[0, 0]             # some applied moves kept the span and shortened another route
    trace, w = [], fl.mirror(d)
    fb.balance(d, start, k, mode, None, 16 * (k + n), trace=trace)
    alone = 0
    for sp, delta, code, i, j, was, now in trace:
        before = fl.lengths(w, was, k, mode)[0]
        alone += fl.split(was, k)[before.index(max(before))] == fl.split(now, k)[before.index(max(before))] and before.count(max(before)) == 1
    assert alone > 0


@pytest.mark.parametrize("k", [1, 3, 17])
@pytest.mark.parametrize("N", [63, 64, 65, 255, 256, 257])
def test_sizes_about_the_wavefront_and_the_workgroup(eng, N, k):
    n = N - k
    limit = 16 * N if N <= 65 else 10                                 # (the model takes a sweep of the larger sizes in tens of ms)
    d, t = fl.matrix("euclid", N, 3), fl.matrix("ints", N, 3)
    for mode in fl.MODES:
        starts = [fl.random_row(k, n, 3), fl.start_row(fl.mirror(d), k), fl.random_row(k, n, 4)]
        route, lens, value, status, info = check(eng, [d, d, t], starts, k, mode, limit=limit, tag="sizes")
        assert np.all(value[:, 0] <= value[:, 2]) and info[0, 0] >= 10 and np.all(status == (0 if N <= 65 else 2))
        assert N > 65 or fb.improving_candidates(t, route[2], k, mode, None) == []


def test_the_largest_size_under_a_cap_of_eight_moves(eng):
    N, k = fl.MAX_N, 8
    d = fl.matrix("euclid", N, 1)
    route, lens, value, status, info = check(eng, d, [fl.random_row(k, N - k, 4), all_on(k, N - k, k - 1)], k, 1, shared=True, limit=8, tag="largest")
    assert list(status) == [2, 2] and info[:, :2].tolist() == [[8, 9], [8, 9]] and np.all(value[:, 0] < value[:, 2])


# ---- 2. batches, capacities and the cap on the moves
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_batch_sizes_at_n_12(eng, B, shared):
    k, n, mode = 3, 9, B % 2
    kinds = ("ints", "uniform", "euclid")
    starts = [fl.random_row(k, n, b) for b in range(B)]
    if shared:
        check(eng, fl.matrix("euclid", 12, 7), starts, k, mode, shared=True, tag="batch")
        return
    mats = [fl.matrix(kinds[b % 3], 12, b) for b in range(B)]
    if B >= 3:
        mats[1][2, 9] = fl.INF                                        # one problem of the batch is not searched
    route, lens, value, status, info = check(eng, mats, starts, k, mode, tag="batch")
    assert [s == 1 for s in status] == [b == 1 and B >= 3 for b in range(B)]
    if B >= 3:
        assert np.all(route[1] == -1) and np.all(value[1] == fl.INF) and np.all(lens[1] == fl.INF) and not info[1].any()


@pytest.mark.parametrize("k,n", [(3, 10), (5, 61)])
def test_capacities_that_bind(eng, k, n):
    N = k + n
    d = fl.matrix("euclid", N, 6)
    for mode in fl.MODES:
        caps = ceil_caps(k, n)
        starts = [fl.random_row(k, n, s, caps) for s in range(3)]
        route, lens, value, status, info = check(eng, d, starts, k, mode, shared=True, cap=caps, tag="ceil")
        assert np.all(info[:, 0] > 0)
        held = fl.structure(starts[0], k)[1]                          # caps equal to the start's counts: no task changes hands
        route, lens, value, status, info = check(eng, d, [starts[0]], k, mode, shared=True, cap=held, tag="held")
        assert [sorted(x) for x in fl.split(route[0], k)] == [sorted(x) for x in fl.split(starts[0], k)]
        route = check(eng, d, [all_on(k, n, 1)], k, mode, shared=True, cap=[0, n] + [0] * (k - 2), tag="shut")[0]
        assert fl.structure(route[0], k)[1] == [0, n] + [0] * (k - 2)
        loose = check(eng, d, starts, k, mode, shared=True, cap=[n] * k, tag="loose")
        free = check(eng, d, starts, k, mode, shared=True, tag="free")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(loose, free))


@pytest.mark.parametrize("k,n", [(2, 7), (4, 60)])
def test_a_local_optimum_and_the_cap_on_the_moves(eng, k, n):
    N = k + n
    d = fl.matrix("euclid", N, 5)
    for mode in fl.MODES:
        start = fl.random_row(k, n, 5)
        full = model(d, start, k, mode, None, 16 * N)
        best, moves = full[0], full[4][0]
        assert full[3] == 0 and moves >= 3
        route, lens, value, status, info = check(eng, d, [best, start], k, mode, shared=True, tag="optimum")
        assert info[0].tolist() == [0, 1, 0, 0, 0] and route[0].tolist() == best and [tc.bits(x) for x in value[0, :2]] == [tc.bits(x) for x in value[0, 2:]]
        for limit in (0, 1, moves - 1, moves):
            route, lens, value, status, info = check(eng, d, [start, best], k, mode, shared=True, limit=limit, tag="cap")
            assert list(status) == [0 if limit == moves else 2, 0] and info[0, :2].tolist() == [limit, limit + 1]
            assert limit or route[0].tolist() == start


def test_cap_null_info_null_and_five_identical_runs(eng):
    for k, n in ((2, 9), (3, 128)):
        N = k + n
        limit = 16 * N if N < 65 else 20
        mats = [fl.matrix(kind, N, 13) for kind in ("ints", "uniform", "euclid", "ints")]
        starts = [fl.random_row(k, n, b) for b in range(4)]
        first = run(eng, mats, starts, k, 1, False, None, limit, want_info=False)
        ref = check(eng, mats, starts, k, 1, limit=limit, tag="identical")
        for _ in range(5):
            again = run(eng, mats, starts, k, 1, False, None, limit)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ref))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:4], ref[:4]))


# ---- 3. what the matrices hold
@pytest.mark.parametrize("k,n", [(2, 5), (3, 130)])
def test_matrix_content(eng, k, n):
    N = k + n
    limit = 16 * N if N < 65 else 10
    base = fl.matrix("uniform", N, 11)
    equal = np.full((N, N), 2.75)
    junk = base.copy()
    junk[np.tril_indices(N)] = np.resize([np.nan, -1.0, -fl.INF, 2.0 ** 1010, fl.INF], N * (N + 1) // 2)   # never read
    junk[:k, :k] = np.resize([fl.INF, np.nan, -3.0, 2.0 ** 1010], (k, k))                                 # robot to robot: never read
    hole = base.copy()
    hole[0, N - 1] = fl.INF
    big = np.where(fl.matrix("ints", N, 5) == 1.0, BIG, np.where(fl.matrix("ints", N, 6) == 1.0, 0.0, base))
    mats = [fl.matrix("ints", N, 2), equal, junk, hole, big, base]
    for mode in fl.MODES:
        starts = [fl.random_row(k, n, b) for b in range(5)] + [fl.random_row(k, n, 2)]
        route, lens, value, status, info = check(eng, mats, starts, k, mode, limit=limit, tag="content")
        assert [s == 1 for s in status] == [b == 3 for b in range(6)]
        assert words(route[2], lens[2], value[2], status[2], info[2]) == words(route[5], lens[5], value[5], status[5], info[5])
        assert np.all(route[3] == -1) and np.all(value[3] == fl.INF) and np.all(lens[3] == fl.INF)
        assert np.isfinite(value[4]).all() and value[4, 3] >= BIG


def test_one_robot_is_the_sum_rule(eng):
    from test_gpu_fleet import run as sum_run
    for N in (9, 40):
        d = fl.matrix("euclid", N, 8)
        for mode in fl.MODES:
            start = fl.random_row(1, N - 1, 2)
            route, lens, value, status, info = check(eng, d, [start], 1, mode, shared=True, tag="one")
            sr, sl, sv, ss, si = sum_run(eng, d, [start], 1, mode, True, None, 16 * N)
            assert status[0] == ss[0] == 0 and route.tolist() == sr.tolist() and info[0, :4].tolist() == si[0].tolist()
            assert [tc.bits(x) for x in value[0]] == [tc.bits(x) for x in (sv[0, 0], sv[0, 0], sv[0, 1], sv[0, 1])]


# ---- 4. FleetTours(objective="makespan") end to end
def against_the_model(t, g, cells, fields, search, cap=None):
    ids = [r * g.shape[1] + c for r, c in cells]
    want_m = np.ascontiguousarray(fields[:, ids])
    assert t.matrix.tobytes() == fl.mirror(want_m).tobytes()
    want = fb.search(want_m, t.k, t.mode, cap=cap, max_moves=t.max_moves, **search)
    assert t.feasible == want["feasible"] and list(t.route) == list(want["route"]) and t.routes == want["routes"] and t.moves == want["moves"]
    assert [tc.bits(x) for x in [t.total, t.start_total, t.makespan, t.start_makespan] + t.history + t.total_history + t.lengths] == \
           [tc.bits(x) for x in [want["total"], want["start_total"], want["makespan"], want["start_makespan"]] + want["history"] + want["total_history"] + want["lengths"]]
    if t.feasible:
        assert tc.bits(t.route_cost(t.routes)) == tc.bits(t.total) and tc.bits(t.route_makespan(t.routes)) == tc.bits(t.makespan)
        assert fl.valid_row(t.route, t.k, t.N, cap)
    return want


@pytest.mark.parametrize("name,end,capacity", [("fig7", "open", None), ("fig7", "return", None), ("g256", "return", None), ("g256", "open", [12, 9, 12, 10])])
def test_fleet_tours_makespan_end_to_end(name, end, capacity):
    from pathfit import DistanceField, Engine, FleetTours
    g = gio.grid(name)[0]
    if name == "fig7":
        robots, tasks, search = fl.MAP_ROBOTS, fl.MAP_TASKS, fl.MAP_SEARCH
    else:
        cells = reachable_cells(g, 44, 5)
        robots, tasks, search = cells[:4], cells[4:], dict(starts=5, rounds=2, seed=9)
    e = Engine(g)
    t = s = df = None
    try:
        t = FleetTours(g, robots, tasks, end=end, capacity=capacity, engine=e, objective="makespan", **search)
        df = DistanceField(g, sources=robots + tasks, engine=e)
        against_the_model(t, g, robots + tasks, df.fields.reshape(len(robots + tasks), -1), search, capacity)
        assert t.feasible and t.kernel_ms > 0 and len(t.history) == len(t.total_history) == search["rounds"] + 1 and t.makespan == t.history[-1] <= t.history[0]
        if name == "fig7":
            mode = fl.MODES[end == "return"]
            s = FleetTours(g, robots, tasks, end=end, engine=e, **search)
            assert (s.makespan, s.total) == fb.MAP_SUM[mode] and (t.makespan, t.total) == fb.MAP_BALANCED[mode] and t.routes == fb.MAP_BALANCED_ROUTES[mode]
            assert s.objective == "sum" and s.total_history == s.history and t.start_total == s.start_total and t.start_makespan == s.start_makespan
        legs_against_distance_field(t, df, g, robots + tasks)
    finally:
        for o in (t, s, df):
            if o is not None:
                o.close()
        e.close()


def test_refresh_after_update_grid():
    from pathfit import DistanceField, FleetTours
    g, robots, tasks = two_rooms()
    search = dict(starts=4, rounds=2, seed=1)
    t = FleetTours(g, robots, tasks, end="return", objective="makespan", **search)
    try:
        first = t.makespan
        g2 = g.copy()
        g2[7, 10] = 1
        t.engine.update_grid(g2)
        t.refresh()
        df = DistanceField(g2, sources=robots + tasks, engine=t.engine)
        try:
            against_the_model(t, g2, robots + tasks, df.fields.reshape(6, -1), search)
            legs_against_distance_field(t, df, g2, robots + tasks)
        finally:
            df.close()
        assert t.feasible and t.makespan >= first
    finally:
        t.close()


def test_a_makespan_search_a_sum_search_and_an_assignment_take_turns(eng):
    import assign_checkers as ac
    from pathfit import Assignment, FleetTours
    g = gio.grid("fig7")[0]
    m = FleetTours(g, fl.MAP_ROBOTS, fl.MAP_TASKS, engine=eng, objective="makespan", **fl.MAP_SEARCH)
    f = FleetTours(g, fl.MAP_ROBOTS, fl.MAP_TASKS, engine=eng, **fl.MAP_SEARCH)
    a = Assignment(g, ac.GREEDY_ROBOTS, ac.GREEDY_TASKS, engine=eng)
    try:
        lm, lf, pa = m.paths(), f.paths(), a.paths()
        f.refresh()
        assert [list(x.cells) for x in m.paths()] == [list(x.cells) for x in lm]
        m.refresh()
        a.refresh()
        assert (m.makespan, m.total) == fb.MAP_BALANCED[0] and m.routes == fb.MAP_BALANCED_ROUTES[0] and [list(x.cells) for x in m.paths()] == [list(x.cells) for x in lm]
        assert f.total == fl.MAP_ROUNDS_TOTAL and f.routes == fl.MAP_ROUTES and [list(x.cells) for x in f.paths()] == [list(x.cells) for x in lf]
        assert a.total == ac.GREEDY_OPTIMUM and [list(p.cells) for p in a.paths()] == [list(p.cells) for p in pa]
    finally:
        for o in (m, f, a):
            o.close()


def test_balance_matrices(eng):
    from pathfit import FleetTours
    mats = np.array([fl.matrix(kind, 10, 2) for kind in ("ints", "uniform", "euclid")])
    out = FleetTours.balance_matrices(eng, mats, 3, end="return", capacity=[3, 3, 3])
    assert out.value.shape == (3, 4) and out.info.shape == (3, 5)
    for b in range(3):
        want = model(mats[b], fl.start_row(fl.mirror(mats[b]), 3, [3, 3, 3]), 3, 1, [3, 3, 3], 160)
        assert words(out.route[b], out.lengths[b], out.value[b], out.status[b], out.info[b]) == words(*want)
    starts = [fl.random_row(2, 8, b) for b in range(5)]
    out = FleetTours.balance_matrices(eng, mats[2], 2, starts, shared=True, max_moves=2)
    for b in range(5):
        assert words(out.route[b], out.lengths[b], out.value[b], out.status[b], out.info[b]) == words(*model(mats[2], starts[b], 2, 0, None, 2))


# ---- 5. argument errors of the raw ABI
def test_argument_and_validation_errors_leave_every_output_untouched(eng):
    e, L = eng, eng.L
    k, n, B = 3, 4, 3
    N = k + n
    good = np.array([fl.matrix("uniform", N, b) for b in range(B)])
    rows = np.array([fl.random_row(k, n, b, [2, 2, 2]) for b in range(B)], np.int32)
    held = np.full(B * N + 2 * PAD, CANARY, np.int32)
    held[PAD:PAD + B * N] = rows.reshape(-1)
    ob, lb, vb = e.put(held), between_canaries(e, B * k, np.float64), between_canaries(e, 4 * B, np.float64)
    sb, ib = between_canaries(e, B, np.int32), between_canaries(e, 5 * B, np.int64)
    dm, dc = e.put(good.reshape(-1)), e.put(np.array([2, 2, 2], np.int32))
    route, lens, value, status, info = ob.at(PAD), lb.at(PAD), vb.at(PAD), sb.at(PAD), ib.at(PAD)
    try:
        balance = L.pf_fleet_balance
        out = (route, lens, value, status, info)
        assert balance(None, 0, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == -2
        for args, msg in [((2, k, n, B, 0, dm.ptr, dc.ptr, 9) + out, "mode = 2"), ((-1, k, n, B, 0, dm.ptr, dc.ptr, 9) + out, "mode = -1"),
                          ((0, 0, n, B, 0, dm.ptr, dc.ptr, 9) + out, "k = 0"), ((0, k, 0, B, 0, dm.ptr, dc.ptr, 9) + out, "n = 0"),
                          ((0, k, 1022, B, 0, dm.ptr, dc.ptr, 9) + out, "k + n = 1025"), ((0, 2 ** 31 - 1, 2 ** 31 - 1, B, 0, dm.ptr, dc.ptr, 9) + out, "k + n = 4294967294"),
                          ((0, k, n, 0, 0, dm.ptr, dc.ptr, 9) + out, "B = 0"), ((0, k, n, B, 2, dm.ptr, dc.ptr, 9) + out, "shared = 2"),
                          ((0, k, n, B, -1, dm.ptr, dc.ptr, 9) + out, "shared = -1"), ((0, k, n, B, 0, dm.ptr, dc.ptr, -1) + out, "max_moves = -1"),
                          ((0, k, n, B, 0, dm.ptr, dc.ptr, (1 << 20) + 1) + out, "max_moves = 1048577"),
                          ((0, k, n, B, 0, None, dc.ptr, 9) + out, "must not be null"), ((0, k, n, B, 0, dm.ptr, dc.ptr, 9, None, lens, value, status, info), "must not be null"),
                          ((0, k, n, B, 0, dm.ptr, dc.ptr, 9, route, None, value, status, info), "must not be null"),
                          ((0, k, n, B, 0, dm.ptr, dc.ptr, 9, route, lens, None, status, info), "must not be null"),
                          ((0, k, n, B, 0, dm.ptr, dc.ptr, 9, route, lens, value, None, info), "must not be null")]:
            assert balance(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode() and "pf_fleet_balance" in L.pf_last_error(e.h).decode(), (msg, L.pf_last_error(e.h))
        dc.upload(np.array([2, -1, 5], np.int32))
        assert balance(e.h, 0, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == -1 and "cap[1] = -1" in L.pf_last_error(e.h).decode()
        dc.upload(np.array([2, 2, 2], np.int32))
        # a NaN, a negative entry and an entry beyond 2^1000 among the readable entries: the smallest (b, i, j) is named
        bad = good.copy()
        bad[2, 1, 3], bad[1, 3, 4], bad[0, 4, 0], bad[0, 2, 2], bad[0, 0, 1], bad[0, 1, 2] = -1.0, np.nan, np.nan, -3.0, np.nan, -1.0   # (the last four are never read)
        assert fl.first_bad_entry(bad, k) == (1, 3, 4)
        dm.upload(bad.reshape(-1))
        assert balance(e.h, 1, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == -1 and "(b, i, j) = (1, 3, 4)" in L.pf_last_error(e.h).decode()
        bad[1, 3, 4] = BIG
        dm.upload(bad.reshape(-1))
        assert balance(e.h, 1, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == -1 and "(b, i, j) = (2, 1, 3)" in L.pf_last_error(e.h).decode()
        bad[2, 1, 3], bad[2, 3, 4] = 1.0, 2.0 ** 1001
        dm.upload(bad.reshape(-1))
        assert balance(e.h, 1, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == -1 and "(b, i, j) = (2, 3, 4)" in L.pf_last_error(e.h).decode()
        dm.upload(good.reshape(-1))
        # a bad start row: the smallest (b, position) is named
        r1 = [int(v) for v in rows[1]]
        m1, m2 = r1.index(1), r1.index(2)
        t2 = [p for p in range(N) if rows[2, p] >= k]
        for change, at in [({(2, t2[1]): int(rows[2, t2[0]])}, (2, t2[1])), ({(1, m1): 2, (1, m2): 1, (2, t2[1]): int(rows[2, t2[0]])}, (1, m1)),
                           ({(1, 2): N}, (1, 2)), ({(0, N - 1): -1}, (0, N - 1)), ({(1, 0): r1[1], (1, 1): 0}, (1, 0))]:
            broken = rows.copy()
            for (b, p), v in change.items():
                broken[b, p] = v
            assert fl.first_bad_row(broken, k, N) == at
            held[PAD:PAD + B * N] = broken.reshape(-1)
            ob.upload(held)
            assert balance(e.h, 0, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == -1
            assert f"(b, position) = ({at[0]}, {at[1]})" in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
            assert np.array_equal(ob.download(), held)
        # a robot beyond its capacity: the smallest (b, robot) is named
        held[PAD:PAD + B * N] = rows.reshape(-1)
        ob.upload(held)
        caps = fl.structure(rows[0], k)[1]                           # what row 0 holds: a later row holds more somewhere
        want = fl.first_over_cap(rows, k, N, caps)
        assert want is not None
        dc.upload(np.array(caps, np.int32))
        assert balance(e.h, 0, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == -1
        assert f"(b, robot) = ({want[0]}, {want[1]})" in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
        assert np.array_equal(ob.download(), held)
        for b in (lb, vb, sb, ib):
            assert np.all(b.download() == CANARY)
        # the handle still works
        dc.upload(np.array([2, 2, 2], np.int32))
        assert balance(e.h, 1, k, n, B, 0, dm.ptr, dc.ptr, 9, *out) == 0
        want = model(good[0], rows[0], k, 1, [2, 2, 2], 9)
        assert tc.bits(vb.download()[PAD]) == tc.bits(want[2][0]) and list(ob.download()[PAD:PAD + N]) == want[0]
    finally:
        for b in (ob, lb, vb, sb, ib, dm, dc):
            b.free()
