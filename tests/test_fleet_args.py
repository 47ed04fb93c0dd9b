"""FleetTours argument checks: every ValueError before any device is touched, and the numpy side (the chunks, the mirrored matrix,
the start rule, the perturbation stream, incumbent replacement and its tie rule, history, route_cost, legs, paths, solve_matrices,
refresh) over a model engine whose pf_fleet_improve is the checkers' (runs on a CPU-only host)."""
import numpy as np
import pytest

import cost_checkers as cc
import field_checkers as fc
import fleet_checkers as fl
import golden_io as gio
from test_assign_args import ModelEngine as FieldModelEngine


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import fleet

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(fleet, "Engine", boom)


class ModelEngine(FieldModelEngine):
    """The field calls of the assignment tests' model engine, and pf_fleet_improve as the checkers' literal loop; `improves` logs
    (mode, k, n, B, shared, caps, max_moves, the start rows) per call.  `script`: totals to answer with instead, one list per call."""

    def __init__(self, g, script=None):
        super().__init__(g)
        self.improves = []
        self.script = script

    def fleet_improve(self, mode, k, n, B, shared, d_mat, d_cap, max_moves, d_route, d_len, d_value, d_status, d_info=None):
        self.calls.append("fleet_improve")
        N = k + n
        mats = d_mat.a.reshape(-1, N, N)
        cap = None if d_cap is None else [int(c) for c in d_cap.a]
        assert len(mats) == (1 if shared else B) and (cap is None or len(cap) == k)
        assert fl.first_bad_row(d_route.a, k, N) is None and fl.first_over_cap(d_route.a, k, N, cap) is None
        rows = d_route.a.reshape(B, N).copy()
        self.improves.append((mode, k, n, B, bool(shared), cap, max_moves, rows))
        for b in range(B):
            o, lens, v, st, info = fl.improve(mats[0 if shared else b], rows[b], k, mode, cap, max_moves)
            if self.script is not None and st != 1:
                o, v = list(rows[b]), (self.script[len(self.improves) - 1][b], v[1], v[2])
            d_route.a[b * N:(b + 1) * N] = o
            d_len.a[b * k:(b + 1) * k] = lens
            d_value.a[3 * b:3 * b + 3] = v
            d_status.a[b] = st
            if d_info is not None:
                d_info.a[4 * b:4 * b + 4] = info


def fig7():
    return gio.grid("fig7")[0]


def make(g, robots, tasks, **kw):
    from pathfit import FleetTours
    return FleetTours(g, robots, tasks, **kw)


def gathered(g, cells, ad=True, rs=True):
    mm = fc.move_masks(np.asarray(g, np.uint8), ad, rs)
    ids = [r * g.shape[1] + c for r, c in cells]
    fields = np.array([fc.reference_dijkstra(np.asarray(g, np.uint8), mm, s)[0] for s in ids]).reshape(len(ids), -1)
    return np.ascontiguousarray(fields[:, ids])


R3, T12 = fl.MAP_ROBOTS, fl.MAP_TASKS


# ---- every ValueError, before the device
def test_grid_and_engine(no_engine):
    with pytest.raises(ValueError, match="^FleetTours: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)], [(0, 1)])

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^FleetTours: the engine's grid has another shape"):
        make(fig7(), [(0, 0)], [(0, 1)], engine=Other())
    with pytest.raises(AssertionError, match="the device was touched"):
        make(fig7(), R3, T12)


def test_robots_and_tasks(no_engine):
    g = np.zeros((40, 40), int)
    with pytest.raises(ValueError, match="^FleetTours: robots is empty"):
        make(g, [], [(0, 0)])
    with pytest.raises(ValueError, match="^FleetTours: tasks is empty"):
        make(g, [(0, 0)], [])
    with pytest.raises(ValueError, match="^FleetTours: robots must be a list"):
        make(g, 5, [(0, 0)])
    with pytest.raises(ValueError, match="^FleetTours: tasks must be a list"):
        make(g, [(0, 0)], 5)
    with pytest.raises(ValueError, match=r"^FleetTours: tasks\[1\] = \(40, 0\) is outside the 40x40 grid"):
        make(g, [(0, 0)], [(0, 0), (40, 0)])
    with pytest.raises(ValueError, match=r"^FleetTours: robots\[0\] = \(0, -1\) is outside the 40x40 grid"):
        make(g, [(0, -1)], [(0, 0)])
    with pytest.raises(ValueError, match=r"^FleetTours: robots\[0\] must be an \(r, c\) pair"):
        make(g, [7], [(0, 0)])
    cells = [(r, c) for r in range(26) for c in range(40)]
    with pytest.raises(ValueError, match="^FleetTours: 3 robots and 1022 tasks; at most 1024 cells together"):
        make(g, cells[:3], cells[3:1025])
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, cells[:3], cells[3:1024])


def test_end(no_engine):
    for end in ("last", "closed", 0, None):
        with pytest.raises(ValueError, match="^FleetTours: end must be 'open' or 'return'"):
            make(fig7(), R3, T12, end=end)


def test_capacity(no_engine):
    g = fig7()
    for bad in ([4, 4], [4, 4, 4, 4], "444", 4.0, [[4, 4, 4]]):
        with pytest.raises(ValueError, match="^FleetTours: capacity"):
            make(g, R3, T12, capacity=bad)
    for bad in ([4, 4, -1], [4, 4.0, 4], [True, 12, 12], [4, None, 4]):
        with pytest.raises(ValueError, match=r"^FleetTours: capacity\[\d\] must be an integer"):
            make(g, R3, T12, capacity=bad)
    with pytest.raises(ValueError, match="^FleetTours: capacity must be None, an integer or a list of 3"):
        make(g, R3, T12, capacity=True)
    with pytest.raises(ValueError, match="^FleetTours: the capacities hold 11 tasks, fewer than the 12 given"):
        make(g, R3, T12, capacity=[4, 4, 3])
    with pytest.raises(ValueError, match="^FleetTours: the capacities hold 9 tasks"):
        make(g, R3, T12, capacity=3)
    for good in (4, [12, 0, 0], np.array([4, 4, 4]), np.int64(5)):
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, R3, T12, capacity=good)


def test_cost_map(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^FleetTours: cost has shape"):
        make(g, R3, T12, cost=np.ones((20, 19)))
    c = np.ones((20, 20))
    c[tuple(np.argwhere(g != 1)[3])] = 0.5
    with pytest.raises(ValueError, match="^FleetTours: cost"):
        make(g, R3, T12, cost=c)


def test_starts_rounds_seed_and_max_moves(no_engine):
    g = fig7()
    for name, bad in (("starts", (0, -1, 1.5, "8", True, None, (1 << 16) + 1)), ("rounds", (-1, 2.0, None, True)), ("seed", (-1, 0.5, None, "x")),
                      ("max_moves", (-1, (1 << 20) + 1, 3.0, True))):
        for v in bad:
            with pytest.raises(ValueError, match=f"^FleetTours: {name} must be an integer in "):
                make(g, R3, T12, **{name: v})
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, R3, T12, starts=1, rounds=0, seed=np.int64(5), max_moves=0)


def test_solve_matrices_errors():
    from pathfit import FleetTours
    e = ModelEngine(fig7())
    sm = FleetTours.solve_matrices
    with pytest.raises(ValueError, match="^FleetTours: mats has shape"):
        sm(e, np.zeros((2, 3, 4)), 1)
    with pytest.raises(ValueError, match="^FleetTours: 2 robots and 1023 tasks; at most 1024"):
        sm(e, np.zeros((1, 1025, 1025)), 2)
    with pytest.raises(ValueError, match="^FleetTours: tasks is empty"):
        sm(e, np.zeros((1, 3, 3)), 3)
    with pytest.raises(ValueError, match="^FleetTours: k must be an integer in"):
        sm(e, np.zeros((1, 3, 3)), 0)
    with pytest.raises(ValueError, match="^FleetTours: end must be"):
        sm(e, np.zeros((1, 3, 3)), 1, end="last")
    with pytest.raises(ValueError, match="^FleetTours: shared=True takes one"):
        sm(e, np.zeros((2, 3, 3)), 1, shared=True)
    with pytest.raises(ValueError, match="^FleetTours: max_moves must be an integer"):
        sm(e, np.zeros((2, 3, 3)), 1, max_moves=-1)
    with pytest.raises(ValueError, match="^FleetTours: the capacities hold 1 tasks"):
        sm(e, np.zeros((2, 3, 3)), 1, capacity=1)
    m = np.array([fl.matrix("uniform", 5, b) for b in range(3)])
    for x, shown in ((np.nan, "nan"), (-1.0, "-1.0"), (2.0 ** 1001, "2.14")):
        bad = m.copy()
        bad[2, 1, 3], bad[0, 3, 1], bad[1, 2, 2], bad[0, 0, 1] = x, np.nan, -2.0, np.nan   # (the lower triangle, the diagonal, robot-robot: never read)
        with pytest.raises(ValueError, match=rf"^FleetTours: mats\[2, 1, 3\] = {shown}.* is neither"):
            sm(e, bad, 2)
    for routes, at in (([[0, 2, 1, 3, 4], [0, 2, 2, 1, 4], [0, 1, 2, 3, 4]], r"\[1, 2\] = 2"), ([[0, 1, 2, 3, 4]] * 2 + [[1, 0, 2, 3, 4]], r"\[2, 0\] = 1"),
                       ([[0, 1, 2, 3, 5]] * 3, r"\[0, 4\] = 5"), ([[2, 0, 1, 3, 4]] * 3, r"\[0, 0\] = 2")):
        with pytest.raises(ValueError, match=rf"^FleetTours: routes{at}: a start is a permutation"):
            sm(e, m, 2, routes)
    with pytest.raises(ValueError, match=r"^FleetTours: routes\[0, 1\] = 2: a start is a permutation"):
        sm(e, m, 3, [[0, 2, 1, 3, 4]] * 3)                            # robot 2 in front of robot 1
    with pytest.raises(ValueError, match=r"^FleetTours: routes\[1\] gives robot 0 3 tasks, more than its capacity 2"):
        sm(e, m, 2, [[0, 2, 1, 3, 4], [0, 2, 3, 4, 1], [0, 1, 2, 3, 4]], capacity=[2, 3])
    for routes in ([[0, 1, 2, 3, 4]] * 2, [[0, 1, 2]] * 3, [[0.0, 1.0, 2.0, 3.0, 4.0]] * 3, "abc"):
        with pytest.raises(ValueError, match="^FleetTours: routes must be an integer array"):
            sm(e, m, 2, routes)
    assert e.calls == []


# ---- the numpy side over the model engine
def test_the_facade_over_the_model():
    g = fig7()
    e = ModelEngine(g)
    t = make(g, R3, T12, engine=e, **fl.MAP_SEARCH)
    k, n, N, want_m = 3, 12, 15, gathered(g, R3 + T12)
    assert e.calls == ["dist_field_batch", "assign_matrix"] + ["fleet_improve"] * 4
    assert t.matrix.tobytes() == fl.mirror(want_m).tobytes()
    # the calls: the start row alone, then the rounds' perturbations of the incumbent, all over the one shared matrix
    assert [c[:7] for c in e.improves] == [(0, k, n, 1, True, None, 16 * N)] + [(0, k, n, 8, True, None, 16 * N)] * 3
    assert e.improves[0][7].tolist() == [fl.start_row(t.matrix, k, None)]
    rng, best = np.random.default_rng(0), fl.MAP_ROUND0_TOTAL
    o = fl.improve(want_m, e.improves[0][7][0], k, 0, None, 16 * N)[0]
    for call in e.improves[1:]:
        assert call[7].tolist() == fl.perturbations(rng, o, k, None, 8)
        for row in call[7]:
            got = fl.improve(want_m, row, k, 0, None, 16 * N)
            if got[2][0] < best:
                best, o = got[2][0], got[0]
    want = fl.search(want_m, k, 0, solver=fl.improve, **fl.MAP_SEARCH)
    assert t.feasible and list(t.route) == want["route"] == o and t.routes == want["routes"] == fl.MAP_ROUTES and t.moves == want["moves"]
    assert t.history == want["history"] and t.lengths == want["lengths"] and t.makespan == want["makespan"] == max(t.lengths)
    assert (t.start_total, t.history[0], t.total) == (fl.MAP_START_TOTAL, fl.MAP_ROUND0_TOTAL, fl.MAP_ROUNDS_TOTAL) and t.total == best
    assert t.route_cost(t.routes) == t.total
    assert t.route_cost([[v - k for v in tasks] for tasks in fl.split(fl.start_row(t.matrix, k, None), k)]) == t.start_total
    assert t.route_cost([[], [], []]) == 0.0 and t.route_cost([[0], [], [1]]) == t.matrix[0, 3] + t.matrix[2, 4]
    with pytest.raises(ValueError, match=r"^FleetTours: routes\[1\]\[0\] = 12 is outside \[0, 12\)"):
        t.route_cost([[0], [12], []])
    with pytest.raises(ValueError, match=r"^FleetTours: routes\[2\]\[1\] = 0 is visited twice"):
        t.route_cost([[0], [], [1, 0]])
    for bad in (3, [[0], [1]], [0, 1, 2]):
        with pytest.raises(ValueError, match="^FleetTours: routes must be 3 sequences"):
            t.route_cost(bad)
    legs = t.legs()
    assert e.calls[6:] == ["dist_field_parents", "dist_field_paths"] and [len(x) for x in legs] == [len(r) for r in t.routes]
    for r, (route, mine) in enumerate(zip(t.routes, legs)):
        cells = [R3[r]] + [T12[v] for v in route]
        for leg, a, b in zip(mine, cells[:-1], cells[1:]):
            assert leg[0] == a and leg[-1] == b
    paths = t.paths()
    assert [len(p) for p in paths] == [sum(len(x) for x in mine) - (len(mine) - 1) for mine in legs]
    assert e.calls[8:] == ["dist_field_paths"]                        # the parent maps are kept
    t.close()


@pytest.mark.parametrize("end", ["open", "return"])
def test_both_ends_the_caps_and_the_seed(end):
    g = fig7()
    robots, tasks = R3[:2], T12[:7]
    mode = fl.MODES[end == "return"]
    want_m = gathered(g, robots + tasks)
    runs = []
    for seed in (0, 0, 7):
        e = ModelEngine(g)
        t = make(g, robots, tasks, end=end, capacity=[5, 4], starts=5, rounds=3, seed=seed, max_moves=40, engine=e)
        want = fl.search(want_m, 2, mode, cap=[5, 4], starts=5, rounds=3, seed=seed, max_moves=40)
        assert (list(t.route), t.routes, t.lengths, t.total, t.makespan, t.start_total, t.history, t.moves) == \
               (want["route"], want["routes"], want["lengths"], want["total"], want["makespan"], want["start_total"], want["history"], want["moves"])
        assert fl.valid_row(t.route, 2, 9, [5, 4]) and t.route_cost(t.routes) == t.total
        assert all(c[5] == [5, 4] and c[6] == 40 for c in e.improves)
        assert [len(x) for x in t.legs()] == [len(r) + (mode == 1 and len(r) > 0) for r in t.routes]
        runs.append(e.improves)
    assert all(np.array_equal(a[7], b[7]) for a, b in zip(runs[0], runs[1])) and not all(np.array_equal(a[7], b[7]) for a, b in zip(runs[0], runs[2]))


def test_the_incumbent_is_replaced_by_a_strictly_smaller_total_at_the_smallest_index():
    g = fig7()
    script = [[50.0], [50.0, 60.0, 50.0], [49.0, 48.0, 48.0], [48.0, 47.5, 40.0], [40.0, 40.0, 40.0]]
    e = ModelEngine(g, script)
    t = make(g, R3, T12[:6], starts=3, rounds=4, engine=e)
    assert t.history == [50.0, 50.0, 48.0, 40.0, 40.0] and t.total == 40.0
    rows = [c[7] for c in e.improves]                                 # (the scripted answers keep the start rows)
    rng = np.random.default_rng(0)
    incumbents = [rows[0][0], rows[0][0], rows[2][1], rows[3][2]]     # equal totals replace nothing; of two equal ones the first wins
    for call, inc in zip(rows[1:], incumbents):
        assert call.tolist() == fl.perturbations(rng, inc, 3, None, 3)
    assert list(t.route) == list(rows[3][2])


def test_the_smallest_fleets_and_an_empty_route():
    g = fig7()
    one = make(g, R3[:1], T12[:1], end="return", rounds=1, starts=2, engine=ModelEngine(g))
    assert one.routes == [[0]] and one.total == 2 * one.matrix[0, 1] and len(one.legs()[0]) == 2 and one.history == [one.total] * 2
    far = make(g, [T12[0], R3[2]], [T12[1]], engine=ModelEngine(g))   # one task: one robot keeps an empty route
    assert sorted(far.routes) == [[], [0]] and far.max_moves == 48 and min(far.lengths) == 0.0 and far.makespan == far.total
    legs, paths = far.legs(), far.paths()
    idle = far.routes.index([])
    assert legs[idle] == [] and len(paths[idle]) == 1 and paths[idle][0] == (far.robots[idle]) and len(paths[1 - idle]) == len(legs[1 - idle][0])


def test_the_chunks():
    from pathfit import FleetTours
    g = fig7()
    robots, tasks = R3[:2], T12[:5]
    whole = make(g, robots, tasks, end="return", starts=3, rounds=1, engine=ModelEngine(g))

    class Small(FleetTours):
        CHUNK_BYTES = 3 * 400 * 8
    e = ModelEngine(g)
    t = Small(g, robots, tasks, end="return", starts=3, rounds=1, engine=e)
    assert t.chunk == 3 and whole.chunk == 7 and e.rows_asked == [3, 3, 1]
    assert e.calls == ["dist_field_batch", "assign_matrix"] * 3 + ["fleet_improve"] * 2
    assert t.matrix.tobytes() == whole.matrix.tobytes() and list(t.route) == list(whole.route) and t.history == whole.history
    want = [[list(p.cells) for p in mine] for mine in whole.legs()]
    assert sum(len(x) for x in want) == 5 + sum(len(r) > 0 for r in whole.routes) and [[list(p.cells) for p in mine] for mine in t.legs()] == want
    assert e.calls[8:].count("dist_field_batch") == 2                 # the last chunk was held; the two released ones are computed again
    assert [[list(p.cells) for p in mine] for mine in t.legs()] == want
    assert [list(p.cells) for p in t.paths()] == [list(p.cells) for p in whole.paths()]


def test_an_unreachable_task():
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    e = ModelEngine(g)
    t = make(g, [(4, 2)], [(0, 18), (8, 3)], engine=e)
    assert not t.feasible and t.total == fl.INF and t.makespan == fl.INF and t.history == [fl.INF] and list(t.route) == [-1] * 3 and t.moves == 0
    assert t.routes == [[]] and t.lengths == [fl.INF] and t.legs() == [] and t.paths() == [] and e.calls.count("fleet_improve") == 1
    two = make(g, [(4, 2), (0, 18)], [(8, 3), (8, 18)], engine=ModelEngine(g))     # the robots cannot reach each other: never read; the tasks can
    assert not two.feasible                                           # (task 0 is out of robot 1's reach: a readable entry)


def test_a_cost_map_goes_through_pf_cost_field_and_refresh_recomputes():
    g = fig7()
    e = ModelEngine(g)
    cost = cc.cost_of_kind("u50", g.shape, 3)
    robots, tasks = R3[:2], T12[:4]
    ids = [r * 20 + c for r, c in robots + tasks]
    t = make(g, robots, tasks, cost=cost, starts=2, rounds=1, engine=e)
    assert e.calls == ["cost_field", "assign_matrix", "fleet_improve", "fleet_improve"]
    want = cc.fields(g, cost, [[s] for s in ids], True, True)[0].reshape(6, -1)[:, ids]
    assert t.matrix.tobytes() == fl.mirror(want).tobytes() and list(t.route) == fl.search(want, 2, 0, starts=2, rounds=1)["route"]
    g2 = g.copy()
    g2[g2 > 1] = 0
    for r, c in [tuple(c) for c in np.argwhere(g2 == 0) if tuple(c) not in robots + tasks][:5]:
        g2[r, c] = 1
    e.update_grid(g2)
    t.refresh()
    want2 = cc.fields(g2, cost, [[s] for s in ids], True, True)[0].reshape(6, -1)[:, ids]
    assert t.matrix.tobytes() == fl.mirror(want2).tobytes() and t.total == fl.search(want2, 2, 0, starts=2, rounds=1)["total"]
    with pytest.raises(ValueError, match="^FleetTours: refresh\\(cost\\) needs fleet tours built with a cost map"):
        make(g, robots, tasks, engine=ModelEngine(g)).refresh(cost=cost)


def test_solve_matrices_over_the_model():
    from pathfit import FleetTours
    e = ModelEngine(fig7())
    mats = np.array([fl.matrix(kind, 9, 1) for kind in ("ints", "uniform", "euclid", "tenths")])
    mats[1][0, 5] = fl.INF
    out = FleetTours.solve_matrices(e, mats, 3, end="return", capacity=[3, 2, 4])
    assert e.improves[-1][:7] == (1, 3, 6, 4, False, [3, 2, 4], 144)
    assert out.route.shape == (4, 9) and out.lengths.shape == (4, 3) and out.value.shape == (4, 3) and out.info.shape == (4, 4)
    for b in range(4):
        assert e.improves[-1][7][b].tolist() == fl.start_row(fl.mirror(mats[b]), 3, [3, 2, 4])
        o, lens, v, st, info = fl.improve_numpy(mats[b], e.improves[-1][7][b], 3, 1, [3, 2, 4], 144)
        assert (list(out.route[b]), list(out.lengths[b]), tuple(out.value[b]), out.status[b], tuple(out.info[b])) == (o, lens, v, st, info)
    assert out.status.tolist() == [0, 1, 0, 0]
    starts = [[0, 3, 1, 2, 4, 5, 6, 7, 8], [0, 1, 2, 3, 4, 5, 6, 7, 8]]
    FleetTours.solve_matrices(e, mats[2], 3, starts, shared=True, max_moves=1)
    assert e.improves[-1][:7] == (0, 3, 6, 2, True, None, 1) and e.improves[-1][7].tolist() == starts
    one = FleetTours.solve_matrices(e, mats[0], 1)
    assert one.route.shape == (1, 9) and e.improves[-1][:7] == (0, 1, 8, 1, False, None, 144)
