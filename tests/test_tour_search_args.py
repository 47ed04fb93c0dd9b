"""TourSearch argument checks: every ValueError before any device is touched, and the numpy side (the chunks, the mirrored matrix,
the nearest-neighbour start, the perturbation stream, incumbent replacement and its tie rule, history, route_cost, legs,
solve_matrices, refresh) over a model engine whose pf_tour_improve is the checkers' (runs on a CPU-only host)."""
import numpy as np
import pytest

import cost_checkers as cc
import field_checkers as fc
import golden_io as gio
import tour_checkers as tc
import tour_search_checkers as ts
from test_assign_args import ModelEngine as FieldModelEngine


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import tour_search

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(tour_search, "Engine", boom)


class ModelEngine(FieldModelEngine):
    """The field calls of the assignment tests' model engine, and pf_tour_improve as the checkers' literal loop; `improves` logs
    (mode, n, B, shared, max_moves, the start rows) per call.  `script`: totals to answer with instead, one list per call."""

    def __init__(self, g, script=None):
        super().__init__(g)
        self.improves = []
        self.script = script

    def tour_improve(self, mode, n, B, shared, d_mat, max_moves, d_order, d_value, d_status, d_info=None):
        self.calls.append("tour_improve")
        mats = d_mat.a.reshape(-1, n, n)
        assert len(mats) == (1 if shared else B)
        assert ts.first_bad_start(d_order.a, n, mode) is None
        rows = d_order.a.reshape(B, n).copy()
        self.improves.append((mode, n, B, bool(shared), max_moves, rows))
        for b in range(B):
            o, v, st, info = ts.two_opt(mats[0 if shared else b], rows[b], mode, max_moves)
            if self.script is not None and st != 1:
                o, v = list(rows[b]), (self.script[len(self.improves) - 1][b], v[1])
            d_order.a[b * n:(b + 1) * n] = o
            d_value.a[2 * b:2 * b + 2] = v
            d_status.a[b] = st
            if d_info is not None:
                d_info.a[4 * b:4 * b + 4] = info


def fig7():
    return gio.grid("fig7")[0]


def make(g, stops, **kw):
    from pathfit import TourSearch
    return TourSearch(g, stops, **kw)


def gathered(g, stops, ad=True, rs=True):
    mm = fc.move_masks(np.asarray(g, np.uint8), ad, rs)
    ids = [r * g.shape[1] + c for r, c in stops]
    fields = np.array([fc.reference_dijkstra(np.asarray(g, np.uint8), mm, s)[0] for s in ids]).reshape(len(ids), -1)
    return np.ascontiguousarray(fields[:, ids])


# ---- every ValueError, before the device
def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^TourSearch: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)])


def test_engine_of_another_shape(no_engine):
    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^TourSearch: the engine's grid has another shape"):
        make(fig7(), [(0, 0)], engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    with pytest.raises(AssertionError, match="the device was touched"):
        make(fig7(), ts.MAP_STOPS)


def test_stops(no_engine):
    g = np.zeros((40, 40), int)
    with pytest.raises(ValueError, match="^TourSearch: stops is empty"):
        make(g, [])
    with pytest.raises(ValueError, match="^TourSearch: stops must be a list"):
        make(g, 5)
    with pytest.raises(ValueError, match=r"^TourSearch: stops\[1\] = \(40, 0\) is outside the 40x40 grid"):
        make(g, [(0, 0), (40, 0)])
    with pytest.raises(ValueError, match=r"^TourSearch: stops\[0\] must be an \(r, c\) pair"):
        make(g, [7])
    with pytest.raises(ValueError, match="^TourSearch: end='last' needs at least two stops"):
        make(g, [(0, 0)], end="last")
    cells = [(r, c) for r in range(26) for c in range(40)]
    for end in ("open", "return", "last"):
        with pytest.raises(ValueError, match="^TourSearch: 1025 stops; at most 1024"):
            make(g, cells[:1025], end=end)
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, cells[:1024], end=end)


def test_end_and_no_precedence(no_engine):
    for end in ("closed", 0, None):
        with pytest.raises(ValueError, match="^TourSearch: end must be 'open', 'return' or 'last'"):
            make(fig7(), [(0, 0)], end=end)
    with pytest.raises(TypeError):
        make(fig7(), [(0, 0), (0, 1)], before=[(0, 1)])


def test_cost_map(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^TourSearch: cost has shape"):
        make(g, [(0, 0)], cost=np.ones((20, 19)))
    c = np.ones((20, 20))
    c[tuple(np.argwhere(g != 1)[3])] = 0.5
    with pytest.raises(ValueError, match="^TourSearch: cost"):
        make(g, [(0, 0)], cost=c)


def test_starts_rounds_seed_and_max_moves(no_engine):
    g = fig7()
    for name, bad in (("starts", (0, -1, 1.5, "8", True, None, (1 << 16) + 1)), ("rounds", (-1, 2.0, None, True)), ("seed", (-1, 0.5, None, "x")),
                      ("max_moves", (-1, (1 << 20) + 1, 3.0, True))):
        for v in bad:
            with pytest.raises(ValueError, match=f"^TourSearch: {name} must be an integer in "):
                make(g, ts.MAP_STOPS, **{name: v})
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, ts.MAP_STOPS, starts=1, rounds=0, seed=np.int64(5), max_moves=0)


def test_solve_matrices_errors():
    from pathfit import TourSearch
    e = ModelEngine(fig7())
    with pytest.raises(ValueError, match="^TourSearch: mats has shape"):
        TourSearch.solve_matrices(e, np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="^TourSearch: mats has shape"):
        TourSearch.solve_matrices(e, np.zeros((2, 3, 3, 3)))
    with pytest.raises(ValueError, match="^TourSearch: 1025 stops; at most 1024"):
        TourSearch.solve_matrices(e, np.zeros((1, 1025, 1025)))
    with pytest.raises(ValueError, match="^TourSearch: end must be"):
        TourSearch.solve_matrices(e, np.zeros((1, 3, 3)), end="x")
    with pytest.raises(ValueError, match="^TourSearch: shared=True takes one"):
        TourSearch.solve_matrices(e, np.zeros((2, 3, 3)), shared=True)
    with pytest.raises(ValueError, match="^TourSearch: max_moves must be an integer"):
        TourSearch.solve_matrices(e, np.zeros((2, 3, 3)), max_moves=-1)
    m = np.array([ts.matrix("uniform", 4, b) for b in range(3)])
    for x, shown in ((np.nan, "nan"), (-1.0, "-1.0"), (2.0 ** 1001, "2.14")):
        bad = m.copy()
        bad[2, 1, 3], bad[0, 3, 1], bad[1, 2, 2] = x, np.nan, -2.0    # (the lower triangle and the diagonal are never read)
        with pytest.raises(ValueError, match=rf"^TourSearch: mats\[2, 1, 3\] = {shown}.* is neither"):
            TourSearch.solve_matrices(e, bad)
    for orders, at in (([[0, 1, 2, 3], [0, 1, 1, 3], [0, 1, 2, 3]], r"\[1, 2\] = 1"), ([[0, 1, 2, 3], [0, 1, 2, 3], [1, 0, 2, 3]], r"\[2, 0\] = 1"),
                       ([[0, 1, 2, 4]] * 3, r"\[0, 3\] = 4"), ([[0, 3, 2, 1]] * 3, r"\[0, 3\] = 1")):
        with pytest.raises(ValueError, match=rf"^TourSearch: orders{at}: a start is a permutation"):
            TourSearch.solve_matrices(e, m, orders, end="last" if at.endswith("3\\] = 1") else "open")
    for orders in ([[0, 1, 2, 3]] * 2, [[0, 1, 2]] * 3, [[0.0, 1.0, 2.0, 3.0]] * 3, "abc"):
        with pytest.raises(ValueError, match="^TourSearch: orders must be an integer array"):
            TourSearch.solve_matrices(e, m, orders)
    assert e.calls == []


# ---- the numpy side over the model engine
def test_the_facade_over_the_model():
    g = fig7()
    e = ModelEngine(g)
    t = make(g, ts.MAP_STOPS, engine=e, **ts.MAP_SEARCH)
    n, want_m = 24, gathered(g, ts.MAP_STOPS)
    assert e.calls == ["dist_field_batch", "assign_matrix"] + ["tour_improve"] * 4
    assert t.matrix.tobytes() == ts.mirror(want_m).tobytes() and (want_m != want_m.T).any()
    # the calls: the nearest-neighbour order alone, then the rounds' perturbations of the incumbent, all over the one shared matrix
    assert [c[:5] for c in e.improves] == [(0, n, 1, True, 16 * n)] + [(0, n, 8, True, 16 * n)] * 3
    assert e.improves[0][5].tolist() == [tc.nearest_neighbour(t.matrix, 0)]
    rng, o, best = np.random.default_rng(0), ts.two_opt(want_m, e.improves[0][5][0], 0, 16 * n)[0], ts.MAP_TWO_OPT_TOTAL
    for call in e.improves[1:]:
        assert call[5].tolist() == ts.perturbations(rng, o, n - 1, 8)
        for row in call[5]:
            o2, v2, _, _ = ts.two_opt(want_m, row, 0, 16 * n)
            if v2[0] < best:
                best, o = v2[0], o2
    want = ts.search(want_m, 0, improve=ts.two_opt, **ts.MAP_SEARCH)
    assert t.feasible and list(t.order) == want["order"] == o and t.moves == want["moves"] and t.history == want["history"]
    assert (t.start_total, t.history[0], t.total) == (ts.MAP_NN_TOTAL, ts.MAP_TWO_OPT_TOTAL, ts.MAP_ROUNDS_TOTAL) and t.total == best
    assert t.route_cost(t.order) == t.total and t.route_cost(tc.nearest_neighbour(t.matrix, 0)) == t.start_total
    with pytest.raises(ValueError, match=r"^TourSearch: order\[1\] = 24 is outside \[0, 24\)"):
        t.route_cost([0, 24])
    with pytest.raises(ValueError, match="^TourSearch: order must be a sequence"):
        t.route_cost(3)
    legs = t.legs()
    assert e.calls[6:] == ["dist_field_parents", "dist_field_paths"] and len(legs) == n - 1
    for leg, a, b in zip(legs, t.order[:-1], t.order[1:]):
        assert leg[0] == ts.MAP_STOPS[a] and leg[-1] == ts.MAP_STOPS[b]
    p = t.path()
    assert len(p) == sum(len(x) for x in legs) - (n - 2) and e.calls[8:] == ["dist_field_paths"]      # the parent maps are kept
    t.close()


@pytest.mark.parametrize("end", ["open", "return", "last"])
def test_the_three_ends_and_the_seed(end):
    g = fig7()
    stops = ts.MAP_STOPS[:11]
    mode = {"open": 0, "return": 1, "last": 2}[end]
    want_m = gathered(g, stops)
    runs = []
    for seed in (0, 0, 7):
        t = make(g, stops, end=end, starts=5, rounds=3, seed=seed, max_moves=40, engine=ModelEngine(g))
        want = ts.search(want_m, mode, starts=5, rounds=3, seed=seed, max_moves=40)
        assert (list(t.order), t.total, t.start_total, t.history, t.moves) == (want["order"], want["total"], want["start_total"], want["history"], want["moves"])
        assert tc.admissible(t.order, 11, mode, None) and t.route_cost(t.order) == t.total and len(t.legs()) == (11 if mode == 1 else 10)
        runs.append(t.engine.improves)
    assert all(np.array_equal(a[5], b[5]) for a, b in zip(runs[0], runs[1])) and not all(np.array_equal(a[5], b[5]) for a, b in zip(runs[0], runs[2]))


def test_the_incumbent_is_replaced_by_a_strictly_smaller_total_at_the_smallest_index():
    g = fig7()
    stops = ts.MAP_STOPS[:8]
    script = [[50.0], [50.0, 60.0, 50.0], [49.0, 48.0, 48.0], [48.0, 47.5, 40.0], [40.0, 40.0, 40.0]]
    e = ModelEngine(g, script)
    t = make(g, stops, starts=3, rounds=4, engine=e)
    assert t.history == [50.0, 50.0, 48.0, 40.0, 40.0] and t.total == 40.0
    rows = [c[5] for c in e.improves]                                 # (the scripted answers keep the start rows)
    rng = np.random.default_rng(0)
    incumbents = [rows[0][0], rows[0][0], rows[2][1], rows[3][2]]     # equal totals replace nothing; of two equal ones the first wins
    for call, inc in zip(rows[1:], incumbents):
        assert call.tolist() == ts.perturbations(rng, inc, 7, 3)
    assert list(t.order) == list(rows[3][2])


def test_few_stops_run_no_rounds():
    g = fig7()
    for k, end, calls in ((1, "open", 1), (2, "last", 1), (3, "open", 1), (4, "last", 1), (4, "open", 3), (5, "last", 3)):
        e = ModelEngine(g)
        t = make(g, ts.MAP_STOPS[:k], end=end, starts=2, rounds=2, engine=e)
        assert e.calls.count("tour_improve") == calls and len(t.history) == calls and t.feasible
        assert len(t.legs()) == k - 1 and t.max_moves == 16 * k
    one = make(g, ts.MAP_STOPS[:1], end="return", engine=ModelEngine(g))
    assert one.total == 0.0 and list(one.order) == [0] and one.legs() == [] and len(one.path()) == 0


def test_the_chunks():
    from pathfit import TourSearch
    g = fig7()
    stops = ts.MAP_STOPS[:7]
    whole = make(g, stops, end="return", starts=3, rounds=1, engine=ModelEngine(g))

    class Small(TourSearch):
        CHUNK_BYTES = 3 * 400 * 8
    e = ModelEngine(g)
    t = Small(g, stops, end="return", starts=3, rounds=1, engine=e)
    assert t.chunk == 3 and whole.chunk == 7 and e.rows_asked == [3, 3, 1]
    assert e.calls == ["dist_field_batch", "assign_matrix"] * 3 + ["tour_improve"] * 2
    assert t.matrix.tobytes() == whole.matrix.tobytes() and list(t.order) == list(whole.order) and t.history == whole.history
    want = [list(p.cells) for p in whole.legs()]
    assert len(want) == 7 and [list(p.cells) for p in t.legs()] == want
    assert e.calls[8:].count("dist_field_batch") == 2                 # the last chunk was held; the two released ones are computed again
    assert [list(p.cells) for p in t.legs()] == want


def test_an_unreachable_stop():
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    e = ModelEngine(g)
    t = make(g, [(4, 2), (0, 18), (8, 3)], engine=e)
    assert not t.feasible and t.total == ts.INF and t.history == [ts.INF] and list(t.order) == [-1] * 3 and t.moves == 0
    assert t.legs() == [] and len(t.path()) == 0 and e.calls.count("tour_improve") == 1


def test_a_cost_map_goes_through_pf_cost_field_and_refresh_recomputes():
    g = fig7()
    e = ModelEngine(g)
    cost = cc.cost_of_kind("u50", g.shape, 3)
    stops = ts.MAP_STOPS[:6]
    ids = [r * 20 + c for r, c in stops]
    t = make(g, stops, cost=cost, starts=2, rounds=1, engine=e)
    assert e.calls == ["cost_field", "assign_matrix", "tour_improve", "tour_improve"]
    want = cc.fields(g, cost, [[s] for s in ids], True, True)[0].reshape(6, -1)[:, ids]
    assert t.matrix.tobytes() == ts.mirror(want).tobytes() and list(t.order) == ts.search(want, 0, starts=2, rounds=1)["order"]
    g2 = g.copy()
    g2[g2 > 1] = 0
    for r, c in [tuple(c) for c in np.argwhere(g2 == 0) if tuple(c) not in stops][:5]:
        g2[r, c] = 1
    e.update_grid(g2)
    t.refresh()
    want2 = cc.fields(g2, cost, [[s] for s in ids], True, True)[0].reshape(6, -1)[:, ids]
    assert t.matrix.tobytes() == ts.mirror(want2).tobytes() and t.total == ts.search(want2, 0, starts=2, rounds=1)["total"]
    with pytest.raises(ValueError, match="^TourSearch: refresh\\(cost\\) needs a tour search built with a cost map"):
        make(g, stops, engine=ModelEngine(g)).refresh(cost=cost)


def test_solve_matrices_over_the_model():
    from pathfit import TourSearch
    e = ModelEngine(fig7())
    mats = np.array([ts.matrix(k, 9, 1) for k in ("ints", "uniform", "euclid", "tenths")])
    mats[1][0, 5] = ts.INF
    out = TourSearch.solve_matrices(e, mats, end="return")
    assert e.improves[-1][:5] == (1, 9, 4, False, 144) and out.order.shape == (4, 9) and out.value.shape == (4, 2) and out.info.shape == (4, 4)
    for b in range(4):
        assert e.improves[-1][5][b].tolist() == tc.nearest_neighbour(ts.mirror(mats[b]), 1)
        o, v, st, info = ts.two_opt_numpy(mats[b], e.improves[-1][5][b], 1, 144)
        assert (list(out.order[b]), tuple(out.value[b]), out.status[b], tuple(out.info[b])) == (o, v, st, info)
    assert out.status.tolist() == [0, 1, 0, 0]
    starts = [[0, 3, 1, 2, 4, 5, 6, 7, 8], list(range(9))]
    out = TourSearch.solve_matrices(e, mats[2], starts, end="last", shared=True, max_moves=1)
    assert e.improves[-1][:5] == (2, 9, 2, True, 1) and e.improves[-1][5].tolist() == starts
    one = TourSearch.solve_matrices(e, mats[0])
    assert one.order.shape == (1, 9) and e.improves[-1][:5] == (0, 9, 1, False, 144)
