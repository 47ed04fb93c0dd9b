"""FleetTours(objective="makespan") on a CPU-only host: every new ValueError before any device is touched, and the search driver
over a model engine whose pf_fleet_improve and pf_fleet_balance are the checkers' (the two-step round 0, the rounds' calls,
incumbent replacement by the strictly smallest (makespan, total) and its tie rule, history, total_history, route_makespan,
balance_matrices)."""
import numpy as np
import pytest

import fleet_balance_checkers as fb
import fleet_checkers as fl
from test_fleet_args import ModelEngine as SumModelEngine
from test_fleet_args import R3, T12, fig7, gathered, make, no_engine  # noqa: F401  (no_engine is a fixture)


class ModelEngine(SumModelEngine):
    """test_fleet_args' model engine, and pf_fleet_balance as the checkers' numpy form; `balances` logs (mode, k, n, B, shared,
    caps, max_moves, the start rows) per call.  `pairs`: (makespan, total) pairs to answer with instead, one list per call."""

    def __init__(self, g, pairs=None):
        super().__init__(g)
        self.balances = []
        self.pairs = pairs

    def fleet_balance(self, mode, k, n, B, shared, d_mat, d_cap, max_moves, d_route, d_len, d_value, d_status, d_info=None):
        self.calls.append("fleet_balance")
        N = k + n
        mats = d_mat.a.reshape(-1, N, N)
        cap = None if d_cap is None else [int(c) for c in d_cap.a]
        assert len(mats) == (1 if shared else B) and (cap is None or len(cap) == k)
        assert fl.first_bad_row(d_route.a, k, N) is None and fl.first_over_cap(d_route.a, k, N, cap) is None
        rows = d_route.a.reshape(B, N).copy()
        self.balances.append((mode, k, n, B, bool(shared), cap, max_moves, rows))
        for b in range(B):
            o, lens, v, st, info = fb.balance_numpy(mats[0 if shared else b], rows[b], k, mode, cap, max_moves)
            if self.pairs is not None and st != 1:
                o, v = list(rows[b]), tuple(self.pairs[len(self.balances) - 1][b]) + v[2:]
            d_route.a[b * N:(b + 1) * N] = o
            d_len.a[b * k:(b + 1) * k] = lens
            d_value.a[4 * b:4 * b + 4] = v
            d_status.a[b] = st
            if d_info is not None:
                d_info.a[5 * b:5 * b + 5] = info


def test_objective(no_engine):
    for bad in ("max", "Makespan", "", 0, None, True, ["sum"]):
        with pytest.raises(ValueError, match="^FleetTours: objective must be 'sum' or 'makespan'"):
            make(fig7(), R3, T12, objective=bad)
    for good in ("sum", "makespan"):
        with pytest.raises(AssertionError, match="the device was touched"):
            make(fig7(), R3, T12, objective=good)
    for kw, msg in ((dict(end="last"), "end must be"), (dict(capacity=3), "the capacities hold 9 tasks"), (dict(starts=0), "starts must be an integer"),
                    (dict(max_moves=-1), "max_moves must be an integer")):
        with pytest.raises(ValueError, match=f"^FleetTours: {msg}"):    # the other arguments are checked as before, whatever the objective
            make(fig7(), R3, T12, objective="makespan", **kw)


def test_balance_matrices_errors():
    from pathfit import FleetTours
    e = ModelEngine(fig7())
    bm = FleetTours.balance_matrices
    with pytest.raises(ValueError, match="^FleetTours: mats has shape"):
        bm(e, np.zeros((2, 3, 4)), 1)
    with pytest.raises(ValueError, match="^FleetTours: tasks is empty"):
        bm(e, np.zeros((1, 3, 3)), 3)
    with pytest.raises(ValueError, match="^FleetTours: k must be an integer in"):
        bm(e, np.zeros((1, 3, 3)), 0)
    with pytest.raises(ValueError, match="^FleetTours: end must be"):
        bm(e, np.zeros((1, 3, 3)), 1, end="last")
    with pytest.raises(ValueError, match="^FleetTours: shared=True takes one"):
        bm(e, np.zeros((2, 3, 3)), 1, shared=True)
    with pytest.raises(ValueError, match="^FleetTours: max_moves must be an integer"):
        bm(e, np.zeros((2, 3, 3)), 1, max_moves=-1)
    m = np.array([fl.matrix("uniform", 5, b) for b in range(3)])
    bad = m.copy()
    bad[2, 1, 3] = np.nan
    with pytest.raises(ValueError, match=r"^FleetTours: mats\[2, 1, 3\] = nan.* is neither"):
        bm(e, bad, 2)
    with pytest.raises(ValueError, match=r"^FleetTours: routes\[1, 2\] = 2: a start is a permutation"):
        bm(e, m, 2, [[0, 2, 1, 3, 4], [0, 2, 2, 1, 4], [0, 1, 2, 3, 4]])
    with pytest.raises(ValueError, match=r"^FleetTours: routes\[1\] gives robot 0 3 tasks, more than its capacity 2"):
        bm(e, m, 2, [[0, 2, 1, 3, 4], [0, 2, 3, 4, 1], [0, 1, 2, 3, 4]], capacity=[2, 3])
    assert e.calls == []


def test_the_facade_over_the_model():
    g = fig7()
    k, n, N, want_m = 3, 12, 15, gathered(g, R3 + T12)
    for end in ("open", "return"):
        mode = fl.MODES[end == "return"]
        e = ModelEngine(g)
        t = make(g, R3, T12, end=end, engine=e, objective="makespan", **fl.MAP_SEARCH)
        # round 0 improves the greedy start under the sum rule and balances the result; each round is one balance call
        assert e.calls == ["dist_field_batch", "assign_matrix", "fleet_improve"] + ["fleet_balance"] * 4
        assert [c[:7] for c in e.improves] == [(mode, k, n, 1, True, None, 16 * N)]
        assert [c[:7] for c in e.balances] == [(mode, k, n, 1, True, None, 16 * N)] + [(mode, k, n, 8, True, None, 16 * N)] * 3
        start = fl.start_row(t.matrix, k, None)
        assert e.improves[0][7].tolist() == [start]
        assert e.balances[0][7].tolist() == [fl.improve(want_m, start, k, mode, None, 16 * N)[0]]
        got = fb.balance_numpy(want_m, e.balances[0][7][0], k, mode, None, 16 * N)
        rng, best, o = np.random.default_rng(0), (got[2][0], got[2][1]), got[0]
        for call in e.balances[1:]:
            assert call[7].tolist() == fl.perturbations(rng, o, k, None, 8)
            for row in call[7]:
                got = fb.balance_numpy(want_m, row, k, mode, None, 16 * N)
                if (got[2][0], got[2][1]) < best:
                    best, o = (got[2][0], got[2][1]), got[0]
        want = fb.search(want_m, k, mode, **fl.MAP_SEARCH)
        assert t.feasible and list(t.route) == want["route"] == o and t.routes == want["routes"] == fb.MAP_BALANCED_ROUTES[mode] and t.moves == want["moves"]
        assert t.history == want["history"] and t.total_history == want["total_history"] and t.lengths == want["lengths"]
        assert (t.makespan, t.total) == best == fb.MAP_BALANCED[mode] and t.makespan == max(t.lengths) == t.history[-1] and t.total == t.total_history[-1]
        assert (t.start_total, t.start_makespan) == (want["start_total"], want["start_makespan"]) == fl.lengths(t.matrix, start, k, mode)[1:]
        assert t.route_makespan(t.routes) == t.makespan and t.route_cost(t.routes) == t.total
        assert t.route_makespan([[], [], []]) == 0.0 and t.route_makespan([[0], [], [1, 2]]) == max(fl.lengths(t.matrix, fl.row_of([[3], [], [4, 5]]), k, mode)[0])
        with pytest.raises(ValueError, match=r"^FleetTours: routes\[1\]\[0\] = 12 is outside \[0, 12\)"):
            t.route_makespan([[0], [12], []])
        assert [len(x) for x in t.legs()] == [len(r) + (mode == 1 and len(r) > 0) for r in t.routes]
        # the sum objective on the same engine class: the calls, the attributes and the numbers of before
        e = ModelEngine(g)
        s = make(g, R3, T12, end=end, engine=e, **fl.MAP_SEARCH)
        assert e.calls == ["dist_field_batch", "assign_matrix"] + ["fleet_improve"] * 4 and e.balances == [] and s.objective == "sum"
        assert (s.makespan, s.total) == fb.MAP_SUM[mode] and s.total_history == s.history and (s.start_total, s.start_makespan) == (t.start_total, t.start_makespan)
        assert t.makespan < s.makespan and t.total > s.total


def test_the_incumbent_is_replaced_by_a_strictly_smaller_pair_at_the_smallest_index():
    g = fig7()
    pairs = [[(50.0, 90.0)], [(50.0, 90.0), (60.0, 10.0), (50.0, 95.0)], [(50.0, 89.0), (49.0, 99.0), (49.0, 99.0)], [(49.0, 99.0), (49.0, 98.5), (49.0, 98.5)],
             [(49.5, 1.0), (49.0, 98.5), (48.0, 200.0)]]
    e = ModelEngine(g, pairs)
    t = make(g, R3, T12[:6], starts=3, rounds=4, engine=e, objective="makespan")
    assert t.history == [50.0, 50.0, 49.0, 49.0, 48.0] and t.total_history == [90.0, 90.0, 99.0, 98.5, 200.0] and (t.makespan, t.total) == (48.0, 200.0)
    rows = [c[7] for c in e.balances]                                 # (the scripted answers keep the start rows)
    rng = np.random.default_rng(0)
    # an equal pair and a larger makespan with a smaller total replace nothing; the makespan decides before the total; of two equal
    # pairs the first wins; an equal makespan with a smaller total replaces
    incumbents = [rows[0][0], rows[0][0], rows[2][1], rows[3][1]]
    for call, inc in zip(rows[1:], incumbents):
        assert call.tolist() == fl.perturbations(rng, inc, 3, None, 3)
    assert list(t.route) == list(rows[4][2]) and e.calls.count("fleet_improve") == 1


def test_an_unreachable_task_and_the_smallest_fleet():
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    e = ModelEngine(g)
    t = make(g, [(4, 2)], [(0, 18), (8, 3)], engine=e, objective="makespan")
    assert not t.feasible and t.total == t.makespan == t.start_total == t.start_makespan == fl.INF and t.history == t.total_history == [fl.INF]
    assert list(t.route) == [-1] * 3 and t.moves == 0 and t.routes == [[]] and t.legs() == [] and e.calls.count("fleet_balance") == 0
    one = make(fig7(), R3[:1], T12[:1], end="return", rounds=1, starts=2, engine=ModelEngine(fig7()), objective="makespan")
    assert one.routes == [[0]] and one.total == one.makespan == 2 * one.matrix[0, 1] and one.history == one.total_history == [one.total] * 2


def test_balance_matrices_over_the_model():
    from pathfit import FleetTours
    e = ModelEngine(fig7())
    mats = np.array([fl.matrix(kind, 9, 1) for kind in ("ints", "uniform", "euclid", "ints")])
    mats[1][0, 5] = fl.INF
    out = FleetTours.balance_matrices(e, mats, 3, end="return", capacity=[3, 2, 4])
    assert e.balances[-1][:7] == (1, 3, 6, 4, False, [3, 2, 4], 144) and e.improves == []
    assert out.route.shape == (4, 9) and out.lengths.shape == (4, 3) and out.value.shape == (4, 4) and out.info.shape == (4, 5)
    for b in range(4):
        assert e.balances[-1][7][b].tolist() == fl.start_row(fl.mirror(mats[b]), 3, [3, 2, 4])
        o, lens, v, st, info = fb.balance_numpy(mats[b], e.balances[-1][7][b], 3, 1, [3, 2, 4], 144)
        assert (list(out.route[b]), list(out.lengths[b]), tuple(out.value[b]), out.status[b], tuple(out.info[b])) == (o, lens, v, st, info)
    assert out.status.tolist() == [0, 1, 0, 0]
    starts = [[0, 3, 1, 2, 4, 5, 6, 7, 8], [0, 1, 2, 3, 4, 5, 6, 7, 8]]
    FleetTours.balance_matrices(e, mats[2], 3, starts, shared=True, max_moves=1)
    assert e.balances[-1][:7] == (0, 3, 6, 2, True, None, 1) and e.balances[-1][7].tolist() == starts
