"""Placement argument checks: every ValueError before any device is touched, and the numpy side (the chunks, `keep`, the
perturbation stream and its dropped draws, incumbent replacement and its tie rule, history, placement_cost, loads, field, paths,
solve_matrices, refresh) over a model engine whose pf_place_improve is the checkers' (runs on a CPU-only host)."""
import numpy as np
import pytest

import cost_checkers as cc
import field_checkers as fc
import golden_io as gio
import place_checkers as pc
from test_assign_args import ModelEngine as FieldModelEngine


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import placement

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(placement, "Engine", boom)


class ModelEngine(FieldModelEngine):
    """The field calls of the assignment tests' model engine, and pf_place_improve as the checkers' literal loop; `improves` logs
    (mode, m, n, p, fixed, B, shared, max_moves, the start rows) per call.  `script`: keys to answer with instead, one list of
    (unserved, total, radius) per call."""

    def __init__(self, g, script=None):
        super().__init__(g)
        self.improves = []
        self.script = script

    def place_improve(self, mode, m, n, p, fixed, B, shared, d_mat, max_moves, d_sel, d_owner, d_value, d_status, d_info=None):
        self.calls.append("place_improve")
        mats = d_mat.a.reshape(-1, m, n)
        assert len(mats) == (1 if shared else B) and pc.first_bad_entry(mats) is None and pc.first_bad_row(d_sel.a, m, p, fixed) is None
        rows = d_sel.a.reshape(B, p).copy()
        self.improves.append((mode, m, n, p, fixed, B, bool(shared), max_moves, rows))
        for b in range(B):
            row, owner, v, st, info = pc.improve(mats[0 if shared else b], rows[b], mode, fixed, max_moves)
            if self.script is not None:
                uns, total, radius = self.script[len(self.improves) - 1][b]
                row, v, info = list(rows[b]), (total, radius, v[2], v[3]), (info[0], info[1], uns, info[3])
                owner = pc.owners(mats[0 if shared else b], [int(x) for x in row])
            d_sel.a[b * p:(b + 1) * p] = row
            if d_owner is not None:
                d_owner.a[b * n:(b + 1) * n] = owner
            d_value.a[4 * b:4 * b + 4] = v
            d_status.a[b] = st
            if d_info is not None:
                d_info.a[4 * b:4 * b + 4] = info


def fig7():
    return gio.grid("fig7")[0]


def make(g, sites, demands, count, **kw):
    from pathfit import Placement
    return Placement(g, sites, demands, count, **kw)


def gathered(g, sites, demands, ad=True, rs=True):
    mm = fc.move_masks(np.asarray(g, np.uint8), ad, rs)
    C = g.shape[1]
    fields = np.array([fc.reference_dijkstra(np.asarray(g, np.uint8), mm, r * C + c)[0] for r, c in sites]).reshape(len(sites), -1)
    return np.ascontiguousarray(fields[:, [r * C + c for r, c in demands]])


CELLS = pc.map_cells(fig7())
S9, D20 = CELLS[5::33], CELLS[2::15]                                  # 9 candidate sites, 20 demands


# ---- every ValueError, before the device
def test_grid_and_engine(no_engine):
    with pytest.raises(ValueError, match="^Placement: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)], [(0, 1)], 1)

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^Placement: the engine's grid has another shape"):
        make(fig7(), [(0, 0)], [(0, 1)], 1, engine=Other())
    with pytest.raises(AssertionError, match="the device was touched"):
        make(fig7(), S9, D20, 3)


def test_sites_demands_and_count(no_engine):
    g = np.zeros((70, 70), int)
    cells = [(r, c) for r in range(70) for c in range(70)]
    with pytest.raises(ValueError, match="^Placement: sites is empty"):
        make(g, [], [(0, 0)], 1)
    with pytest.raises(ValueError, match="^Placement: demands is empty"):
        make(g, [(0, 0)], [], 1)
    with pytest.raises(ValueError, match="^Placement: sites must be a list"):
        make(g, 5, [(0, 0)], 1)
    with pytest.raises(ValueError, match="^Placement: demands must be a list"):
        make(g, [(0, 0)], 5, 1)
    with pytest.raises(ValueError, match=r"^Placement: demands\[1\] = \(70, 0\) is outside the 70x70 grid"):
        make(g, [(0, 0)], [(0, 0), (70, 0)], 1)
    with pytest.raises(ValueError, match=r"^Placement: sites\[0\] must be an \(r, c\) pair"):
        make(g, [7], [(0, 0)], 1)
    with pytest.raises(ValueError, match="^Placement: 1025 sites; at most 1024 are searched"):
        make(g, cells[:1025], cells[:3], 2)
    with pytest.raises(ValueError, match="^Placement: 4097 demands; at most 4096 are served"):
        make(g, cells[:3], cells[:4097], 2)
    for bad in (0, 4, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match=r"^Placement: count must be an integer in \[1, 3\]"):
            make(g, cells[:3], cells[:9], bad)
    with pytest.raises(ValueError, match=r"^Placement: count must be an integer in \[1, 64\]"):
        make(g, cells[:100], cells[:9], 65)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, cells[:1024], cells[:4096], 64)


def test_objective_and_keep(no_engine):
    g = fig7()
    for bad in ("max_sum", "min", 0, None):
        with pytest.raises(ValueError, match="^Placement: objective must be 'sum' or 'max'"):
            make(g, S9, D20, 3, objective=bad)
    with pytest.raises(ValueError, match="^Placement: keep must be a list"):
        make(g, S9, D20, 3, keep=4)
    for bad in ([9], [-1], [1.5], ["a"], [True]):
        with pytest.raises(ValueError, match=r"^Placement: keep\[0\] = .* is outside \[0, 9\)"):
            make(g, S9, D20, 3, keep=bad)
    with pytest.raises(ValueError, match="^Placement: keep names a site twice"):
        make(g, S9, D20, 3, keep=[2, 2])
    with pytest.raises(ValueError, match="^Placement: keep holds 4 sites, more than count = 3"):
        make(g, S9, D20, 3, keep=[0, 1, 2, 3])
    for good in ([], [8], (0, 1, 2), np.array([4, 5])):
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, S9, D20, 3, keep=good)


def test_cost_map(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^Placement: cost has shape"):
        make(g, S9, D20, 3, cost=np.ones((20, 19)))
    c = np.ones((20, 20))
    c[tuple(np.argwhere(g != 1)[3])] = 0.5
    with pytest.raises(ValueError, match="^Placement: cost"):
        make(g, S9, D20, 3, cost=c)


def test_starts_rounds_seed_and_max_moves(no_engine):
    g = fig7()
    for name, bad in (("starts", (0, -1, 1.5, "8", True, None, (1 << 16) + 1)), ("rounds", (-1, 2.0, None, True)), ("seed", (-1, 0.5, None, "x")),
                      ("max_moves", (-1, (1 << 20) + 1, 3.0, True))):
        for v in bad:
            with pytest.raises(ValueError, match=f"^Placement: {name} must be an integer in "):
                make(g, S9, D20, 3, **{name: v})
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, S9, D20, 3, starts=1, rounds=0, seed=np.int64(5), max_moves=0)


def test_solve_matrices_errors():
    from pathfit import Placement
    e = ModelEngine(fig7())
    sm = Placement.solve_matrices
    with pytest.raises(ValueError, match="^Placement: mats has shape"):
        sm(e, np.zeros((2, 3, 4, 5)), [[0]])
    with pytest.raises(ValueError, match="^Placement: 1025 sites; at most 1024"):
        sm(e, np.zeros((1, 1025, 2)), [[0]])
    with pytest.raises(ValueError, match="^Placement: 4097 demands; at most 4096"):
        sm(e, np.zeros((1, 2, 4097)), [[0]])
    with pytest.raises(ValueError, match="^Placement: objective must be"):
        sm(e, np.zeros((1, 3, 3)), [[0]], objective="max_sum")
    with pytest.raises(ValueError, match="^Placement: shared=True takes one"):
        sm(e, np.zeros((2, 3, 3)), [[0], [1]], shared=True)
    with pytest.raises(ValueError, match="^Placement: max_moves must be an integer"):
        sm(e, np.zeros((2, 3, 3)), [[0], [1]], max_moves=-1)
    with pytest.raises(ValueError, match=r"^Placement: fixed must be an integer in \[0, 2\]"):
        sm(e, np.zeros((2, 3, 3)), [[0, 1], [1, 2]], fixed=3)
    with pytest.raises(ValueError, match=r"^Placement: count must be an integer in \[1, 3\]"):
        sm(e, np.zeros((1, 3, 3)), [[0, 1, 2, -1]])
    for rows in ([[0, 1]] * 2, [[0.0, 1.0]] * 3, "abc", [[[0]]] * 3):
        with pytest.raises(ValueError, match="^Placement: rows must be an integer array"):
            sm(e, np.zeros((3, 3, 3)), rows)
    a = np.array([pc.matrix("euclid", 4, 5, b) for b in range(3)])
    for x, shown in ((np.nan, "nan"), (-1.0, "-1.0"), (-0.0, "-0.0"), (2.0 ** 1010, "1.09")):
        bad = a.copy()
        bad[2, 1, 3], bad[1, 3, 4] = x, x
        with pytest.raises(ValueError, match=rf"^Placement: mats\[1, 3, 4\] = {shown}.* is neither"):
            sm(e, bad, [[0, 1]] * 3)
    for rows, fixed, at in (([[0, 1], [2, 2], [0, 1]], 0, r"\[1, 1\] = 2"), ([[0, 1], [2, 3], [0, 4]], 0, r"\[2, 1\] = 4"), ([[0, -2], [2, 3], [0, 1]], 0, r"\[0, 1\] = -2"),
                            ([[0, 1], [-1, 3], [0, 1]], 1, r"\[1, 0\] = -1")):
        with pytest.raises(ValueError, match=rf"^Placement: rows{at}: a start holds sites"):
            sm(e, a, rows, fixed=fixed)
    assert e.calls == []


# ---- the numpy side over the model engine
def test_the_facade_over_the_model():
    g = fig7()
    e = ModelEngine(g)
    search = dict(starts=4, rounds=3, seed=5)
    t = make(g, S9, D20, 3, keep=[6], engine=e, **search)
    m, n, p, want_m = 9, 20, 3, gathered(g, S9, D20)
    assert e.calls == ["dist_field_batch", "assign_matrix"] + ["place_improve"] * 4
    assert t.matrix.tobytes() == want_m.tobytes() and t.max_moves == 48
    # the calls: the kept row alone, then the rounds' perturbations of the incumbent, all over the one shared matrix
    assert [c[:8] for c in e.improves] == [(0, m, n, p, 1, 1, True, 48)] + [(0, m, n, p, 1, 4, True, 48)] * 3
    assert e.improves[0][8].tolist() == [[6, -1, -1]]
    rng = np.random.default_rng(5)
    best = pc.improve(want_m, [6, -1, -1], 0, 1, 48)
    for call in e.improves[1:]:
        assert call[8].tolist() == pc.perturbations(rng, best[0], 1, m, 4)
        for row in call[8]:
            got = pc.improve(want_m, row, 0, 1, 48)
            if pc.key_of_result(got, 0) < pc.key_of_result(best, 0):
                best = got
    want = pc.search(want_m, p, 0, keep=(6,), solver=pc.improve, **search)
    assert list(t.row) == want["row"] == best[0] and t.row[0] == 6 and t.sites == [v for v in t.row if v >= 0] and t.cells == [S9[v] for v in t.sites]
    assert (t.total, t.radius, t.unserved, t.moves, t.history) == (want["total"], want["radius"], want["unserved"], want["moves"], want["history"])
    assert t.feasible and len(t.history) == 4 and [t.sites[o] for o in t.owner] == want["owner"] and t.loads == [want["owner"].count(v) for v in t.sites]
    assert sum(t.loads) == n and t.placement_cost(t.sites) == (t.total, t.radius, 0)
    # placement_cost: any other set, the left-to-right sum
    near = want_m[[0, 4]].min(0)
    total = 0.0
    for x in near:
        total = total + float(x)
    assert t.placement_cost([0, 4]) == (total, float(near.max()), 0) and t.placement_cost([]) == (0.0, 0.0, n)
    with pytest.raises(ValueError, match=r"^Placement: sites\[1\] = 9 is outside \[0, 9\)"):
        t.placement_cost([0, 9])
    with pytest.raises(ValueError, match="^Placement: sites names a site twice"):
        t.placement_cost([1, 1])
    with pytest.raises(ValueError, match="^Placement: sites must be a sequence"):
        t.placement_cost(3)
    paths = t.paths()
    assert e.calls[6:] == ["dist_field_parents", "dist_field_paths"] and len(paths) == n
    for j, path in enumerate(paths):
        assert path[0] == t.cells[t.owner[j]] and path[-1] == D20[j]
    t.paths()
    assert e.calls[8:] == ["dist_field_paths"]                        # the parent maps are kept
    t.close()


@pytest.mark.parametrize("objective", ["sum", "max"])
def test_both_objectives_and_the_seed(objective):
    g = fig7()
    mode = pc.MODES[objective == "max"]
    want_m = gathered(g, S9, D20)
    runs = []
    for seed in (0, 0, 7):
        e = ModelEngine(g)
        t = make(g, S9, D20, 5, objective=objective, starts=6, rounds=2, seed=seed, max_moves=40, engine=e)
        want = pc.search(want_m, 5, mode, starts=6, rounds=2, seed=seed, max_moves=40)
        assert (list(t.row), t.total, t.radius, t.unserved, t.history, t.moves) == (want["row"], want["total"], want["radius"], want["unserved"], want["history"], want["moves"])
        assert all(c[7] == 40 and c[4] == 0 for c in e.improves) and all(len(k) == 2 + mode for k in t.history)
        runs.append(e.improves)
    assert all(np.array_equal(a[8], b[8]) for a, b in zip(runs[0], runs[1])) and not all(np.array_equal(a[8], b[8]) for a, b in zip(runs[0], runs[2]))


def test_dropped_draws_and_the_stream():
    from pathfit import placement
    rng = np.random.default_rng(11)
    draws = np.random.default_rng(11).integers(0, [8, 12], (6, 2, 2))          # Q = (p - f) // 4 = 2 draws a start
    row = [3, 7, 0, 1, 2, 4, 5, 6, 8, -1]
    rows = placement.perturbations(rng, row, 2, 12, 6)
    assert rows == pc.perturbations(np.random.default_rng(11), row, 2, 12, 6)
    dropped = 0
    for s in range(6):
        want = list(row)
        for slot, site in draws[s]:
            if int(site) in want:
                dropped += 1
            else:
                want[2 + int(slot)] = int(site)
        assert rows[s] == want and rows[s][:2] == [3, 7] and pc.valid_row(rows[s], 12, 10, 2)
    assert dropped > 0
    twin = np.random.default_rng(11)
    twin.integers(0, [8, 12], (6, 2, 2))
    assert rng.integers(0, 1 << 30) == twin.integers(0, 1 << 30)      # one draw a round, whatever was dropped


def test_the_incumbent_is_replaced_by_a_strictly_smaller_key_at_the_smallest_index():
    g = fig7()
    script = [[(0, 50.0, 9.0)], [(0, 50.0, 9.0), (1, 10.0, 1.0), (0, 50.0, 8.0)], [(0, 49.0, 9.0), (0, 48.0, 9.5), (0, 48.0, 9.0)], [(0, 48.0, 9.5), (0, 47.5, 9.9), (0, 40.0, 9.9)],
              [(0, 40.0, 9.9), (0, 40.0, 1.0), (1, 0.0, 0.0)]]
    e = ModelEngine(g, script)
    t = make(g, S9, D20, 3, starts=3, rounds=4, engine=e)
    assert t.history == [(0, 50.0), (0, 50.0), (0, 48.0), (0, 40.0), (0, 40.0)] and t.total == 40.0 and t.radius == 9.9
    rows = [c[8] for c in e.improves]                                 # (the scripted answers keep the start rows)
    rng = np.random.default_rng(0)
    incumbents = [rows[0][0], rows[0][0], rows[2][1], rows[3][2]]     # equal keys replace nothing; of two equal ones the first wins; unserved comes first
    for call, inc in zip(rows[1:], incumbents):
        assert call.tolist() == pc.perturbations(rng, [int(v) for v in inc], 0, 9, 3)
    assert list(t.row) == list(rows[3][2])
    e = ModelEngine(g, script)
    t = make(g, S9, D20, 3, objective="max", starts=3, rounds=4, engine=e)     # the same answers under (unserved, radius, total)
    assert t.history == [(0, 9.0, 50.0), (0, 8.0, 50.0), (0, 8.0, 50.0), (0, 8.0, 50.0), (0, 1.0, 40.0)]


def test_every_slot_kept_and_one_site():
    g = fig7()
    e = ModelEngine(g)
    t = make(g, S9, D20, 2, keep=[4, 1], rounds=3, engine=e)
    assert list(t.row) == [4, 1] and t.sites == [4, 1] and t.history == [t.history[0]] and e.calls.count("place_improve") == 1 and t.moves == 0
    assert e.improves[0][:8] == (0, 9, 20, 2, 2, 1, True, 32)
    one = make(g, S9[:1], D20[:1], 1, rounds=1, starts=2, engine=ModelEngine(g))
    assert one.sites == [0] and one.loads == [1] and one.total == one.matrix[0, 0] == one.radius and len(one.history) == 2


def test_the_chunks():
    from pathfit import Placement
    g = fig7()
    whole = make(g, S9[:7], D20[:9], 3, starts=3, rounds=1, engine=ModelEngine(g))

    class Small(Placement):
        CHUNK_BYTES = 3 * 400 * 8
    e = ModelEngine(g)
    t = Small(g, S9[:7], D20[:9], 3, starts=3, rounds=1, engine=e)
    assert t.chunk == 3 and whole.chunk == 7 and e.rows_asked == [3, 3, 1]
    assert e.calls == ["dist_field_batch", "assign_matrix"] * 3 + ["place_improve"] * 2
    assert t.matrix.tobytes() == whole.matrix.tobytes() and list(t.row) == list(whole.row) and t.history == whole.history
    want = [list(p.cells) for p in whole.paths()]
    assert [list(p.cells) for p in t.paths()] == want
    assert [list(p.cells) for p in t.paths()] == want


def test_a_demand_nobody_reaches_and_field():
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    g[:, 15] = 1
    e = ModelEngine(g)
    t = make(g, [(4, 2), (0, 12), (8, 3)], [(0, 0), (8, 14), (4, 18), (3, 3)], 2, engine=e)
    assert not t.feasible and t.unserved == 1 and t.owner[2] == -1 and sorted(t.sites)[-1] == 1 and t.loads == [list(t.owner).count(x) for x in range(2)]
    assert np.isfinite(t.total) and t.paths()[2] is None and all(p is not None for j, p in enumerate(t.paths()) if j != 2)

    from pathfit import nearest_field

    class Seen(Exception):
        pass

    def fake(grid, sets, ad, rs, engine=None):
        raise Seen(sets, engine)
    real = nearest_field.NearestSourceField
    nearest_field.NearestSourceField = fake
    try:
        with pytest.raises(Seen) as got:
            t.field()
        assert got.value.args == ([t.cells], e)
    finally:
        nearest_field.NearestSourceField = real


def test_a_cost_map_goes_through_pf_cost_field_and_refresh_recomputes():
    g = fig7()
    e = ModelEngine(g)
    cost = cc.cost_of_kind("u50", g.shape, 3)
    sites, demands = S9[:4], D20[:6]
    C = g.shape[1]
    sid, did = [r * C + c for r, c in sites], [r * C + c for r, c in demands]
    t = make(g, sites, demands, 2, cost=cost, starts=2, rounds=1, engine=e)
    assert e.calls == ["cost_field", "assign_matrix", "place_improve", "place_improve"]
    want = cc.fields(g, cost, [[s] for s in sid], True, True)[0].reshape(4, -1)[:, did]
    assert t.matrix.tobytes() == np.ascontiguousarray(want).tobytes() and list(t.row) == pc.search(want, 2, 0, starts=2, rounds=1)["row"]
    g2 = g.copy()
    g2[g2 > 1] = 0
    for r, c in [tuple(c) for c in np.argwhere(g2 == 0) if tuple(c) not in sites + demands][:5]:
        g2[r, c] = 1
    e.update_grid(g2)
    t.refresh()
    want2 = cc.fields(g2, cost, [[s] for s in sid], True, True)[0].reshape(4, -1)[:, did]
    assert t.matrix.tobytes() == np.ascontiguousarray(want2).tobytes() and t.total == pc.search(want2, 2, 0, starts=2, rounds=1)["total"]
    with pytest.raises(ValueError, match="^Placement: refresh\\(cost\\) needs a placement built with a cost map"):
        make(g, sites, demands, 2, engine=ModelEngine(g)).refresh(cost=cost)


def test_solve_matrices_over_the_model():
    from pathfit import Placement
    e = ModelEngine(fig7())
    mats = np.array([pc.matrix(kind, 6, 9, 1) for kind in pc.KINDS])
    rows = [[2, -1, -1], [2, 0, 5], [2, -1, 4], [-1 + 3, 1, -1]]
    out = Placement.solve_matrices(e, mats, rows, objective="max", fixed=1)
    assert e.improves[-1][:8] == (1, 6, 9, 3, 1, 4, False, 48) and e.improves[-1][8].tolist() == rows
    assert out.row.shape == (4, 3) and out.owner.shape == (4, 9) and out.value.shape == (4, 4) and out.info.shape == (4, 4)
    for b in range(4):
        row, owner, v, st, info = pc.improve_numpy(mats[b], rows[b], 1, 1, 48)
        assert (list(out.row[b]), list(out.owner[b]), tuple(out.value[b]), out.status[b], tuple(out.info[b])) == (row, owner, v, st, info)
    Placement.solve_matrices(e, mats[0], [[-1, -1]] * 5, shared=True, max_moves=1)
    assert e.improves[-1][:8] == (0, 6, 9, 2, 0, 5, True, 1)
    one = Placement.solve_matrices(e, mats[0], [0, 1, 2])
    assert one.row.shape == (1, 3) and e.improves[-1][:8] == (0, 6, 9, 3, 0, 1, False, 48)
    doubled = np.concatenate([mats[0], mats[0][:, :2]], axis=1)      # a demand listed twice counts twice
    out = Placement.solve_matrices(e, doubled, [[0]], max_moves=0)
    assert out.value[0, 0] == pc.cost(doubled, [0])[1] > pc.cost(mats[0], [0])[1]
