"""Assignment argument checks: every ValueError before any device is touched, and the numpy side (task_of / robot_of on both sides
of n <= m, assignment_cost, pairs, the chunks, solve_matrices' transposition, refresh) over a model engine whose assign calls are
the checkers (runs on a CPU-only host)."""
import numpy as np
import pytest

import assign_checkers as ac
import cost_checkers as cc
import field_checkers as fc
import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import assignment

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(assignment, "Engine", boom)


class HostBuf:
    def __init__(self, shape, dtype):
        self.a = np.zeros(shape, dtype).reshape(-1)
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)

    def download(self):
        return self.a.copy().reshape(self.shape)

    def upload(self, arr):
        self.a[:] = np.asarray(arr, self.a.dtype).reshape(-1)
        return self

    def free(self):
        pass


class ModelEngine:
    """An engine of the grid's shape whose calls are the CPU checkers; `calls` logs them by name."""
    h = 1

    def __init__(self, g):
        self.grid_u8 = np.asarray(g, np.uint8)
        self.R, self.C = self.grid_u8.shape
        self.calls = []
        self.rows_asked = []

    def update_grid(self, g):
        self.grid_u8 = np.asarray(g, np.uint8)

    def buf(self, shape, dtype):
        return HostBuf(shape, dtype)

    def put(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype)
        return HostBuf(a.shape if a.ndim else (1,), a.dtype).upload(a)

    def last_kernel_ms(self):
        return 0.0

    def default_path_cap(self):
        return self.R * self.C

    def dist_field_batch(self, ids, d_out, ad, rs):
        self.calls.append("dist_field_batch")
        self.rows_asked.append(len(ids))
        mm = fc.move_masks(self.grid_u8, ad, rs)
        rows = np.array([fc.reference_dijkstra(self.grid_u8, mm, int(s))[0] for s in ids]).reshape(-1)
        d_out.a[:len(rows)] = rows

    def cost_field(self, d_cost, off, ids, d_out, ad, rs):
        self.calls.append("cost_field")
        assert list(off) == list(range(len(ids) + 1))
        rows = cc.fields(self.grid_u8, d_cost.a.reshape(self.R, self.C), [[int(s)] for s in ids], ad, rs)[0].reshape(-1)
        d_out.a[:len(rows)] = rows

    def assign_matrix(self, n_rows, cols, d_fields, d_mat, row0=0, ld=None, transpose=False):
        self.calls.append("assign_matrix")
        cols = np.asarray(cols)
        ld = len(cols) if ld is None else ld
        got = d_fields.a[:n_rows * self.R * self.C].reshape(n_rows, -1)[:, cols]
        view = d_mat.a.reshape(-1, ld)
        if transpose:
            view[:len(cols), row0:row0 + n_rows] = got.T
        else:
            view[row0:row0 + n_rows, :len(cols)] = got

    def assign_solve(self, mode, n, m, B, d_mat, d_col, d_value, d_status, d_dual=None, d_info=None):
        self.calls.append("assign_solve")
        self.shape = (mode, n, m, B)
        for b, a in enumerate(d_mat.a.reshape(B, n, m)):
            r = ac.solve(a, mode)
            d_col.a[b * n:(b + 1) * n] = r.col
            d_value.a[2 * b:2 * b + 2] = (r.sum, r.max)
            d_status.a[b] = r.status
            if d_dual is not None:
                d_dual.a[b * (n + m):(b + 1) * (n + m)] = r.dual
            if d_info is not None:
                d_info.a[4 * b:4 * b + 4] = r.info

    def dist_field_parents(self, K, d_fields, d_parents, ad, rs):
        self.calls.append("dist_field_parents")
        mm = fc.move_masks(self.grid_u8, ad, rs)
        rows = np.array([fc.rule_parents(f, mm) for f in d_fields.a[:K * self.R * self.C].reshape(K, self.R, self.C)]).reshape(-1)
        d_parents.a[:len(rows)] = rows

    def dist_field_paths(self, K, d_parents, d_target, n, cap, d_cells, d_len, d_status, d_field_idx, d_fields, reverse, d_chosen):
        self.calls.append("dist_field_paths")
        codes = d_parents.a[:K * self.R * self.C].reshape(K, self.R, self.C)
        for q in range(n):
            row = fc.trace(codes[d_field_idx.a[q]], int(d_target.a[q]))
            d_len.a[q], d_status.a[q] = len(row), 0 if row else 1
            d_cells.a[q * cap:q * cap + len(row)] = row

    def __getattr__(self, name):
        raise AssertionError(f"the model engine has no {name}")


def fig7():
    return gio.grid("fig7")[0]


def make(g, robots, tasks, **kw):
    from pathfit import Assignment
    return Assignment(g, robots, tasks, **kw)


# ---- every ValueError, before the device
def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^Assignment: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)], [(0, 1)])


def test_engine_of_another_shape(no_engine):
    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^Assignment: the engine's grid has another shape"):
        make(fig7(), [(0, 0)], [(0, 1)], engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    with pytest.raises(AssertionError, match="the device was touched"):
        make(fig7(), ac.GREEDY_ROBOTS, ac.GREEDY_TASKS)


def test_robots_and_tasks(no_engine):
    g = np.zeros((40, 40), int)
    for what, args in (("robots", lambda v: (v, [(0, 0)])), ("tasks", lambda v: ([(0, 0)], v))):
        with pytest.raises(ValueError, match=f"^Assignment: {what} is empty"):
            make(g, *args([]))
        with pytest.raises(ValueError, match=f"^Assignment: {what} must be a list"):
            make(g, *args(5))
        with pytest.raises(ValueError, match=rf"^Assignment: {what}\[1\] = \(40, 0\) is outside the 40x40 grid"):
            make(g, *args([(0, 0), (40, 0)]))
        with pytest.raises(ValueError, match=rf"^Assignment: {what}\[0\] must be an \(r, c\) pair"):
            make(g, *args([7]))
        cells = [(r, c) for r in range(26) for c in range(40)]
        with pytest.raises(ValueError, match=f"^Assignment: 1025 {what}; at most 1024"):
            make(g, *args(cells[:1025]))
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, *args(cells[:1024]))


def test_objective(no_engine):
    for objective in ("min", 0, None):
        with pytest.raises(ValueError, match="^Assignment: objective must be 'sum', 'max' or 'max_sum'"):
            make(fig7(), [(0, 0)], [(0, 1)], objective=objective)


def test_cost_map(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^Assignment: cost has shape"):
        make(g, [(0, 0)], [(0, 1)], cost=np.ones((20, 19)))
    c = np.ones((20, 20))
    free = np.argwhere(g != 1)[3]
    c[tuple(free)] = 0.5
    with pytest.raises(ValueError, match="^Assignment: cost"):
        make(g, [(0, 0)], [(0, 1)], cost=c)


def test_solve_matrices_errors():
    from pathfit import Assignment
    e = ModelEngine(fig7())
    with pytest.raises(ValueError, match="^Assignment: matrices has shape"):
        Assignment.solve_matrices(np.zeros((2, 3, 4, 5)), "sum", e)
    with pytest.raises(ValueError, match="^Assignment: matrices has shape"):
        Assignment.solve_matrices(np.zeros((2, 0, 4)), "sum", e)
    with pytest.raises(ValueError, match="^Assignment: matrices of 3 x 1025"):
        Assignment.solve_matrices(np.zeros((1, 3, 1025)), "sum", e)
    m = ac.matrix("real", 3, 4, 0)[None].repeat(3, 0)
    for x, shown in ((np.nan, "nan"), (-np.inf, "-inf"), (2.0 ** 1001, "2.14")):
        bad = m.copy()
        bad[2, 1, 3] = x
        with pytest.raises(ValueError, match=rf"^Assignment: matrices\[2, 1, 3\] = {shown}.* is neither"):
            Assignment.solve_matrices(bad, "sum", e)
    with pytest.raises(ValueError, match="^Assignment: objective must be"):
        Assignment.solve_matrices(m, "x", e)
    assert e.calls == []


# ---- the numpy side over the model engine
def test_the_facade_over_the_model():
    g = fig7()
    e = ModelEngine(g)
    t = make(g, ac.GREEDY_ROBOTS, ac.GREEDY_TASKS, engine=e)
    assert e.calls == ["dist_field_batch", "assign_matrix", "assign_solve"] and e.shape == (0, 8, 8, 1)
    want = ac.solve(t.matrix, 0)
    assert t.feasible and t.total == ac.GREEDY_OPTIMUM and list(t.task_of) == want.col and t.makespan == want.max
    assert [list(t.task_of).index(j) for j in range(8)] == list(t.robot_of)
    assert t.duals.tobytes() == want.dual.tobytes() and list(t.info) == want.info
    assert t.assignment_cost(t.task_of) == (t.total, t.makespan)
    assert t.assignment_cost(ac.greedy_nearest(t.matrix))[0] == ac.GREEDY_COST
    assert t.assignment_cost([-1] * 8) == (0.0, -ac.INF)
    with pytest.raises(ValueError, match=r"^Assignment: task_of\[1\] = 8 is outside \[0, 8\)"):
        t.assignment_cost([0, 8, 1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError, match="^Assignment: task_of has 2 entries for 8 robots"):
        t.assignment_cost([0, 1])
    with pytest.raises(ValueError, match="^Assignment: task_of gives a task to two robots"):
        t.assignment_cost([0, 0, 1, 2, 3, 4, 5, 6])
    starts, goals = t.pairs()
    assert starts == ac.GREEDY_ROBOTS and goals == [ac.GREEDY_TASKS[j] for j in t.task_of]
    paths = t.paths()
    assert e.calls[3:] == ["dist_field_parents", "dist_field_paths"] and len(paths) == 8
    for p, s, q in zip(paths, starts, goals):
        assert p[0] == s and p[-1] == q
    t.paths()
    assert e.calls[5:] == ["dist_field_paths"]                        # the parent maps are kept
    t.close()


@pytest.mark.parametrize("nr,nt", [(3, 6), (6, 3)])
def test_both_sides_of_n_le_m(nr, nt):
    g = fig7()
    cells = ac.free_cells(g, nr + nt, 4)
    robots, tasks = cells[:nr], cells[nr:]
    e = ModelEngine(g)
    for objective in ("sum", "max", "max_sum"):
        t = make(g, robots, tasks, objective=objective, engine=e)
        assert e.shape == (ac.OBJECTIVES[objective], 3, 6, 1) and t.transposed == (nr > nt)
        mm = fc.move_masks(g, 1, 1)
        want_m = np.array([[fc.reference_dijkstra(g, mm, r * 20 + c)[0][tr, tc] for tr, tc in tasks] for r, c in robots])
        assert t.matrix.tobytes() == want_m.tobytes()
        want = ac.solve(want_m.T if nr > nt else want_m, ac.OBJECTIVES[objective])
        small, large = (t.robot_of, t.task_of) if nr > nt else (t.task_of, t.robot_of)
        assert list(small) == want.col and sorted(v for v in large if v >= 0) == [0, 1, 2] and list(large).count(-1) == 3
        assert all(small[large[k]] == k for k in range(6) if large[k] >= 0)
        assert t.assignment_cost(t.task_of) == (t.total, t.makespan) == (want.sum, want.max)
        starts, goals = t.pairs()
        assert len(starts) == len(goals) == 3 == len(t.paths())
        assert starts == [robots[i] for i in range(nr) if t.task_of[i] >= 0]


def test_the_chunks():
    from pathfit import Assignment
    from pathfit.assignment import chunk_rows
    assert chunk_rows(8, 400, 256 << 20) == 8 and chunk_rows(1024, 1 << 20, 256 << 20) == 32
    assert chunk_rows(5, 1 << 26, 256 << 20) == 1 and chunk_rows(7, 400, 3 * 400 * 8) == 3 and chunk_rows(7, 400, 3 * 400 * 8 - 1) == 2
    g = fig7()
    cells = ac.free_cells(g, 12, 8)
    robots, tasks = cells[:7], cells[7:]                               # more robots than tasks: the chunks are gathered transposed
    whole = make(g, robots, tasks, engine=ModelEngine(g))

    class Small(Assignment):
        CHUNK_BYTES = 3 * 400 * 8
    e = ModelEngine(g)
    t = Small(g, robots, tasks, engine=e)
    assert t.chunk == 3 and e.rows_asked == [3, 3, 1] and e.calls == ["dist_field_batch", "assign_matrix"] * 3 + ["assign_solve"]
    assert t.matrix.tobytes() == whole.matrix.tobytes() and list(t.task_of) == list(whole.task_of) and t.total == whole.total
    want = [list(p.cells) for p in whole.paths()]
    assert [list(p.cells) for p in t.paths()] == want
    held, again = 6, 0                                                # the last chunk computed is the one held
    for r0 in (6, 0, 3):                                              # the chunk held is visited first: it is not computed again
        if any(t.task_of[i] >= 0 for i in range(r0, min(r0 + 3, 7))) and held != r0:
            held, again = r0, again + 1
    assert e.calls[7:].count("dist_field_batch") == again >= 1        # a released chunk is computed again
    assert [list(p.cells) for p in t.paths()] == want


def test_a_cost_map_goes_through_pf_cost_field_and_refresh_recomputes():
    g = fig7()
    e = ModelEngine(g)
    cost = cc.cost_of_kind("u50", g.shape, 3)
    cells = ac.free_cells(g, 7, 2)
    robots, tasks = cells[:3], cells[3:]
    t = make(g, robots, tasks, cost=cost, engine=e)
    assert e.calls == ["cost_field", "assign_matrix", "assign_solve"]
    rid, tid = [r * 20 + c for r, c in robots], [r * 20 + c for r, c in tasks]
    want = cc.fields(g, cost, [[s] for s in rid], True, True)[0].reshape(3, -1)[:, tid]
    assert np.array_equal(t.matrix.view(np.int64), want.view(np.int64)) and list(t.task_of) == ac.solve(want, 0).col
    g2 = g.copy()
    g2[g2 > 1] = 0
    wall = [tuple(c) for c in np.argwhere(g2 == 0) if tuple(c) not in cells][:5]
    for r, c in wall:
        g2[r, c] = 1
    e.update_grid(g2)
    t.refresh()
    want2 = cc.fields(g2, cost, [[s] for s in rid], True, True)[0].reshape(3, -1)[:, tid]
    assert np.array_equal(t.matrix.view(np.int64), want2.view(np.int64)) and list(t.task_of) == ac.solve(want2, 0).col
    with pytest.raises(ValueError, match="^Assignment: refresh\\(cost\\) needs an assignment built with a cost map"):
        make(g, robots, tasks, engine=ModelEngine(g)).refresh(cost=cost)


def test_solve_matrices_over_the_model():
    from pathfit import Assignment
    e = ModelEngine(fig7())
    mats = np.array([ac.matrix(k, 4, 6, 1) for k in ac.KINDS])
    out = Assignment.solve_matrices(mats, "max_sum", e)
    assert e.shape == (2, 4, 6, 7) and out.task_of.shape == (7, 4) and out.robot_of.shape == (7, 6) and out.dual.shape == (7, 10)
    for b in range(7):
        want = ac.solve(mats[b], 2)
        assert list(out.task_of[b]) == want.col and (ac.bits(out.value[b, 0]), ac.bits(out.value[b, 1])) == (ac.bits(want.sum), ac.bits(want.max))
        assert out.status[b] == want.status and list(out.info[b]) == want.info and out.dual[b].tobytes() == want.dual.tobytes()
    tall = np.ascontiguousarray(mats.transpose(0, 2, 1))               # [7, 6, 4]: solved transposed, answered as given
    out2 = Assignment.solve_matrices(tall, "max_sum", e)
    assert e.shape == (2, 4, 6, 7) and out2.task_of.shape == (7, 6) and out2.robot_of.shape == (7, 4)
    assert out2.task_of.tobytes() == out.robot_of.tobytes() and out2.robot_of.tobytes() == out.task_of.tobytes()
    assert out2.value.tobytes() == out.value.tobytes()
    one = Assignment.solve_matrices(mats[0], "sum", e)
    assert one.task_of.shape == (1, 4) and list(one.task_of[0]) == ac.solve(mats[0], 0).col
