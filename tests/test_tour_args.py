"""Tour argument checks: every ValueError before any device is touched, and the numpy side (route_cost, the joining of legs, `before`
to need words, solve_matrices) over a model engine whose tour calls are the checker (runs on a CPU-only host)."""
import numpy as np
import pytest

import cost_checkers as cc
import field_checkers as fc
import golden_io as gio
import tour_checkers as tc


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import tour

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(tour, "Engine", boom)


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
        mm = fc.move_masks(self.grid_u8, ad, rs)
        d_out.a[:] = np.array([fc.reference_dijkstra(self.grid_u8, mm, int(s))[0] for s in ids]).reshape(-1)

    def cost_field(self, d_cost, off, ids, d_out, ad, rs):
        self.calls.append("cost_field")
        assert list(off) == list(range(len(ids) + 1))
        d_out.a[:] = cc.fields(self.grid_u8, d_cost.a.reshape(self.R, self.C), [[int(s)] for s in ids], ad, rs)[0].reshape(-1)

    def tour_matrix(self, ids, d_fields, d_mat):
        self.calls.append("tour_matrix")
        n = len(ids)
        d_mat.a[:] = d_fields.a.reshape(n, -1)[:, np.asarray(ids)].reshape(-1)

    def tour_solve(self, mode, n, B, d_mat, d_total, d_order, d_status, need=None, d_info=None):
        self.calls.append("tour_solve")
        self.need = None if need is None else [int(v) for v in need]
        for b, d in enumerate(d_mat.a.reshape(B, n, n)):
            total, order, finite, last = tc.held_karp(d, mode, self.need)
            d_total.a[b], d_status.a[b] = total, 0 if total < tc.INF else 1
            d_order.a[b * n:(b + 1) * n] = order
            if d_info is not None:
                d_info.a[4 * b:4 * b + 4] = (finite, last, 0, 0)

    def dist_field_parents(self, K, d_fields, d_parents, ad, rs):
        self.calls.append("dist_field_parents")
        mm = fc.move_masks(self.grid_u8, ad, rs)
        d_parents.a[:] = np.array([fc.rule_parents(f, mm) for f in d_fields.a.reshape(K, self.R, self.C)]).reshape(-1)

    def dist_field_paths(self, K, d_parents, d_target, n, cap, d_cells, d_len, d_status, d_field_idx, d_fields, reverse, d_chosen):
        self.calls.append("dist_field_paths")
        codes = d_parents.a.reshape(K, self.R, self.C)
        for q in range(n):
            row = fc.trace(codes[d_field_idx.a[q]], int(d_target.a[q]))
            d_len.a[q], d_status.a[q] = len(row), 0 if row else 1
            d_cells.a[q * cap:q * cap + len(row)] = row

    def __getattr__(self, name):
        raise AssertionError(f"the model engine has no {name}")


def fig7():
    return gio.grid("fig7")[0]


def make(g, stops, **kw):
    from pathfit import Tour
    return Tour(g, stops, **kw)


# ---- every ValueError, before the device
def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^Tour: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)])


def test_engine_of_another_shape(no_engine):
    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^Tour: the engine's grid has another shape"):
        make(fig7(), [(0, 0)], engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    with pytest.raises(AssertionError, match="the device was touched"):
        make(fig7(), tc.NN_STOPS)


def test_stops(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^Tour: stops is empty"):
        make(g, [])
    with pytest.raises(ValueError, match="^Tour: stops must be a list"):
        make(g, 5)
    with pytest.raises(ValueError, match=r"^Tour: stops\[1\] = \(20, 0\) is outside the 20x20 grid"):
        make(g, [(0, 0), (20, 0)])
    with pytest.raises(ValueError, match=r"^Tour: stops\[0\] must be an \(r, c\) pair"):
        make(g, [7])
    cells = [(r, c) for r in range(2) for c in range(10)]
    for end, most in (("open", 17), ("return", 17), ("last", 18)):
        with pytest.raises(ValueError, match=f"^Tour: {most + 1} stops; at most {most}"):
            make(g, cells[:most + 1], end=end)
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, cells[:most], end=end)
    with pytest.raises(ValueError, match="^Tour: end='last' needs at least two stops"):
        make(g, [(0, 0)], end="last")


def test_end(no_engine):
    for end in ("closed", 1, None):
        with pytest.raises(ValueError, match="^Tour: end must be 'open', 'return' or 'last'"):
            make(fig7(), [(0, 0), (0, 1)], end=end)


def test_before(no_engine):
    g, st = fig7(), [(0, 0), (0, 1), (0, 2), (0, 3)]
    for bad in ([(1, 4)], [(-1, 2)], [(1,)], [(1, 2, 3)], [(1.5, 2)], [(True, 2)]):
        with pytest.raises(ValueError, match=r"^Tour: before\[0\] = .* is no pair of stop indices in \[0, 4\)"):
            make(g, st, before=bad)
    with pytest.raises(ValueError, match="^Tour: before must be a list"):
        make(g, st, before=3)
    with pytest.raises(ValueError, match=r"^Tour: before\[1\] = \(2, 2\) puts a stop before itself"):
        make(g, st, before=[(1, 2), (2, 2)])
    with pytest.raises(ValueError, match=r"^Tour: before\[0\] = \(1, 0\) puts a stop before the start"):
        make(g, st, before=[(1, 0)])
    with pytest.raises(ValueError, match=r"^Tour: before\[0\] = \(3, 1\) puts the last stop of end='last' before another"):
        make(g, st, end="last", before=[(3, 1)])
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, st, end="open", before=[(3, 1), (0, 2)])


def test_cost_map(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^Tour: cost has shape"):
        make(g, [(0, 0)], cost=np.ones((20, 19)))
    c = np.ones((20, 20))
    free = np.argwhere(g != 1)[3]
    c[tuple(free)] = 0.5
    with pytest.raises(ValueError, match="^Tour: cost"):
        make(g, [(0, 0)], cost=c)


def test_solve_matrices_errors():
    from pathfit import Tour
    e = ModelEngine(fig7())
    with pytest.raises(ValueError, match="^Tour: mats has shape"):
        Tour.solve_matrices(e, np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="^Tour: 18 stops"):
        Tour.solve_matrices(e, np.zeros((1, 18, 18)))
    m = tc.matrix("asym", 4, 0)[None].repeat(3, 0)
    m[2, 1, 3] = -1.0
    with pytest.raises(ValueError, match=r"^Tour: mats\[2, 1, 3\] = -1.0 is neither"):
        Tour.solve_matrices(e, m)
    m[2, 1, 3] = np.nan
    with pytest.raises(ValueError, match=r"^Tour: mats\[2, 1, 3\] = nan"):
        Tour.solve_matrices(e, m)
    with pytest.raises(ValueError, match="^Tour: end must be"):
        Tour.solve_matrices(e, m, end="x")
    assert e.calls == []


# ---- the numpy side over the model engine
def test_the_facade_over_the_model():
    from pathfit import DistanceField  # noqa: F401  (the class the legs are documented against)
    g = fig7()
    e = ModelEngine(g)
    t = make(g, tc.NN_STOPS, engine=e)
    assert e.calls == ["dist_field_batch", "tour_matrix", "tour_solve"]
    assert t.feasible and t.total == 49.62741699796952 and list(t.order) == tc.held_karp(t.matrix, 0)[1]
    assert t.route_cost(t.order) == t.total
    assert t.route_cost(tc.nearest_neighbour(t.matrix, 0)) == 61.45584412271571
    assert t.route_cost([0]) == 0.0 and t.route_cost([]) == 0.0
    with pytest.raises(ValueError, match=r"^Tour: order\[1\] = 8 is outside \[0, 8\)"):
        t.route_cost([0, 8])
    legs = t.legs()
    assert e.calls[3:] == ["dist_field_parents", "dist_field_paths"] and len(legs) == 7
    C = g.shape[1]
    for leg, a, b in zip(legs, t.order[:-1], t.order[1:]):
        assert leg[0] == tc.NN_STOPS[a] and leg[-1] == tc.NN_STOPS[b]
    p = t.path()
    assert e.calls[5:] == ["dist_field_paths"]                        # the parent maps are kept
    assert len(p) == sum(len(leg) for leg in legs) - 6
    cells = p.cells
    assert all(max(abs(int(u) // C - int(v) // C), abs(int(u) % C - int(v) % C)) == 1 for u, v in zip(cells[:-1], cells[1:]))
    t.close()


def test_before_becomes_need_words_and_return_closes_the_route():
    g = fig7()
    e = ModelEngine(g)
    st = tc.NN_STOPS[:5]
    t = make(g, st, end="return", before=[(3, 1), (3, 2), (0, 4), (2, 1)], engine=e)
    assert e.need == [0, (1 << 3) | (1 << 2), 1 << 3, 0, 1]
    order = list(t.order)
    assert order.index(3) < order.index(2) < order.index(1)
    assert t.total == t.route_cost(order) == tc.route_cost(t.matrix, order, 1)
    legs = t.legs()
    assert len(legs) == 5 and legs[-1][-1] == st[0] and t.path()[0] == t.path()[-1] == st[0]
    cyc = make(g, st, before=[(1, 2), (2, 1)], engine=e)
    assert not cyc.feasible and cyc.total == tc.INF and list(cyc.order) == [-1] * 5 and cyc.legs() == [] and len(cyc.path()) == 0


def test_join_legs_skips_a_shared_cell_only():
    from pathfit.paths import CellPath
    from pathfit.tour import join_legs
    legs = [CellPath([1, 2, 3], 10), CellPath([3], 10), CellPath([3, 4], 10), CellPath([], 10), CellPath([4, 5], 10)]
    assert list(join_legs(legs, 10).cells) == [1, 2, 3, 4, 5]
    assert len(join_legs([], 10)) == 0


def test_a_cost_map_goes_through_pf_cost_field_and_refresh_recomputes():
    g = fig7()
    e = ModelEngine(g)
    cost = cc.cost_of_kind("u50", g.shape, 3)
    st = tc.NN_STOPS[:4]
    t = make(g, st, end="last", cost=cost, engine=e)
    assert e.calls == ["cost_field", "tour_matrix", "tour_solve"]
    ids = [r * 20 + c for r, c in st]
    want = cc.fields(g, cost, [[s] for s in ids], True, True)[0].reshape(4, -1)[:, ids]
    assert np.array_equal(t.matrix.view(np.int64), want.view(np.int64))
    assert list(t.order) == tc.held_karp(want, 2)[1] and t.order[-1] == 3
    g2 = g.copy()
    g2[g2 > 1] = 0
    wall = [tuple(c) for c in np.argwhere(g2 == 0) if tuple(c) not in st][:5]
    for r, c in wall:
        g2[r, c] = 1
    e.update_grid(g2)
    t.refresh()
    want2 = cc.fields(g2, cost, [[s] for s in ids], True, True)[0].reshape(4, -1)[:, ids]
    assert np.array_equal(t.matrix.view(np.int64), want2.view(np.int64))
    with pytest.raises(ValueError, match="^Tour: refresh\\(cost\\) needs a tour built with a cost map"):
        make(g, st, engine=ModelEngine(g)).refresh(cost=cost)


def test_solve_matrices_over_the_model():
    from pathfit import Tour
    e = ModelEngine(fig7())
    mats = np.array([tc.matrix(k, 6, 1) for k in tc.KINDS])
    tot, orders, status, info = Tour.solve_matrices(e, mats, end="last", before=[(2, 1)])
    assert e.need == [0, 4, 0, 0, 0, 0] and tot.shape == (5,) and orders.shape == (5, 6) and info.shape == (5, 4)
    for b in range(5):
        want = tc.held_karp(mats[b], 2, e.need)
        assert (tc.bits(tot[b]), list(orders[b]), int(info[b, 0]), int(info[b, 1])) == (tc.bits(want[0]), want[1], want[2], want[3])
        assert status[b] == (0 if want[0] < tc.INF else 1)
