"""CostField argument checks and Clearance.cost_map's numpy side: every ValueError comes before any Engine exists, and the facade's
host side runs over a model engine whose `cost_field` is the checker (runs on a CPU-only host)."""
import math

import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc
import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import cost_field

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(cost_field, "Engine", boom)


def make(g, cost, sets, **kw):
    from pathfit import CostField
    return CostField(g, cost, sets, **kw)


class HostBuf:
    def __init__(self, shape, dtype):
        self.a = np.zeros(int(np.prod(shape)), dtype)
        self.shape, self.freed = tuple(np.atleast_1d(shape)), False

    def upload(self, arr):
        self.a[:] = np.asarray(arr).reshape(-1)
        return self

    def download(self):
        return self.a.reshape(self.shape).copy()

    def free(self):
        self.freed = True


class ModelEngine:
    """An engine of the grid's shape whose `cost_field` is the heap checker; any other device call fails the test."""
    h = 1

    def __init__(self, g):
        self.R, self.C = g.shape
        self.grid_u8 = np.asarray(g, np.uint8)
        self.calls = 0

    def buf(self, shape, dtype):
        return HostBuf(shape, dtype)

    def put(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype)
        return HostBuf(a.shape, a.dtype).upload(a)

    def cost_field(self, d_cost, set_off, sources, d_out, allow_diag=True, restrict_corner=True, d_info=None):
        sets = [list(sources[set_off[b]:set_off[b + 1]]) for b in range(len(set_off) - 1)]
        D, _, info = ck.fields(self.grid_u8, d_cost.a.reshape(self.R, self.C), sets, allow_diag, restrict_corner)
        d_out.a[:] = D.reshape(-1)
        d_info.a[:] = info.reshape(-1)
        self.calls += 1

    def cost_field_work(self):
        return (1, 1, 1, 0)

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def fig7():
    g, _, _ = gio.grid("fig7")
    return g, np.ones(g.shape)


def test_the_inherited_checks_carry_the_class_name(no_engine):
    g, c = fig7()
    with pytest.raises(ValueError, match="^CostField: grid must be 2-D"):
        make(np.zeros(16, int), np.ones(16), [(0, 0)])
    with pytest.raises(ValueError, match="^CostField: source_sets is empty"):
        make(g, c, [])
    with pytest.raises(ValueError, match=r"^CostField: source_sets\[1\] is empty"):
        make(g, c, [[(0, 0)], []])
    with pytest.raises(ValueError, match="^CostField: source_sets must be a list of lists"):
        make(g, c, 5)
    with pytest.raises(ValueError, match=r"^CostField: source_sets\[0\]\[1\] = \(0, 20\) is outside the 20x20 grid"):
        make(g, c, [(0, 0), (0, 20)])
    with pytest.raises(ValueError, match=r"^CostField: source_sets\[0\]\[0\] must be an \(r, c\) pair"):
        make(g, c, [[7]])
    r, k = (int(v) for v in np.argwhere(g == 1)[0])
    with pytest.raises(ValueError, match=rf"^CostField: source_sets\[0\]\[0\] = \({r}, {k}\) is on an obstacle"):
        make(g, c, [[(r, k)]])

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^CostField: the engine's grid has another shape"):
        make(g, c, [(0, 0)], engine=Other())


@pytest.mark.parametrize("bad", ["abc", None, [[1.0, "x"]], object()])
def test_cost_must_be_numbers(no_engine, bad):
    g, _ = fig7()
    with pytest.raises(ValueError, match="^CostField: cost (must be an \\[R, C\\] array of numbers|has shape)"):
        make(g, bad, [(0, 0)])


@pytest.mark.parametrize("shape", [(20,), (20, 21), (21, 20), (400,), (1, 20, 20)])
def test_cost_shape(no_engine, shape):
    g, _ = fig7()
    with pytest.raises(ValueError, match=r"^CostField: cost has shape .*, the grid has \(20, 20\)"):
        make(g, np.ones(shape), [(0, 0)])


@pytest.mark.parametrize("v", [0.5, 0.0, -3.0, 2.0 ** 20 + 1, math.nan, math.inf, -math.inf])
def test_cost_range_on_a_free_cell(no_engine, v):
    g, c = fig7()
    r, k = (int(x) for x in np.argwhere(g != 1)[5])
    c[r, k] = v
    with pytest.raises(ValueError, match=rf"^CostField: cost\[{r}, {k}\] = .* on a free cell is not a finite number in \[1, 2\^20\]"):
        make(g, c, [(0, 0)])


def test_garbage_on_obstacles_and_the_bounds_themselves_are_accepted(no_engine):
    from pathfit.cost_field import checked_cost
    g, c = fig7()
    c[g == 1] = math.nan
    c.reshape(-1)[np.flatnonzero(g.reshape(-1) == 1)[1::2]] = -7.0
    c.reshape(-1)[np.flatnonzero(g.reshape(-1) != 1)[:2]] = [1.0, 2.0 ** 20]
    out = checked_cost("CostField", g, c)
    assert out.dtype == np.float64 and out is not c and np.array_equal(out, c, equal_nan=True)
    with pytest.raises(AssertionError, match="the device was touched"):           # every argument is fine: the device comes next
        make(g, c, [(0, 0)])
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, np.ones(g.shape, np.int32).tolist(), [[(0, 0)], [(19, 19)]], allow_diagonal_moves=False)


def test_the_facade_over_a_model_engine(no_engine):
    g, _ = fig7()
    cost = ck.cost_of_kind("u50", g.shape, 1)
    e = ModelEngine(g)
    f = make(g, cost, [[(0, 0)], [(19, 19), (0, 0)]], engine=e)
    want, _, winfo = ck.fields(g, cost, [[0], [399, 0]], True, True)
    assert e.calls == 1 and f.B == 2 and f.work == (1, 1, 1, 0)
    assert np.array_equal(f.fields, want) and np.array_equal(f.info, winfo) and f.info.dtype == np.int64
    assert f.length(1, (3, 3)) == want[1, 3, 3] and np.array_equal(f.reachable(0), np.isfinite(want[0]))
    assert np.array_equal(f.cost_device.a.reshape(g.shape), cost) and f.cost is not cost
    # refresh: a new cost map is checked first, then uploaded; a bad one changes nothing
    bad = cost.copy()
    bad[0, 0] = 0.25
    with pytest.raises(ValueError, match=r"^CostField: cost\[0, 0\] = 0.25 on a free cell"):
        f.refresh(cost=bad)
    with pytest.raises(ValueError, match="^CostField: cost has shape"):
        f.refresh(cost=np.ones((3, 3)))
    assert e.calls == 1 and np.array_equal(f.cost, cost) and np.array_equal(f.fields, want)
    cost2 = ck.cost_of_kind("int14", g.shape, 2)
    assert f.refresh(cost=cost2) is f and e.calls == 2
    assert np.array_equal(f.fields, ck.fields(g, cost2, [[0], [399, 0]], True, True)[0])
    # refresh after update_grid: the engine's map counts, and the held cost map is checked against it
    g2 = g.copy()
    wall = tuple(int(v) for v in np.argwhere(g == 1)[0])
    g2[wall] = 0
    cost2[wall] = math.nan                                                          # garbage under the old wall: a free cell now
    f.cost[wall] = math.nan
    e.grid_u8 = g2.astype(np.uint8)
    with pytest.raises(ValueError, match=rf"^CostField: cost\[{wall[0]}, {wall[1]}\] = nan on a free cell"):
        f.refresh()
    cost2[wall] = 2.0
    f.refresh(cost=cost2)
    assert e.calls == 3 and np.array_equal(f.fields, ck.fields(g2, cost2, [[0], [399, 0]], True, True)[0]) and f.grid[wall] == 0


@pytest.mark.parametrize("bad, msg", [
    (5, "paths must be a sequence of paths or a"),
    ([7], r"paths\[0\] must be a CellPath, a list of \(r, c\) pairs or an integer cell array"),
    ([[(0, 0), 3]], r"paths\[0\]\[1\] must be an \(r, c\) pair"),
])
def test_path_costs_arguments(no_engine, bad, msg):
    g, c = fig7()
    f = make(g, c, [(0, 0)], engine=ModelEngine(g))
    with pytest.raises(ValueError, match="^CostField: " + msg):
        f.path_costs(bad)
    from pathfit.paths import CellPath
    with pytest.raises(ValueError, match=r"^CostField: paths\[0\] belongs to a grid of 7 columns, not 20"):
        f.path_costs([CellPath(np.array([0, 1], np.int32), 7)])
    tot, bad_at = f.path_costs([])
    assert tot.shape == (0,) and tot.dtype == np.float64 and bad_at.shape == (0,) and bad_at.dtype == np.int32


# ---- Clearance.cost_map's numpy side
def cost_map(d2, grid, **kw):
    from pathfit.clearance import cost_map_of
    return cost_map_of(d2, grid, **kw)


@pytest.mark.parametrize("kw, msg", [
    ({}, "give exactly one of margin and margin_sq"),
    ({"margin": 2.0, "margin_sq": 4}, "give exactly one of margin and margin_sq"),
    ({"margin": 0}, r"margin must be a number in \(0, 46340\)"),
    ({"margin": -1.5}, r"margin must be a number in \(0, 46340\)"),
    ({"margin": "wide"}, r"margin must be a number in \(0, 46340\)"),
    ({"margin": True}, r"margin must be a number in \(0, 46340\)"),
    ({"margin": math.nan}, r"margin must be a number in \(0, 46340\)"),
    ({"margin_sq": 0}, r"margin_sq must be an integer in \[1, 2\^31 - 1\]"),
    ({"margin_sq": 2.5}, r"margin_sq must be an integer in \[1, 2\^31 - 1\]"),
    ({"margin": 2.0, "weight": -1.0}, "weight must be a finite number >= 0"),
    ({"margin": 2.0, "weight": math.inf}, "weight must be a finite number >= 0"),
    ({"margin": 2.0, "weight": "heavy"}, "weight must be a finite number >= 0"),
    ({"margin": 2.0, "weight": False}, "weight must be a finite number >= 0"),
])
def test_cost_map_arguments(kw, msg):
    d2 = np.ones((3, 4), np.int32)
    with pytest.raises(ValueError, match="^Clearance: " + msg):
        cost_map(d2, np.zeros((3, 4), int), **kw)
    with pytest.raises(ValueError, match="^Clearance: the field has shape"):
        cost_map(np.ones((3, 5), np.int32), np.zeros((3, 4), int), margin=2.0)


def test_cost_map_values():
    import clearance_checkers as clk
    g, _, _ = gio.grid("img1")
    d2 = clk.brute_force(g, False)[0]
    for kw, m in (({"margin": 4}, 4.0), ({"margin": 2.5, "weight": 3.0}, 2.5), ({"margin_sq": 10, "weight": 0.5}, math.sqrt(10)),
                  ({"margin": 3.0, "weight": 0.0}, 3.0), ({"margin": 40000.0, "weight": 1e6}, 40000.0)):
        w = float(kw.get("weight", 1.0))
        c = cost_map(d2, g, **kw)
        assert c.dtype == np.float64 and c.shape == g.shape
        for r in range(g.shape[0]):
            for k in range(g.shape[1]):
                want = 1.0 if g[r, k] == 1 else min(1.0 + w * max(0.0, m - math.sqrt(float(d2[r, k]))) ** 2, float(2 ** 20))
                assert c[r, k] == want, (kw, r, k)
        assert c.min() >= 1.0 and c.max() <= 2.0 ** 20 and np.all(c[g == 1] == 1.0)
        from pathfit.cost_field import checked_cost
        checked_cost("CostField", g, c)                                             # always a legal cost map
    assert cost_map(d2, g, margin=40000.0, weight=1e6).max() == 2.0 ** 20           # clipped
    far = d2 >= 16
    assert np.all(cost_map(d2, g, margin=4)[far] == 1.0) and (cost_map(d2, g, margin=4)[~far & (g != 1)] > 1.0).all()
    z = np.zeros((3, 4), int)                                                       # a map without obstacles: 1 everywhere
    assert np.all(cost_map(np.full((3, 4), 2 ** 31 - 1, np.int32), z, margin=4) == 1.0)
    assert fc.SQRT2 == math.sqrt(2.0)
