"""TurnField argument checks: every ValueError comes before any Engine exists and starts with the class name, and the facade's host
side runs over a model engine whose `turn_field` is the checker (runs on a CPU-only host)."""
import math

import numpy as np
import pytest

import cost_checkers as ck
import golden_io as gio
import turn_checkers as tk


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import turn_field

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(turn_field, "Engine", boom)


def make(g, sets, wt, **kw):
    from pathfit import TurnField
    return TurnField(g, sets, wt, **kw)


class HostBuf:
    def __init__(self, shape, dtype):
        self.a = np.zeros(int(np.prod(shape)), dtype)
        self.shape, self.freed = tuple(np.atleast_1d(shape)), False

    def upload(self, arr):
        self.a[:] = np.asarray(arr).reshape(-1)
        return self

    def download(self):
        return self.a.reshape(self.shape).copy()

    def read(self, at, n):
        return self.a[at:at + n].copy()

    def free(self):
        self.freed = True


class ModelEngine:
    """An engine of the grid's shape whose `turn_field` is the heap checker; any other device call fails the test."""
    h = 1

    def __init__(self, g):
        self.R, self.C = g.shape
        self.grid_u8 = np.asarray(g, np.uint8)
        self.calls, self.bufs = 0, []

    def buf(self, shape, dtype):
        self.bufs.append(HostBuf(shape, dtype))
        return self.bufs[-1]

    def put(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype)
        self.bufs.append(HostBuf(a.shape, a.dtype).upload(a))
        return self.bufs[-1]

    def turn_field(self, d_cost, turn_weight, set_off, sources, d_states, d_best, allow_diag=True, restrict_corner=True, d_info=None):
        sets = [list(sources[set_off[b]:set_off[b + 1]]) for b in range(len(set_off) - 1)]
        cost = None if d_cost is None else d_cost.a.reshape(self.R, self.C)
        T, best, info = tk.fields(self.grid_u8, cost, sets, turn_weight, allow_diag, restrict_corner)
        d_states.a[:], d_best.a[:], d_info.a[:] = T.reshape(-1), best.reshape(-1), info.reshape(-1)
        self.calls += 1

    def turn_field_work(self):
        return (1, 1, 1, 0)

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def fig7():
    return gio.grid("fig7")[0]


def test_the_shared_checks_carry_the_class_name(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^TurnField: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)], 0.3)
    with pytest.raises(ValueError, match="^TurnField: source_sets is empty"):
        make(g, [], 0.3)
    with pytest.raises(ValueError, match=r"^TurnField: source_sets\[1\] is empty"):
        make(g, [[(0, 0)], []], 0.3)
    with pytest.raises(ValueError, match="^TurnField: source_sets must be a list of lists"):
        make(g, 5, 0.3)
    with pytest.raises(ValueError, match=r"^TurnField: source_sets\[0\]\[1\] = \(0, 20\) is outside the 20x20 grid"):
        make(g, [(0, 0), (0, 20)], 0.3)
    with pytest.raises(ValueError, match=r"^TurnField: source_sets\[0\]\[0\] must be an \(r, c\) pair"):
        make(g, [[7]], 0.3)
    r, k = (int(v) for v in np.argwhere(g == 1)[0])
    with pytest.raises(ValueError, match=rf"^TurnField: source_sets\[0\]\[0\] = \({r}, {k}\) is on an obstacle"):
        make(g, [[(r, k)]], 0.3)

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^TurnField: the engine's grid has another shape"):
        make(g, [(0, 0)], 0.3, engine=Other())


@pytest.mark.parametrize("wt", [-0.5, -0.0 - 1e-300, 2.0 ** 20 + 1, math.nan, math.inf, -math.inf, "0.3", None, True, [0.3], 1j])
def test_turn_weight_range(no_engine, wt):
    with pytest.raises(ValueError, match=r"^TurnField: turn_weight must be a finite number in \[0, 2\^20\], got"):
        make(fig7(), [(0, 0)], wt)


@pytest.mark.parametrize("bad, msg", [
    ("abc", "cost must be an \\[R, C\\] array of numbers|cost has shape"),
    (np.ones((20, 21)), r"cost has shape \(20, 21\), the grid has \(20, 20\)"),
])
def test_cost_checks_are_cost_fields(no_engine, bad, msg):
    with pytest.raises(ValueError, match="^TurnField: (" + msg + ")"):
        make(fig7(), [(0, 0)], 0.3, cost=bad)
    g = fig7()
    c = np.ones(g.shape)
    r, k = (int(x) for x in np.argwhere(g != 1)[5])
    for v in (0.5, 2.0 ** 20 + 1, math.nan, math.inf):
        c[r, k] = v
        with pytest.raises(ValueError, match=rf"^TurnField: cost\[{r}, {k}\] = .* on a free cell is not a finite number in \[1, 2\^20\]"):
            make(g, [(0, 0)], 0.3, cost=c)


def test_good_arguments_reach_the_device(no_engine):
    g = fig7()
    for wt in (0, 0.0, 0.3, np.float32(3.0), np.int64(7), 2 ** 20):
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, [(0, 0)], wt)
    junk = np.ones(g.shape)
    junk[g == 1] = math.nan                                                         # garbage under obstacles is not looked at
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, [[(0, 0)], [(19, 19)]], 0.3, cost=junk, allow_diagonal_moves=False)


def test_the_facade_over_a_model_engine(no_engine):
    g = fig7()
    cost = ck.cost_of_kind("u50", g.shape, 1)
    e = ModelEngine(g)
    f = make(g, [[(0, 0)], [(19, 19), (0, 0)]], 0.3, cost=cost, engine=e)
    sets = [[0], [399, 0]]
    T, best, info = tk.fields(g, cost, sets, 0.3, True, True)
    assert e.calls == 1 and f.B == 2 and f.work == (1, 1, 1, 0) and f.turn_weight == 0.3
    assert np.array_equal(f.states, T) and f.states.shape == (2, 8, 20, 20) and np.array_equal(f.best, best) and f.best.shape == (2, 20, 20)
    assert np.array_equal(f.info, info) and f.info.dtype == np.int64 and f.cost is not cost
    for cell in ((3, 3), (19, 19), (0, 0), tuple(int(v) for v in np.argwhere(g == 1)[0])):
        col = T[1][:, cell[0], cell[1]]
        assert f.heading(1, cell) == (int(np.argmin(col)) if np.isfinite(col.min()) else None)
    f2 = make(g, [(0, 0)], 0.3, engine=ModelEngine(g))                               # no cost map: no cost buffer
    assert f2.cost is None and f2.cost_device is None and np.array_equal(f2.best, tk.fields(g, None, [[0]], 0.3, True, True)[1])
    assert f2.heading(0, (5, 5)) == int(np.argmin(f2.states[0][:, 5, 5]))
    # the index and cell checks of the queries
    with pytest.raises(ValueError, match=r"^TurnField: b = 2 is outside \[0, 2\)"):
        f.heading(2, (0, 0))
    with pytest.raises(ValueError, match=r"^TurnField: cell = \(0, 20\) is outside the 20x20 grid"):
        f.heading(0, (0, 20))
    with pytest.raises(ValueError, match=r"^TurnField: targets\[1\] must be an \(r, c\) pair"):
        f.paths([(0, 0), 5])
    with pytest.raises(ValueError, match=r"^TurnField: b = -1 is outside \[0, 2\)"):
        f.paths([(0, 0)], b=-1)
    with pytest.raises(ValueError, match="^TurnField: path_cap must be >= 1"):
        f.paths([(0, 0)], path_cap=0)
    assert f.paths([]) == []
    # refresh: new arguments are checked first; a bad one changes nothing
    bad = cost.copy()
    bad[0, 0] = 0.25
    with pytest.raises(ValueError, match=r"^TurnField: cost\[0, 0\] = 0.25 on a free cell"):
        f.refresh(cost=bad)
    with pytest.raises(ValueError, match="^TurnField: turn_weight must be a finite number"):
        f.refresh(turn_weight=-1.0)
    with pytest.raises(ValueError, match="^TurnField: turn_weight must be a finite number"):
        f.refresh(cost=ck.cost_of_kind("int14", g.shape, 2), turn_weight=math.nan)
    assert e.calls == 1 and np.array_equal(f.cost, cost) and f.turn_weight == 0.3 and np.array_equal(f.best, best)
    cost2 = ck.cost_of_kind("int14", g.shape, 2)
    assert f.refresh(cost=cost2, turn_weight=3.0) is f and e.calls == 2 and f.turn_weight == 3.0
    assert np.array_equal(f.states, tk.fields(g, cost2, sets, 3.0, True, True)[0])
    assert f2.refresh(cost=cost2).cost_device is not None and np.array_equal(f2.best[0], tk.fields(g, cost2, [[0]], 0.3, True, True)[1][0])
    # refresh after update_grid: the engine's map counts, and the held cost map is checked against it
    g2 = g.copy()
    wall = tuple(int(v) for v in np.argwhere(g == 1)[0])
    g2[wall] = 0
    f.cost[wall] = math.nan
    e.grid_u8 = g2.astype(np.uint8)
    with pytest.raises(ValueError, match=rf"^TurnField: cost\[{wall[0]}, {wall[1]}\] = nan on a free cell"):
        f.refresh()
    cost2[wall] = 2.0
    f.refresh(cost=cost2)
    assert e.calls == 3 and np.array_equal(f.best, tk.fields(g2, cost2, sets, 3.0, True, True)[1]) and f.grid[wall] == 0
    f.close()
    assert f.sbuf is None and f.bbuf is None and all(b.freed for b in e.bufs)
    from pathfit import PathfitError
    with pytest.raises(PathfitError, match="^TurnField: the field is closed"):
        f.refresh()
    assert np.array_equal(f.best[1], tk.fields(g2, cost2, sets, 3.0, True, True)[1][1])      # what was downloaded stays


@pytest.mark.parametrize("bad, msg", [
    (5, "paths must be a sequence of paths or a"),
    ([7], r"paths\[0\] must be a CellPath, a list of \(r, c\) pairs or an integer cell array"),
    ([[(0, 0), 3]], r"paths\[0\]\[1\] must be an \(r, c\) pair"),
])
def test_path_costs_arguments(no_engine, bad, msg):
    g = fig7()
    f = make(g, [(0, 0)], 0.3, engine=ModelEngine(g))
    with pytest.raises(ValueError, match="^TurnField: " + msg):
        f.path_costs(bad)
    from pathfit.paths import CellPath
    with pytest.raises(ValueError, match=r"^TurnField: paths\[0\] belongs to a grid of 7 columns, not 20"):
        f.path_costs([CellPath(np.array([0, 1], np.int32), 7)])
    from pathfit.engine import DevBuf
    dev = object.__new__(DevBuf)
    dev.ptr = 0                                                                     # (never allocated: nothing to free)
    with pytest.raises(ValueError, match=r"^TurnField: path_costs needs n >= 1 and path_cap >= 1 for device rows"):
        f.path_costs((dev, dev, 0, 4))
    tot, turns, bad_at = f.path_costs([])
    assert tot.shape == (0,) and tot.dtype == np.float64 and turns.shape == (0,) and turns.dtype == np.int32 and bad_at.dtype == np.int32
