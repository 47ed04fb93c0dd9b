"""Visibility argument checks: ValueError before any device is touched, and the numpy side of cost_map (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio
import visibility_checkers as vc


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import visibility

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(visibility, "Engine", boom)


class HostBuf:
    def __init__(self, n, dtype):
        self.a = np.zeros(n, dtype)

    def download(self):
        return self.a.copy()

    def free(self):
        pass


class ModelEngine:
    """An engine of the grid's shape whose visibility calls are the model; every device call fails the test when `sealed`."""
    h = 1

    def __init__(self, g):
        self.g, (self.R, self.C) = g, g.shape
        self.grid_u8 = np.asarray(g, np.uint8)
        self.sealed = False

    def buf(self, n, dtype):
        assert not self.sealed, "the device was touched before the arguments were checked (buf)"
        return HostBuf(n, dtype)

    def visibility_count(self, view, d_count, strict, rsq, d_info):
        assert not self.sealed, "the device was touched before the arguments were checked (visibility_count)"
        occ = vc.occ_of(self.g)
        counts = vc.exposure(occ, [(int(v) // self.C, int(v) % self.C) for v in view], strict, rsq)
        d_count.a[:] = counts.reshape(-1)
        d_info.a[:] = vc.count_info(occ, counts)

    def visibility_field(self, view, d_seen, strict, rsq, d_info):
        assert not self.sealed, "the device was touched before the arguments were checked (visibility_field)"
        occ = vc.occ_of(self.g)
        for k, v in enumerate(view):
            a = (int(v) // self.C, int(v) % self.C)
            m = vc.seen_map(occ, a, strict, rsq)
            d_seen.a[k * m.size:(k + 1) * m.size] = m.reshape(-1)
            d_info.a[4 * k:4 * k + 4] = vc.field_info(m, a)

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def make(g, **kw):
    from pathfit import Visibility
    return Visibility(g, **kw)


def test_grid_must_be_2d(no_engine):
    for g in (np.zeros(16, int), np.zeros((2, 2, 2), int)):
        with pytest.raises(ValueError, match="^Visibility: grid must be 2-D"):
            make(g)


def test_engine_of_another_shape(no_engine):
    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^Visibility: the engine's grid has another shape"):
        make(gio.grid("fig7")[0], engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    with pytest.raises(AssertionError, match="the device was touched"):
        make(gio.grid("fig7")[0])


@pytest.fixture
def vis(no_engine):
    g, _, _ = gio.grid("img1")
    e = ModelEngine(g)
    v = make(g, engine=e)
    e.sealed = True
    return v


CALLS = [lambda v, *a: v.seen(*a), lambda v, *a: v.exposure(*a), lambda v, *a: v.exposure_device(*a), lambda v, *a: v.cost_map(a[0], 1.0, *a[1:])]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("bad, msg", [
    ([], "viewpoints is empty"), (5, "viewpoints must be a list"), ("ab", "viewpoints must be a list"),
    ([(0, 0), (20, 0)], r"viewpoints\[1\] = \(20, 0\) is outside the 20x20 grid"), ([(0, -1)], r"viewpoints\[0\] = \(0, -1\) is outside"),
    ([(0, 0, 0)], r"viewpoints\[0\] must be an \(r, c\) pair"), ([3], r"viewpoints\[0\] must be an \(r, c\) pair"),
])
def test_viewpoints(vis, call, bad, msg):
    with pytest.raises(ValueError, match="^Visibility: " + msg):
        call(vis, bad)


def test_a_cell_path_of_another_grid_or_outside(vis):
    from pathfit import CellPath
    with pytest.raises(ValueError, match="^Visibility: viewpoints belongs to a grid of 21 columns, not 20"):
        vis.exposure(CellPath(np.array([0, 1], np.int32), 21))
    with pytest.raises(ValueError, match=r"^Visibility: viewpoints\[1\] = cell 400 is outside the 20x20 grid"):
        vis.seen(CellPath(np.array([0, 400], np.int32), 20))


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("bad", [-1, -0.5, float("nan"), float("inf"), "a", True, [1]])
def test_max_range(vis, call, bad):
    with pytest.raises(ValueError, match="^Visibility: max_range must be None or a finite number >= 0"):
        call(vis, [(0, 0)], bad)


def test_range_to_sq_is_exact_for_integers_and_half_integers():
    from fractions import Fraction

    from pathfit.visibility import range_to_sq
    assert range_to_sq(None) == -1 and range_to_sq(0) == 0 and range_to_sq(0.5) == 0 and range_to_sq(1) == 1
    for n in (1, 2, 5, 7, 1000, 4095, 46340):
        assert range_to_sq(n) == n * n and range_to_sq(float(n)) == n * n
        assert range_to_sq(n + 0.5) == n * n + n and range_to_sq(Fraction(2 * n + 1, 2)) == n * n + n
    assert range_to_sq(np.sqrt(2.0)) == 2 and range_to_sq(1.4142135) == 1                  # fl(sqrt 2)^2 > 2
    assert range_to_sq(1e9) == 2 ** 31 - 2 and range_to_sq(np.int64(3)) == 9


@pytest.mark.parametrize("bad", [-1, -1e-9, float("nan"), float("inf"), "w", None, True])
def test_cost_map_weight(vis, bad):
    with pytest.raises(ValueError, match="^Visibility: weight must be a finite number >= 0"):
        vis.cost_map([(0, 0)], bad)


def test_path_exposure_arguments(vis):
    with pytest.raises(ValueError, match="^Visibility: path_exposure needs counts, or an exposure call before it"):
        vis.path_exposure([[(0, 0)]])
    ok = np.zeros((20, 20), np.int32)
    for bad, msg in [(5, "paths must be a sequence of paths"), ([5], r"paths\[0\] must be a CellPath"), ([[(0, 20)]], r"paths\[0\]\[0\] = \(0, 20\) is outside"),
                     ([np.array([0, 400])], r"paths\[0\]\[1\] = cell 400 is outside the 20x20 grid")]:
        with pytest.raises(ValueError, match="^Visibility: " + msg):
            vis.path_exposure(bad, ok)
    for bad in (np.zeros((20, 21), np.int32), np.zeros((20, 20), np.float64), np.zeros(400, np.int32)):
        with pytest.raises(ValueError, match="^Visibility: counts must be an integer array of shape"):
            vis.path_exposure([[(0, 0)]], bad)
    out = vis.path_exposure([], ok)
    assert len(out) == 4 and all(len(o) == 0 for o in out) and len(vis.status) == 0


def test_a_grid_beyond_the_integer_range(no_engine):
    with pytest.raises(ValueError, match=r"^Visibility: R\^2 \+ C\^2 must stay below 2\^31 - 1"):
        make(np.zeros((46341, 1), np.uint8))                           # 46341^2 + 1 > 2^31 - 1


def test_closed(no_engine):
    from pathfit import PathfitError
    g, _, _ = gio.grid("img1")
    v = make(g, engine=ModelEngine(g))
    v.close()
    with pytest.raises(PathfitError, match="^Visibility: the field is closed"):
        v.seen([(0, 0)])


# ---- the numpy side over the model engine
def test_exposure_and_cost_map_over_the_model(no_engine):
    from pathfit.visibility import cost_map_of
    g, _, _ = gio.grid("img1")
    occ = vc.occ_of(g)
    v = make(g, engine=ModelEngine(g))
    free = [tuple(int(x) for x in p) for p in np.argwhere(occ != 1)[[0, 40, 40, 200]]]
    exp = v.exposure(free)
    assert exp.dtype == np.int32 and np.array_equal(exp, vc.exposure(occ, free, True))
    assert v.coverage == pytest.approx(((exp > 0) & (occ != 1)).sum() / (occ != 1).sum()) and list(v.info) == vc.count_info(occ, exp)
    cm = v.cost_map(free, 2.5)
    assert cm.dtype == np.float64 and np.array_equal(cm, np.where(occ != 1, 1.0 + 2.5 * exp, 1.0)) and cm.min() == 1.0
    assert np.array_equal(v.cost_map(free, 0), np.ones((20, 20)))
    m = v.seen(free[:2], max_range=3.5)
    assert m.dtype == bool and m.shape == (2, 20, 20) and np.array_equal(m[0], vc.seen_map(occ, free[0], True, 12)) and v.info.shape == (2, 4)
    # the bound of CostField: 1 + w * exposure must stay within [1, 2^20] on the free cells
    top = int(exp.max())
    assert np.array_equal(cost_map_of(exp, g, (2 ** 20 - 1) / top), v.cost_map(free, (2 ** 20 - 1) / top))
    with pytest.raises(ValueError, match=r"^Visibility: the cost of the free cell \(\d+, \d+\), 1 \+ .* leaves \[1, 2\^20\]"):
        v.cost_map(free, 2 ** 20 / top)
    with pytest.raises(ValueError, match="^Visibility: the exposure map has shape"):
        cost_map_of(exp[:, :19], g, 1.0)
    on_wall = np.where(occ == 1, 10 ** 9, 0)
    assert np.array_equal(cost_map_of(on_wall, g, 1.0), np.ones((20, 20)))      # counts on obstacles are never looked at
