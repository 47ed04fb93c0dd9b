"""Clearance argument checks: ValueError before any device is touched (runs on a CPU-only host)."""
import numpy as np
import pytest

import clearance_checkers as ck
import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import clearance

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(clearance, "Engine", boom)


class HostBuf:
    def __init__(self, n, dtype):
        self.a = np.zeros(n, dtype)

    def download(self):
        return self.a.copy()

    def free(self):
        pass


class ModelEngine:
    """An engine of the grid's shape whose `clearance_field` is the model; every later device call fails the test when `sealed`."""
    h = 1

    def __init__(self, g):
        self.g, (self.R, self.C) = g, g.shape
        self.grid_u8 = np.asarray(g, np.uint8)
        self.sealed, self.calls = False, 0

    def buf(self, n, dtype):
        assert not self.sealed, "the device was touched before the arguments were checked (buf)"
        return HostBuf(n, dtype)

    def clearance_field(self, d_d2, border, d_near, d_info):
        assert not self.sealed, "the device was touched before the arguments were checked (clearance_field)"
        d2, near, info = ck.brute_force(self.g, border)
        d_d2.a[:] = d2.reshape(-1)
        if d_near is not None:
            d_near.a[:] = near.reshape(-1)
        d_info.a[:] = info
        self.calls += 1

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def make(g, **kw):
    from pathfit import Clearance
    return Clearance(g, **kw)


def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^Clearance: grid must be 2-D"):
        make(np.zeros(16, int))
    with pytest.raises(ValueError, match="^Clearance: grid must be 2-D"):
        make(np.zeros((2, 2, 2), int))


def test_engine_of_another_shape(no_engine):
    g, _, _ = gio.grid("fig7")

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^Clearance: the engine's grid has another shape"):
        make(g, engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, border=True, nearest=True)


@pytest.fixture
def img1(no_engine):
    g, _, _ = gio.grid("img1")
    e = ModelEngine(g)
    cl = make(g, engine=e)
    assert e.calls == 1 and cl.obstacle_cells + cl.free_cells == 400 and cl.obstacle_cells == int((g == 1).sum())
    e.sealed = True
    return cl


@pytest.mark.parametrize("kw", [{}, {"margin": 1.5, "margin_sq": 3}])
def test_exactly_one_margin(img1, kw):
    for call in (lambda: img1.inflated(**kw), lambda: img1.path_clearance([[(0, 0)]], **kw),
                 lambda: img1.path_clearance_device(None, None, 1, 4, **kw)):
        with pytest.raises(ValueError, match="^Clearance: give exactly one of margin and margin_sq"):
            call()


@pytest.mark.parametrize("bad", [0, -1, 1.5, "a", True, 2 ** 31, [1]])
def test_inflated_margin_sq(img1, bad):
    with pytest.raises(ValueError, match=r"^Clearance: margin_sq must be an integer in \[1, 2\^31 - 1\]"):
        img1.inflated(margin_sq=bad)


@pytest.mark.parametrize("bad", [-1, 1.5, "a", False, 2 ** 31])
def test_path_margin_sq(img1, bad):
    with pytest.raises(ValueError, match=r"^Clearance: margin_sq must be an integer in \[0, 2\^31 - 1\]"):
        img1.path_clearance([[(0, 0)]], margin_sq=bad)
    with pytest.raises(ValueError, match=r"^Clearance: margin_sq must be an integer in \[0, 2\^31 - 1\]"):
        img1.path_clearance_device(None, None, 1, 4, margin_sq=bad)


@pytest.mark.parametrize("bad", [0, 0.0, -2.0, float("nan"), float("inf"), 46340.0, "x", True, [1.5]])
def test_margin_must_be_a_positive_number(img1, bad):
    with pytest.raises(ValueError, match=r"^Clearance: margin must be a number in \(0, 46340\)"):
        img1.inflated(margin=bad)
    with pytest.raises(ValueError, match=r"^Clearance: margin must be a number in \(0, 46340\)"):
        img1.path_clearance([[(0, 0)]], margin=bad)


def test_inflated_runs_on_the_host(img1):
    g = img1.grid
    d2 = ck.brute_force(g)[0]
    assert np.array_equal(img1.d2, d2)
    assert np.array_equal(img1.inflated(margin_sq=1) == 1, g == 1) and np.array_equal(img1.inflated(margin_sq=1), g)
    for m in (1.5, 1.8, 3):
        want = ck.inflated(g, d2, ck.margin_sq(m))
        got = img1.inflated(margin=m)
        assert np.array_equal(got, want) and got.dtype == g.dtype
        assert set(np.unique(got[d2 >= ck.margin_sq(m)])) <= {0, 2, 3} and np.all(got[d2 < ck.margin_sq(m)] == 1)
    assert np.array_equal(img1.inflated(margin_sq=4), img1.inflated(margin=1.8))
    s = np.argwhere(g == 2)[0]
    assert img1.inflated(margin_sq=2 ** 31 - 1)[s[0], s[1]] == 1      # a marker on a blocked cell becomes 1
    assert np.array_equal(img1.distance, np.sqrt(d2.astype(np.float64)))
    v = int(img1.info[3])
    assert img1.most_open == ((v // 20, v % 20), int(d2.max())) and d2.reshape(-1)[v] == d2.max()


def test_nearest_must_be_asked_for(img1):
    import pathfit
    with pytest.raises(pathfit.PathfitError, match="Clearance: the nearest obstacles were not asked for"):
        img1.nearest
    g = img1.grid
    cl = make(g, nearest=True, border=True, engine=ModelEngine(g))
    want = ck.brute_force(g, True)
    assert np.array_equal(cl.nearest, want[1]) and np.array_equal(cl.d2, want[0])


def test_distance_is_inf_without_an_obstacle(no_engine):
    g = np.zeros((3, 4), int)
    cl = make(g, engine=ModelEngine(g))
    assert np.all(cl.d2 == ck.NONE) and np.all(np.isinf(cl.distance)) and cl.most_open == ((0, 0), ck.NONE)
    g = np.ones((3, 4), int)
    assert make(g, engine=ModelEngine(g)).most_open == (None, -1)


@pytest.mark.parametrize("bad, msg", [
    (5, "paths must be a sequence of paths"),
    ([7], r"paths\[0\] must be a CellPath, a list of \(r, c\) pairs or an int32 cell array"),
    ([[(0, 0), (1, 2, 3)]], r"paths\[0\]\[1\] must be an \(r, c\) pair"),
    ([[(0, 0)], [(0, 20)]], r"paths\[1\]\[0\] = \(0, 20\) is outside the 20x20 grid"),
    ([np.array([0, 400], np.int32)], r"paths\[0\]\[1\] = cell 400 is outside the 20x20 grid"),
    ([np.array([-1], np.int32)], r"paths\[0\]\[0\] = cell -1 is outside the 20x20 grid"),
])
def test_path_rows(img1, bad, msg):
    with pytest.raises(ValueError, match="^Clearance: " + msg):
        img1.path_clearance(bad, margin=1.5)


def test_path_of_another_grid(img1):
    from pathfit.paths import CellPath
    with pytest.raises(ValueError, match=r"^Clearance: paths\[0\] belongs to a grid of 21 columns, not 20"):
        img1.path_clearance([CellPath(np.array([0, 1], np.int32), 21)], margin=1.5)


@pytest.mark.parametrize("n, cap", [(0, 4), (-1, 4), (1, 0)])
def test_device_rows_need_a_size(img1, n, cap):
    with pytest.raises(ValueError, match="^Clearance: path_clearance_device needs n >= 1 and path_cap >= 1"):
        img1.path_clearance_device(None, None, n, cap, margin=1.5)


@pytest.mark.parametrize("bad, msg", [
    (5, "pairs must be a list"),
    ([7], r"pairs\[0\] must be two \(r, c\) pairs"),
    ([((0, 0),)], r"pairs\[0\] must be two \(r, c\) pairs"),
    (["ab"], r"pairs\[0\] must be two \(r, c\) pairs"),
    ([((0, 0), (1, 1)), ((0, 0), 7)], r"pairs\[1\]\[1\] must be an \(r, c\) pair"),
])
def test_segment_pairs(img1, bad, msg):
    with pytest.raises(ValueError, match="^Clearance: " + msg):
        img1.segment_clearance(bad)


def test_checked_calls_reach_the_device(img1):
    with pytest.raises(AssertionError, match="the device was touched"):
        img1.path_clearance([[(0, 0), (1, 1)]], margin=1.5)
    with pytest.raises(AssertionError, match="the device was touched"):
        img1.path_clearance([[]], margin_sq=0)                        # an empty path is an answer (status 1), no error
    with pytest.raises(AssertionError, match="the device was touched"):
        img1.path_clearance_device(None, None, 1, 4, margin_sq=0)
    with pytest.raises(AssertionError, match="the device was touched"):
        img1.segment_clearance([((0, 0), (3, 40))])                  # a cell beside the grid is an answer, no error
    out, st = img1.path_clearance([], margin=2)
    assert out.shape == (0, 4) and len(st) == 0
    dmin, at = img1.segment_clearance([])
    assert len(dmin) == 0 and at == []


def test_closed_field():
    import pathfit
    g = np.zeros((3, 4), int)
    g[1, 1] = 1
    cl = make(g, engine=ModelEngine(g))
    first = cl.d2
    cl.close()
    assert cl.d2 is first                                             # what was downloaded stays readable
    for call in (cl.refresh, lambda: cl.path_clearance([[(0, 0)]], margin=1.5), lambda: cl.segment_clearance([((0, 0), (1, 1))]),
                 lambda: cl.path_clearance_device(None, None, 1, 4, margin=1.5)):
        with pytest.raises(pathfit.PathfitError, match="Clearance: the field is closed"):
            call()
