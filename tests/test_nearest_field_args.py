"""NearestSourceField argument checks: ValueError before any Engine exists (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import nearest_field

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(nearest_field, "Engine", boom)


def make(g, sets, **kw):
    from pathfit import NearestSourceField
    return NearestSourceField(g, sets, **kw)


class FakeBuf:
    ptr = 1

    def free(self):
        pass


class FakeEngine:
    """An engine that records its calls and computes nothing: the checks of paths / nearest / next_hop come before any of them."""
    R, C, h = 20, 20, 1

    def __init__(self):
        self.calls = []

    def buf(self, shape, dtype):
        return FakeBuf()

    def dist_field_merged(self, *a):
        self.calls.append("merged")

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


@pytest.fixture
def field():
    g, _, _ = gio.grid("fig7")
    e = FakeEngine()
    f = make(g, [[(0, 0), (19, 19)], [(0, 19)]], engine=e)
    assert e.calls == ["merged"] and f.B == 2 and f.set_off.tolist() == [0, 2, 3] and f.ids.tolist() == [0, 399, 19]
    return f


def test_empty_set_list(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^NearestSourceField: source_sets is empty"):
        make(g, [])


def test_an_empty_set(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=r"^NearestSourceField: source_sets\[1\] is empty"):
        make(g, [[(0, 0)], []])


@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3)])
def test_out_of_range(no_engine, cell):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=r"^NearestSourceField: source_sets\[1\]\[1\] = .* is outside the 20x20 grid"):
        make(g, [[(0, 0)], [(0, 0), cell]])
    with pytest.raises(ValueError, match=r"^NearestSourceField: source_sets\[0\]\[1\] = .* is outside the 20x20 grid"):
        make(g, [(0, 0), cell])                                       # one flat list of pairs is one set


def test_on_an_obstacle(no_engine):
    g, _, _ = gio.grid("fig7")
    r, c = (int(v) for v in np.argwhere(np.asarray(g) == 1)[0])
    with pytest.raises(ValueError, match=rf"^NearestSourceField: source_sets\[0\]\[1\] = \({r}, {c}\) is on an obstacle"):
        make(g, [[(0, 0), (r, c)]])


@pytest.mark.parametrize("bad", [[[7]], [[(1, 2, 3)]], [["ab", (0, 0)]], [[None]]])
def test_not_a_pair(no_engine, bad):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=r"^NearestSourceField: source_sets\[0\]\[0\] must be an \(r, c\) pair"):
        make(g, bad)


def test_sets_must_be_lists(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^NearestSourceField: source_sets must be a list of lists"):
        make(g, 5)
    with pytest.raises(ValueError, match=r"^NearestSourceField: source_sets\[1\] must be a list of \(r, c\) pairs"):
        make(g, [[(0, 0)], 7])


def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^NearestSourceField: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)])


def test_engine_of_another_shape(no_engine):
    g, _, _ = gio.grid("fig7")

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^NearestSourceField: the engine's grid has another shape"):
        make(g, [(0, 0)], engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, [(0, 0), (19, 19)])
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, [[(0, 0)], [(19, 19), (0, 0)]], allow_diagonal_moves=False)


@pytest.mark.parametrize("b", [-1, 2, 1.5, "0", None, True])
def test_set_index(field, b):
    for call in (lambda: field.paths([(0, 0)], b=b), lambda: field.nearest(b, (0, 0)), lambda: field.next_hop(b, (0, 0)),
                 lambda: field.territory_sizes(b)):
        with pytest.raises(ValueError, match=r"^NearestSourceField: b = .* is outside \[0, 2\)"):
            call()


@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3)])
def test_cell_out_of_range(field, cell):
    for call in (lambda: field.paths([(0, 0), cell]), lambda: field.nearest(0, cell), lambda: field.next_hop(0, cell)):
        with pytest.raises(ValueError, match=r"^NearestSourceField: targets\[[01]\] = .* is outside the 20x20 grid"):
            call()


@pytest.mark.parametrize("bad", [7, (1, 2, 3), "ab", None])
def test_cell_not_a_pair(field, bad):
    for call in (lambda: field.paths([bad]), lambda: field.nearest(1, bad), lambda: field.next_hop(1, bad)):
        with pytest.raises(ValueError, match=r"^NearestSourceField: targets\[0\] must be an \(r, c\) pair"):
            call()


def test_targets_and_path_cap(field):
    with pytest.raises(ValueError, match="^NearestSourceField: targets must be a list"):
        field.paths(5)
    for cap in (0, -3):
        with pytest.raises(ValueError, match="^NearestSourceField: path_cap must be >= 1"):
            field.paths([(0, 0)], path_cap=cap)
