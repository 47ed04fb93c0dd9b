"""DistanceField argument checks: ValueError before any Engine exists (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import dist_field

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(dist_field, "Engine", boom)


def make(g, **kw):
    from pathfit import DistanceField
    return DistanceField(g, **kw)


def test_empty_source_list(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^DistanceField: sources is empty"):
        make(g, sources=[])


@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3)])
def test_out_of_range(no_engine, cell):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=r"^DistanceField: sources\[1\] = .* is outside the 20x20 grid"):
        make(g, sources=[(0, 0), cell])


def test_on_an_obstacle(no_engine):
    g, _, _ = gio.grid("fig7")
    r, c = (int(v) for v in np.argwhere(np.asarray(g) == 1)[0])
    with pytest.raises(ValueError, match=rf"^DistanceField: sources\[1\] = \({r}, {c}\) is on an obstacle"):
        make(g, sources=[(0, 0), (r, c)])


@pytest.mark.parametrize("bad", [[7], [(1, 2, 3)], ["ab", (0, 0)], [None]])
def test_not_a_pair(no_engine, bad):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=r"^DistanceField: sources\[0\] must be an \(r, c\) pair"):
        make(g, sources=bad)


def test_sources_must_be_a_list(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^DistanceField: sources must be a list"):
        make(g, sources=5)


def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^DistanceField: grid must be 2-D"):
        make(np.zeros(16, int), sources=[(0, 0)])


def test_missing_target_marker(no_engine):
    """sources defaults to the grid's target marker: a grid without one fails with the class's name in front."""
    g, _, _ = gio.grid("fig7")
    h = np.array(g)
    h[h == 3] = 0
    with pytest.raises(ValueError, match="^DistanceField: Target node not found"):
        make(h)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(h, sources=[(0, 0)])


def test_engine_of_another_shape(no_engine):
    g, _, _ = gio.grid("fig7")

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^DistanceField: the engine's grid has another shape"):
        make(g, sources=[(0, 0)], engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, sources=[(0, 0), (19, 19)], allow_diagonal_moves=False)
