"""PathSmoother argument checks: ValueError before any device is touched (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import smooth

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(smooth, "Engine", boom)


class Untouchable:
    """An engine of fig7's shape whose every device call fails the test."""
    R, C = 20, 20

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def make(g, **kw):
    from pathfit import PathSmoother
    return PathSmoother(g, **kw)


def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^PathSmoother: grid must be 2-D"):
        make(np.zeros(16, int))
    with pytest.raises(ValueError, match="^PathSmoother: grid must be 2-D"):
        make(np.zeros((2, 2, 2), int))


def test_engine_of_another_shape(no_engine):
    g, _, _ = gio.grid("fig7")

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^PathSmoother: the engine's grid has another shape"):
        make(g, engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, restrict_diagonal_near_obstacle=False)
    s = make(g, engine=Untouchable())                               # a passed engine is not touched by the constructor
    with pytest.raises(AssertionError, match="the device was touched"):
        s.visible([((0, 0), (3, 4))])
    with pytest.raises(AssertionError, match="the device was touched"):
        s.smooth([[(0, 0), (0, 1), (1, 2)]])
    with pytest.raises(AssertionError, match="the device was touched"):
        s.visible([((0, 0), (3, 40))])                              # an endpoint beside the grid is an answer (False), no error


@pytest.mark.parametrize("bad", [[7], [((0, 0),)], [((0, 0), (1, 1), (2, 2))], ["ab"], [None], [((0, 0), 5)], [((0, 0), (1, 2, 3))],
                                 [((0, 0), (1, 1)), ((0, "x"), (1, 1))]])
def test_not_a_pair_of_pairs(no_engine, bad):
    g, _, _ = gio.grid("fig7")
    s = make(g, engine=Untouchable())
    with pytest.raises(ValueError, match=rf"^PathSmoother: pairs\[{len(bad) - 1}\](\[[01]\])? must be "):
        s.visible(bad)
    with pytest.raises(ValueError, match="^PathSmoother: pairs must be a list"):
        s.visible(5)


@pytest.mark.parametrize("cell, shown", [((-1, 0), r"\(-1, 0\)"), ((0, 20), r"\(0, 20\)"), ((20, 3), r"\(20, 3\)")])
def test_path_cell_outside_the_grid(no_engine, cell, shown):
    g, _, _ = gio.grid("fig7")
    s = make(g, engine=Untouchable())
    with pytest.raises(ValueError, match=rf"^PathSmoother: paths\[1\]\[2\] = {shown} is outside the 20x20 grid"):
        s.smooth([[(0, 0), (0, 1)], [(0, 0), (0, 1), cell, (1, 1)]])


@pytest.mark.parametrize("bad", [-1, 400, 2 ** 31 - 1])
def test_path_cell_id_outside_the_grid(no_engine, bad):
    from pathfit import CellPath
    g, _, _ = gio.grid("fig7")
    s = make(g, engine=Untouchable())
    with pytest.raises(ValueError, match=rf"^PathSmoother: paths\[0\]\[1\] = cell {bad} is outside the 20x20 grid"):
        s.smooth([np.array([0, bad, 2], np.int64)])
    if bad < 2 ** 31 - 1:
        with pytest.raises(ValueError, match=rf"^PathSmoother: paths\[2\]\[0\] = cell {bad} is outside"):
            s.smooth([CellPath([0, 1], 20), [], CellPath([bad], 20)])


def test_path_shapes(no_engine):
    from pathfit import CellPath
    g, _, _ = gio.grid("fig7")
    s = make(g, engine=Untouchable())
    with pytest.raises(ValueError, match=r"^PathSmoother: paths\[0\]\[1\] must be an \(r, c\) pair"):
        s.smooth([[(0, 0), 5]])
    with pytest.raises(ValueError, match=r"^PathSmoother: paths\[1\] must be a CellPath, a list"):
        s.smooth([[(0, 0)], 7])
    with pytest.raises(ValueError, match="^PathSmoother: paths must be a sequence"):
        s.smooth(7)
    with pytest.raises(ValueError, match=r"^PathSmoother: paths\[0\] belongs to a grid of 21 columns"):
        s.smooth([CellPath([0, 1], 21)])
    assert s.smooth([]) == [] and len(s.visible([])) == 0            # nothing to do: nothing is launched
    with pytest.raises(ValueError, match="^PathSmoother: smooth_device needs n >= 1"):
        s.smooth_device(None, None, 0, 8)
    with pytest.raises(ValueError, match="^PathSmoother: smooth_device needs"):
        s.smooth_device(None, None, 4, 8, way_cap=0)


def test_use_after_close(no_engine):
    g, _, _ = gio.grid("fig7")
    s = make(g, engine=Untouchable())
    s.close()
    s.close()
    for call in (lambda: s.visible([((0, 0), (1, 1))]), lambda: s.smooth([[(0, 0)]]), lambda: s.smooth_device(None, None, 1, 8)):
        with pytest.raises(ValueError, match="^PathSmoother: the smoother is closed"):
            call()
