"""DistanceField.paths / next_hop argument checks and the DijkstraSolver.solve_many answers that need no device (runs on a CPU-only
host).  The stub engine serves what building a DistanceField already needed (a buffer, the field launch) and fails the test if a
parent map or a trace is asked for before the arguments are checked."""
import numpy as np
import pytest

import golden_io as gio

INF = float("inf")
EMPTY = ([], INF, 0, 0.0, 0.0, INF)


class StubBuf:
    ptr = 1

    def free(self):
        pass


class StubEngine:
    h = 1

    def __init__(self, R, C):
        self.R, self.C = R, C
        self.calls = []

    def buf(self, shape, dtype):
        return StubBuf()

    def dist_field_batch(self, *a, **k):
        self.calls.append("field")

    def last_kernel_ms(self):
        return 0.0

    def default_path_cap(self, W=None):
        return 64

    def _boom(self, *a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    dist_field_parents = dist_field_paths = put = score_batch = score_host = astar_host = _boom


@pytest.fixture
def field():
    from pathfit import DistanceField
    g, _, _ = gio.grid("fig7")
    return DistanceField(g, sources=[(0, 0), (19, 19), (0, 19)], engine=StubEngine(20, 20))


@pytest.mark.parametrize("bad", [[7], [(1, 2, 3)], [(0, 0), "ab"], [None], [(0, 0), (1.5, "x")]])
def test_target_not_a_pair(field, bad):
    with pytest.raises(ValueError, match=r"^DistanceField: targets\[\d\] must be an \(r, c\) pair"):
        field.paths(bad, k=0)


def test_targets_not_a_list(field):
    with pytest.raises(ValueError, match="^DistanceField: targets must be a list"):
        field.paths(5, k=0)


@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3), (400, 400)])
def test_target_outside_the_grid(field, cell):
    with pytest.raises(ValueError, match=r"^DistanceField: targets\[1\] = .* is outside the 20x20 grid"):
        field.paths([(0, 0), cell])
    with pytest.raises(ValueError, match=r"^DistanceField: targets\[0\] = .* is outside the 20x20 grid"):
        field.next_hop(0, cell)


@pytest.mark.parametrize("k", [-1, 3, 400, "a", 1.5])
def test_k_out_of_range(field, k):
    with pytest.raises(ValueError, match=r"^DistanceField: k = .* is outside \[0, 3\)"):
        field.paths([(0, 0)], k=k)
    with pytest.raises(ValueError, match=r"^DistanceField: k = .* is outside \[0, 3\)"):
        field.paths([(0, 0), (1, 1)], k=[0, k])
    with pytest.raises(ValueError, match=r"^DistanceField: k = .* is outside \[0, 3\)"):
        field.next_hop(k, (0, 0))


def test_k_and_targets_of_different_lengths(field):
    with pytest.raises(ValueError, match="^DistanceField: 2 k for 3 targets"):
        field.paths([(0, 0), (1, 1), (2, 2)], k=[0, 1])
    with pytest.raises(ValueError, match="^DistanceField: 1 k for 0 targets"):
        field.paths([], k=[0])


def test_path_cap_must_be_positive(field):
    with pytest.raises(ValueError, match="^DistanceField: path_cap must be >= 1"):
        field.paths([(0, 0)], k=0, path_cap=0)


def test_no_targets_is_no_device_call(field):
    assert field.paths([]) == [] and field.paths([], k=1) == [] and field.paths([], k=[]) == []
    assert field.chosen.shape == (0,) and field.engine.calls == ["field"]


def test_a_target_on_an_obstacle_is_legal(field):
    """... so with valid arguments the device is reached (an empty path is the device's answer, tests/test_gpu_field_paths.py)."""
    r, c = (int(v) for v in np.argwhere(field.grid == 1)[0])
    with pytest.raises(AssertionError, match="the device was touched"):
        field.paths([(r, c)], k=0)
    with pytest.raises(AssertionError, match="the device was touched"):
        field.paths([(0, 0), (3, 3)])
    with pytest.raises(AssertionError, match="the device was touched"):
        field.next_hop(2, (r, c))
    with pytest.raises(AssertionError, match="the device was touched"):
        field.parents


def test_closed_field_raises():
    from pathfit import DistanceField, PathfitError
    g, _, _ = gio.grid("fig7")
    d = DistanceField(g, sources=[(0, 0)], engine=StubEngine(20, 20))
    d.close()
    with pytest.raises(PathfitError, match="closed"):
        d.parents
    with pytest.raises(PathfitError, match="closed"):
        d.paths([(1, 1)], k=0)


# ---- DijkstraSolver.solve_many: the answers that need no device
def solver():
    from pathfit import DijkstraSolver
    g, _, _ = gio.grid("fig7")
    return DijkstraSolver(g, engine=StubEngine(20, 20)), g


def test_solve_many_without_targets():
    s, _ = solver()
    assert s.solve_many([]) == [] and s.convergence_curve == []


@pytest.mark.parametrize("start", [(-1, 0), (0, 20), (25, 25)])
def test_solve_many_start_outside_the_grid(start):
    s, _ = solver()
    got = s.solve_many([(0, 0), (5, 5), start], start_node_override=start)
    assert got == [EMPTY] * 3 and all(type(t) is tuple for t in got) and s.convergence_curve == []
    assert got[0][0] is not got[1][0]                                 # (each tuple owns its list)


def test_solve_many_start_on_an_obstacle():
    s, g = solver()
    r, c = (int(v) for v in np.argwhere(np.asarray(g) == 1)[0])
    assert s.solve_many([(0, 0), (r, c), None], start_node_override=(r, c)) == [EMPTY] * 3 and s.convergence_curve == []


def test_solve_many_every_target_outside_the_grid():
    s, _ = solver()
    assert s.solve_many([(-1, 3), (20, 0), (0, 99)]) == [EMPTY] * 3 and s.convergence_curve == []


def test_solve_many_reaches_the_device_for_a_target_in_the_grid():
    s, _ = solver()
    with pytest.raises(AssertionError, match="the device was touched"):
        s.solve_many([(-1, 3), (4, 4)])
    assert s.engine.calls == ["field"]
