"""AStarSolver and DijkstraSolver share one body: each still asks Engine.astar_host for its own variant (0 / 2), and its
`*_strictly_restricts_corners` attribute, flipped after construction, still reaches the call (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio


class RecordingEngine:
    """Stands in for an Engine: records what astar_host is asked and answers with the two-cell path start -> target."""

    def __init__(self):
        self.calls = []

    def astar_host(self, variant, starts, targets, avoid_lists=None, path_cap=None, allow_diag=True, restrict_corner=True):
        self.calls.append({"variant": variant, "path_cap": path_cap, "allow_diag": allow_diag, "restrict_corner": restrict_corner})
        return [np.array([starts[0], targets[0]], np.int32)], np.zeros(1, np.int32)

    def score_host(self, paths, sp):
        return np.array([[1.0, 0.0, 0.0, 0.0, 1.0]] * len(paths))


@pytest.mark.parametrize("name, variant, attr", [("AStarSolver", 0, "astar_strictly_restricts_corners"),
                                                 ("DijkstraSolver", 2, "dijkstra_strictly_restricts_corners")])
def test_variant_and_corner_attribute_reach_astar_host(name, variant, attr):
    import pathfit
    g, _, _ = gio.grid("fig7")
    for policy in (True, False):
        e = RecordingEngine()
        solver = getattr(pathfit, name)(g, allow_diagonal_moves=policy, restrict_diagonal_near_obstacle_policy=policy, engine=e)
        assert getattr(solver, attr) is policy
        res = solver.solve()
        assert res[0] == [tuple(solver.start_node), tuple(solver.target_node)] and solver.convergence_curve == [1.0]
        setattr(solver, attr, not policy)                # flipped after construction: the next query obeys it
        solver.solve()
        assert [c["variant"] for c in e.calls] == [variant, variant]
        assert [c["restrict_corner"] for c in e.calls] == [policy, not policy]
        assert [c["allow_diag"] for c in e.calls] == [policy, policy]
        assert [c["path_cap"] for c in e.calls] == [400, 400]
        assert solver.restrict_diagonal_near_obstacle_policy is policy
