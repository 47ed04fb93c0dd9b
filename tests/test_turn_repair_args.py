"""TurnField.repair's host side: every ValueError comes before the device is touched, the changed list is formed as the rule says --
a field without a cost map compares against ones --, and the facade's bookkeeping runs over a model engine whose `turn_field_repair`
is the model of tests/turn_repair_checkers.py (runs on a CPU-only host)."""
import math

import numpy as np
import pytest

import cost_checkers as ck
import golden_io as gio
import turn_checkers as tk
import turn_repair_checkers as tr
from test_turn_field_args import ModelEngine as FieldEngine

WT = 0.3
SETS = [[0], [399, 0]]
PAIRS = [[(0, 0)], [(19, 19), (0, 0)]]


class ModelEngine(FieldEngine):
    """test_turn_field_args' model engine with a repair: the model on the rows it is given, under the grid the engine holds."""

    def __init__(self, g):
        super().__init__(g)
        self.repairs, self.work = [], (1, 1, 1, 0)

    def update_grid(self, g):
        self.grid_u8 = np.asarray(g, np.uint8)

    def turn_field_repair(self, d_cost, turn_weight, changed, set_off, sources, d_states, d_best, allow_diag=True, restrict_corner=True, d_info=None):
        sets = [list(sources[set_off[b]:set_off[b + 1]]) for b in range(len(set_off) - 1)]
        cost = None if d_cost is None else d_cost.a.reshape(self.R, self.C)
        T = d_states.a.reshape(len(sets), 8, self.R, self.C)
        best = d_best.a.reshape(len(sets), self.R, self.C)
        raised = lowered = 0
        for b, s in enumerate(sets):
            out = tr.repair(T[b], self.grid_u8, cost, s, turn_weight, [int(v) for v in changed], allow_diag, restrict_corner, seed=b)
            T[b], best[b] = out.T, out.best
            raised, lowered = raised + out.n_raised, lowered + len(out.lowered)
            d_info.a[4 * b:4 * b + 4] = tk.info_of(self.grid_u8, out.best, s)
        self.repairs.append((np.array(changed).tolist(), turn_weight))
        self.work = (2, 2, lowered, raised)

    def turn_field_work(self):
        return self.work


def make(with_cost):
    from pathfit import TurnField
    g, _, _ = gio.grid("fig7")
    g = np.where(g == 1, 1, 0)
    cost = ck.cost_of_kind("u50", g.shape, 1) if with_cost else None
    e = ModelEngine(g)
    return TurnField(g, PAIRS, WT, cost=cost, engine=e), e, g, cost


def want(g, cost):
    return tk.fields(g, cost, SETS, WT, True, True)


def test_a_bad_cost_map_changes_nothing():
    f, e, g, cost = make(True)
    states = f.states
    for bad, msg in ((np.ones((3, 3)), "^TurnField: cost has shape"), ("abc", "^TurnField: cost (must be an|has shape)"),
                     ([[1.0, "x"]], "^TurnField: cost (must be an|has shape)")):
        with pytest.raises(ValueError, match=msg):
            f.repair(cost=bad)
    for v in (0.5, 0.0, -3.0, 2.0 ** 20 + 1, math.nan, math.inf):
        bad = cost.copy()
        bad[0, 0] = v
        with pytest.raises(ValueError, match=r"^TurnField: cost\[0, 0\] = .* on a free cell is not a finite number in \[1, 2\^20\]"):
            f.repair(cost=bad)
    assert e.repairs == [] and e.calls == 1 and f.states is states and np.array_equal(f.cost, cost)
    assert np.array_equal(f.cost_device.a.reshape(g.shape), cost)
    # the held cost map is checked against the map the engine holds NOW: garbage under a wall that opened
    wall = tuple(int(v) for v in np.argwhere(g == 1)[0])
    g2 = g.copy()
    g2[wall] = 0
    f.cost[wall] = math.nan
    e.update_grid(g2)
    with pytest.raises(ValueError, match=rf"^TurnField: cost\[{wall[0]}, {wall[1]}\] = nan on a free cell"):
        f.repair()
    assert e.repairs == [] and f.grid[wall] == 1
    f.close()
    from pathfit._lib import PathfitError
    with pytest.raises(PathfitError, match="^TurnField: the field is closed"):
        f.repair()


@pytest.mark.parametrize("with_cost", [True, False])
def test_nothing_changed_returns_at_once(with_cost):
    f, e, g, cost = make(with_cost)
    states, best, info = f.states, f.best, f.info
    held = np.ones(g.shape) if cost is None else cost
    assert f.repair() is f and f.repair(cost=held.copy()) is f and f.repair(cost=held.tolist()) is f
    junk = held.copy()
    junk[g == 1] = math.nan                                           # what lies under an obstacle is not compared
    assert f.repair(cost=junk) is f
    assert e.repairs == [] and e.calls == 1 and f.states is states and f.best is best and f.info is info and f.work == (1, 1, 1, 0)
    if with_cost:
        assert np.array_equal(f.cost_device.a.reshape(g.shape), cost)
    else:
        assert f.cost is None and f.cost_device is None               # a map of ones given to a field without one changes nothing: none is taken


def test_the_changed_list_and_the_bookkeeping():
    f, e, g, cost = make(True)
    wall = tuple(int(v) for v in np.argwhere(g == 1)[3])
    free = [tuple(int(v) for v in p) for p in np.argwhere(g != 1)[[5, 40, 90]]]
    # update_grid alone: one cell closes, one opens (its held cost is a legal one)
    g1 = g.copy()
    g1[wall], g1[free[0]] = 0, 1
    e.update_grid(g1)
    _ = f.states, f.best, f.info
    assert f.repair() is f
    assert e.repairs[-1] == (sorted([wall[0] * 20 + wall[1], free[0][0] * 20 + free[0][1]]), WT) and e.calls == 1
    assert f._states is None and f._best is None and f._info is None  # dropped, and downloaded again on use
    T, best, info = want(g1, cost)
    assert tr.same_bits(f.states, T) and tr.same_bits(f.best, best) and np.array_equal(f.info, info)
    assert np.array_equal(f.grid, g1) and f.work[3] > 0 and f.work == e.work and f.turn_weight == WT
    # a new cost map alone: the cells that differ on free cells, nothing under the walls
    cost2 = cost.copy()
    cost2[free[1]], cost2[free[2]] = 1.0, 77.25
    cost2[g1 == 1] = -1.0
    assert f.repair(cost=cost2) is f
    assert e.repairs[-1][0] == sorted(p[0] * 20 + p[1] for p in free[1:]) and f.cost is not cost2
    assert np.array_equal(f.cost, cost2) and np.array_equal(f.cost_device.a.reshape(g.shape), cost2)
    assert tr.same_bits(f.states, want(g1, cost2)[0])
    # both at once; the cell that opens takes its cost from the new map
    g3 = g1.copy()
    g3[free[0]] = 0
    cost3 = cost2.copy()
    cost3[free[0]], cost3[free[1]] = 3.5, 2.0
    e.update_grid(g3)
    f.repair(cost=cost3)
    assert e.repairs[-1][0] == sorted(p[0] * 20 + p[1] for p in free[:2])
    assert tr.same_bits(f.states, want(g3, cost3)[0]) and tr.same_bits(f.best, want(g3, cost3)[1]) and np.array_equal(f.grid, g3)
    assert len(e.repairs) == 3 and e.calls == 1                       # never a field from nothing


def test_a_field_without_a_cost_map_compares_against_ones_and_takes_one():
    f, e, g, _ = make(False)
    free = [tuple(int(v) for v in p) for p in np.argwhere(g != 1)[[7, 60]]]
    g1 = g.copy()
    g1[free[0]] = 1
    e.update_grid(g1)
    f.repair()
    assert e.repairs[-1][0] == [free[0][0] * 20 + free[0][1]] and f.cost is None and f.cost_device is None
    assert tr.same_bits(f.states, want(g1, None)[0])
    cost = np.ones(g.shape)
    cost[free[1]] = 6.5
    cost[free[0]] = math.nan                                          # under the wall now: not looked at
    nbufs = len(e.bufs)
    f.repair(cost=cost)
    assert e.repairs[-1][0] == [free[1][0] * 20 + free[1][1]]          # against ones: the one cell that costs more
    assert len(e.bufs) == nbufs + 1 and f.cost_device is e.bufs[-1] and np.array_equal(f.cost_device.a.reshape(g.shape), cost, equal_nan=True)
    assert np.array_equal(f.cost, cost, equal_nan=True)
    assert tr.same_bits(f.states, want(g1, cost)[0]) and np.array_equal(f.info, want(g1, cost)[2])
    cost2 = cost.copy()
    cost2[free[1]] = 1.0
    f.repair(cost=cost2)                                              # the buffer is kept and uploaded to
    assert len(e.bufs) == nbufs + 1 and tr.same_bits(f.best, want(g1, None)[1])
