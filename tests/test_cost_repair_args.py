"""CostField.repair's host side: every ValueError comes before the device is touched, the changed list is formed as the rule says,
and the facade's bookkeeping runs over a model engine whose `cost_field_repair` is the model of tests/repair_checkers.py (runs on a
CPU-only host)."""
import math

import numpy as np
import pytest

import cost_checkers as ck
import golden_io as gio
import repair_checkers as rc
from test_cost_field_args import HostBuf, ModelEngine as FieldEngine


class ModelEngine(FieldEngine):
    """test_cost_field_args' model engine with a repair: the model on the rows it is given, under the grid the engine holds."""

    def __init__(self, g):
        super().__init__(g)
        self.repairs, self.work = [], (1, 1, 1, 0)

    def update_grid(self, g):
        self.grid_u8 = np.asarray(g, np.uint8)

    def cost_field_repair(self, d_cost, changed, set_off, sources, d_rows, allow_diag=True, restrict_corner=True, d_info=None):
        sets = [list(sources[set_off[b]:set_off[b + 1]]) for b in range(len(set_off) - 1)]
        cost = d_cost.a.reshape(self.R, self.C)
        rows = d_rows.a.reshape(len(sets), self.R, self.C)
        raised = lowered = 0
        for b, s in enumerate(sets):
            out = rc.repair(rows[b], self.grid_u8, cost, s, [int(v) for v in changed], allow_diag, restrict_corner, seed=b)
            rows[b] = out.D
            raised, lowered = raised + out.n_raised, lowered + len(out.lowered)
            d_info.a[4 * b:4 * b + 4] = ck.info_of(self.grid_u8, out.D, s)
        self.repairs.append(np.array(changed).tolist())
        self.work = (2, 2, lowered, raised)

    def cost_field_work(self):
        return self.work


@pytest.fixture
def field():
    from pathfit import CostField
    g, _, _ = gio.grid("fig7")
    g = np.where(g == 1, 1, 0)
    cost = ck.cost_of_kind("u50", g.shape, 1)
    e = ModelEngine(g)
    return CostField(g, cost, [[(0, 0)], [(19, 19), (0, 0)]], engine=e), e, g, cost


SETS = [[0], [399, 0]]


def test_a_bad_cost_map_changes_nothing(field):
    f, e, g, cost = field
    want = f.fields
    for bad, msg in ((np.ones((3, 3)), "^CostField: cost has shape"), ("abc", "^CostField: cost (must be an|has shape)"),
                     ([[1.0, "x"]], "^CostField: cost (must be an|has shape)")):
        with pytest.raises(ValueError, match=msg):
            f.repair(cost=bad)
    for v in (0.5, 0.0, -3.0, 2.0 ** 20 + 1, math.nan, math.inf):
        bad = cost.copy()
        bad[0, 0] = v
        with pytest.raises(ValueError, match=r"^CostField: cost\[0, 0\] = .* on a free cell is not a finite number in \[1, 2\^20\]"):
            f.repair(cost=bad)
    assert e.repairs == [] and e.calls == 1 and f.fields is want and np.array_equal(f.cost, cost)
    assert np.array_equal(f.cost_device.a.reshape(g.shape), cost)
    # the held cost map is checked against the map the engine holds NOW: garbage under a wall that opened
    wall = tuple(int(v) for v in np.argwhere(g == 1)[0])
    g2 = g.copy()
    g2[wall] = 0
    f.cost[wall] = math.nan
    e.update_grid(g2)
    with pytest.raises(ValueError, match=rf"^CostField: cost\[{wall[0]}, {wall[1]}\] = nan on a free cell"):
        f.repair()
    assert e.repairs == [] and f.grid[wall] == 1
    f.close()
    from pathfit._lib import PathfitError
    with pytest.raises(PathfitError, match="^CostField: the field is closed"):
        f.repair()


def test_nothing_changed_returns_at_once(field):
    f, e, g, cost = field
    fields, parents_state = f.fields, f._parents
    assert f.repair() is f and f.repair(cost=cost.copy()) is f and f.repair(cost=cost.tolist()) is f
    junk = cost.copy()
    junk[g == 1] = math.nan                                           # what lies under an obstacle is not compared
    assert f.repair(cost=junk) is f
    assert e.repairs == [] and e.calls == 1 and f.fields is fields and f._parents is parents_state and f.work == (1, 1, 1, 0)
    assert np.array_equal(f.cost_device.a.reshape(g.shape), cost)


def test_the_changed_list_and_the_bookkeeping(field):
    f, e, g, cost = field
    wall = tuple(int(v) for v in np.argwhere(g == 1)[3])
    free = [tuple(int(v) for v in p) for p in np.argwhere(g != 1)[[5, 40, 90]]]
    # update_grid alone: one cell closes, one opens (its held cost is a legal one)
    g1 = g.copy()
    g1[wall], g1[free[0]] = 0, 1
    e.update_grid(g1)
    _ = f.fields
    assert f.repair() is f
    assert e.repairs[-1] == sorted([wall[0] * 20 + wall[1], free[0][0] * 20 + free[0][1]]) and e.calls == 1
    assert rc.same_bits(f.fields, ck.fields(g1, cost, SETS, True, True)[0]) and np.array_equal(f.info, ck.fields(g1, cost, SETS, True, True)[2])
    assert np.array_equal(f.grid, g1) and f.work[3] > 0 and f.work == e.work
    # a new cost map alone: the cells that differ on free cells, nothing under the walls
    cost2 = cost.copy()
    cost2[free[1]], cost2[free[2]] = 1.0, 77.25
    cost2[g1 == 1] = -1.0
    assert f.repair(cost=cost2) is f
    assert e.repairs[-1] == sorted(p[0] * 20 + p[1] for p in free[1:]) and f.cost is not cost2
    assert np.array_equal(f.cost, cost2) and np.array_equal(f.cost_device.a.reshape(g.shape), cost2)
    assert rc.same_bits(f.fields, ck.fields(g1, cost2, SETS, True, True)[0])
    # both at once; the cell that opens takes its cost from the new map
    g3 = g1.copy()
    g3[free[0]] = 0
    cost3 = cost2.copy()
    cost3[free[0]], cost3[free[1]] = 3.5, 2.0
    e.update_grid(g3)
    f.repair(cost=cost3)
    assert e.repairs[-1] == sorted(p[0] * 20 + p[1] for p in free[:2])
    assert rc.same_bits(f.fields, ck.fields(g3, cost3, SETS, True, True)[0]) and np.array_equal(f.grid, g3)
    assert len(e.repairs) == 3 and e.calls == 1                       # never a field from nothing


def test_a_repair_drops_what_was_derived(field):
    f, e, g, cost = field
    f._parents, f._owners, f._counts = "p", "o", "c"
    f.pbuf, f.obuf = HostBuf(4, np.uint8), HostBuf(4, np.int32)
    held = (f.pbuf, f.obuf)
    _ = f.fields, f.info
    f.chosen = np.ones(3, np.int32)
    g1 = g.copy()
    g1[tuple(int(v) for v in np.argwhere(g != 1)[7])] = 1
    e.update_grid(g1)
    f.repair()
    assert f._parents is None and f._owners is None and f._counts is None and f._fields is None and f._info is None
    assert f.pbuf is None and f.obuf is None and held[0].freed and held[1].freed and f.chosen.size == 0
