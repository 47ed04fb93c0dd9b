"""TurnField: the exact optimum of length plus a turn penalty (pf_turn_field) -- what `length + w_t * turns` of the solvers' score
can reach at best, to hold their results against.  A turn depends on the move before, so the field lives on (cell, heading) states:
states[b, d, r, c] is the cheapest cost of a walk from a source of set b that enters (r, c) by move d (helper.py:30-36 order), a
move weighing as CostField's and turn_weight more when it differs from the move before; best[b, r, c] is the smallest of the eight.
At turn_weight == 0 best is CostField's field bit for bit.  `paths` reads the route out of the states alone (pf_turn_field_paths);
`path_costs` scores any path rows under the same rule (pf_turn_paths).  Everything stays in HBM; `refresh` recomputes after
`engine.update_grid`, under a new cost map or a new turn weight; `repair` updates the field it holds for the cells that changed
(pf_turn_field_repair), with the same result."""
import numpy as np

from ._field import Field
from ._lib import PathfitError
from .cost_field import CostField, changed_cells, checked_cost
from .engine import Engine
from .nearest_field import NearestSourceField
from .paths import CellPath

TURN_WEIGHT_MAX = float(2 ** 20)


def checked_turn_weight(who, w):
    """w as a float: a finite number in [0, 2^20]."""
    ok = isinstance(w, (int, float, np.integer, np.floating)) and not isinstance(w, (bool, np.bool_))
    if not (ok and 0.0 <= float(w) <= TURN_WEIGHT_MAX):                # (NaN fails both comparisons)
        raise ValueError(f"{who}: turn_weight must be a finite number in [0, 2^20], got {w!r}")
    return float(w)


class TurnField(Field):
    """best[b, r, c] = the least, over the paths from a source of source_sets[b] to (r, c) under the move policy, of the path's
    length plus turn_weight per turn (inf: an obstacle, or out of reach); the first move of a path is no turn.  cost: None (every
    cell costs 1) or an [R, C] array as CostField's.  A walk's cost is summed left to right in float64, a turning step adding
    fl(w + turn_weight) in one piece; best and states hold exactly what a heap Dijkstra over the states leaves, bit for bit, whatever
    the timing of the device.

    info: int64 [B, 4] = (sources that counted, cells reached, the cell id with the largest finite best -- the smallest on a tie, -1
    when nothing is reached --, 0).  work: (launches of the tile kernel, tile visits, state words lowered, 0) of the last computation
    ((launches of both phases, tile visits of both, state words lowered, state words raised) after `repair`)."""
    _bufs = ("cost_device", "sbuf", "bbuf", "ibuf")
    _set_source_sets = NearestSourceField._set_source_sets

    def __init__(self, grid, source_sets, turn_weight, cost=None, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        who = type(self).__name__
        self._set_grid(grid)
        self._set_source_sets(source_sets, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        self.turn_weight = checked_turn_weight(who, turn_weight)
        self.cost = None if cost is None else checked_cost(who, self.grid, cost)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        e = self.engine
        self.cost_device = None if self.cost is None else e.put(self.cost.reshape(-1), np.float64)
        self.sbuf = e.buf((self.B, 8, self.rows, self.cols), np.float64)
        self.bbuf = e.buf((self.B, self.rows, self.cols), np.float64)
        self.ibuf = e.buf((self.B, 4), np.int64)
        self._compute()

    def _compute(self):
        self._states = self._best = self._info = None
        e = self.engine
        e.turn_field(self.cost_device, self.turn_weight, self.set_off, self.ids, self.sbuf, self.bbuf, self.allow_diagonal_moves,
                     self.restrict_diagonal_near_obstacle, self.ibuf)
        self.kernel_ms = e.last_kernel_ms()
        self.work = e.turn_field_work()

    def _check_open(self):
        if self.bbuf is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the field is closed")

    @property
    def best(self):
        """float64 [B, R, C], downloaded on first use."""
        if self._best is None:
            self._check_open()
            self._best = self.bbuf.download()
        return self._best

    @property
    def states(self):
        """float64 [B, 8, R, C], downloaded on first use."""
        if self._states is None:
            self._check_open()
            self._states = self.sbuf.download()
        return self._states

    @property
    def info(self):
        """int64 [B, 4]: sources that counted, cells reached, the cell with the largest finite best (-1: nothing reached), 0."""
        if self._info is None:
            self._check_open()
            self._info = self.ibuf.download()
        return self._info

    def heading(self, b, cell):
        """The move by which the best route from set b arrives at `cell` (r, c), the one the route rule starts from: the d with the
        smallest (states[b, d, cell], d) -- 0 on a source, whose eight states are 0 --; None where no route ends."""
        b = self._index("b", b, self.B)
        cid = self._cell("cell", cell)
        self._check_open()
        rc = self.rows * self.cols
        if self._states is not None:
            col = self._states.reshape(self.B, 8, rc)[b, :, cid]
        else:
            col = np.array([self.sbuf.read((b * 8 + d) * rc + cid, 1)[0] for d in range(8)])
        d = int(np.argmin(col))                                       # (the first minimum)
        return d if np.isfinite(col[d]) else None

    def paths(self, targets, b=0, reverse=False, path_cap=None):
        """The route from a source of set b to each of `targets` ((r, c) pairs) whose cost is best[b] at the target -> a list of
        CellPath, empty where no route ends.  reverse: target -> source.  path_cap: cells per row (default: the engine's, and once
        more at R * C where a route outgrows it); a route longer than a given path_cap is a PathfitError."""
        who = type(self).__name__
        ids = self._cell_ids("targets", targets)
        b = self._index("b", b, self.B)
        if path_cap is not None and int(path_cap) < 1:
            raise ValueError(f"{who}: path_cap must be >= 1")
        self._check_open()
        n, full = len(ids), self.rows * self.cols
        if n == 0:
            return []
        e = self.engine
        dt, db = e.put(ids, np.int32), e.put(np.full(n, b, np.int32))
        dl, dst = e.buf(n, np.int32), e.buf(n, np.int32)
        cap = int(path_cap) if path_cap else e.default_path_cap()
        dc = None
        try:
            while True:
                dc = e.buf((n, cap), np.int32)
                e.turn_field_paths(self.cost_device, self.turn_weight, self.B, self.sbuf, db, dt, n, cap, dc, dl, dst, reverse)
                self.trace_kernel_ms = e.last_kernel_ms()
                st = dst.download()
                if path_cap or cap >= full or not (st == 3).any():
                    break
                dc.free()
                cap = full
            if (st == 3).any():
                raise PathfitError(f"{who}: {int((st == 3).sum())} paths hold more than path_cap = {cap} cells")
            self.status = st
            lens = dl.download()
            cells = dc.download() if lens.any() else np.zeros((n, 1), np.int32)
            return [CellPath(cells[i, :lens[i]].copy(), self.cols) for i in range(n)]
        finally:
            for buf in (dt, db, dl, dst, dc):
                if buf is not None:
                    buf.free()

    def path_costs(self, paths):
        """paths: what CostField.path_costs accepts (CellPaths, lists of (r, c), integer cell arrays, or the device tuple (d_cells,
        d_len, n, path_cap)) -> (float64 [n], int32 [n], int32 [n]): each row's cost under the rule, summed left to right (0 for a
        one-cell row), its turns, and -1; for a row with a step that is no king move between cells of the grid NaN, 0 and the index
        of the first such step (0 for an empty row).  Obstacles are not consulted."""
        out = CostField.path_costs(self, paths)                       # its parser of the host forms; the rows come back to _path_costs
        return out if len(out) == 3 else (out[0], np.zeros(0, np.int32), out[1])

    def _path_costs(self, d_cells, d_len, n, cap):
        e = self.engine
        dt, dn, db = e.buf(n, np.float64), e.buf(n, np.int32), e.buf(n, np.int32)
        try:
            e.turn_paths(self.cost_device, self.turn_weight, n, cap, d_cells, d_len, dt, dn, db)
            self.path_costs_kernel_ms = e.last_kernel_ms()
            return dt.download(), dn.download(), db.download()
        finally:
            for buf in (dt, dn, db):
                buf.free()

    def refresh(self, cost=None, turn_weight=None):
        """Compute the field again on the map the engine holds now (after engine.update_grid) and, when given, under a new cost map
        or turn weight; everything downloaded before is dropped.  A field built without a cost map takes one here."""
        who = type(self).__name__
        self._check_open()
        held = getattr(self.engine, "grid_u8", None)
        grid = np.array(held, dtype=int) if held is not None else self.grid
        wt = self.turn_weight if turn_weight is None else checked_turn_weight(who, turn_weight)
        new = self.cost if cost is None else cost
        if new is not None:
            new = checked_cost(who, grid, new)
        self.grid, self.turn_weight = grid, wt
        if cost is not None:
            self.cost = new
            if self.cost_device is None:
                self.cost_device = self.engine.put(new.reshape(-1), np.float64)
            else:
                self.cost_device.upload(new.reshape(-1))
        self._compute()
        return self

    def repair(self, cost=None):
        """refresh(cost), done incrementally (pf_turn_field_repair): the field held here is repaired for the map the engine holds now
        (after engine.update_grid) and, when given, a new cost map; the turn weight is not changed here (that is refresh).  The cells
        that differ (cost_field.changed_cells; a field without a cost map compares against ones, and takes a cost map here as refresh
        does) are found here; the states that lost their support are raised to inf on the device, best is rewritten, and both are
        lowered again from there, at a cost that follows the tiles the invalid region crosses instead of the map.  States, best and
        info are bit for bit refresh's.  With nothing changed it returns at once and keeps what was downloaded; otherwise states,
        best and info are dropped as refresh drops them.  work: (launches of both phases, tile visits of both, state words lowered,
        state words raised).  A change next to a source may invalidate most of the field: the repair then crosses the same tiles
        twice and can take as long as refresh, or longer (DESIGN.md 4.23 has the figures)."""
        who = type(self).__name__
        self._check_open()
        held = getattr(self.engine, "grid_u8", None)
        grid = np.array(held, dtype=int) if held is not None else self.grid
        new = self.cost if cost is None else cost
        if new is not None:
            new = checked_cost(who, grid, new)
        ones = np.ones(grid.shape)
        changed = changed_cells(self.grid, ones if self.cost is None else self.cost, grid, ones if new is None else new)
        if changed.size == 0:
            return self
        if cost is not None:
            if self.cost_device is None:
                self.cost_device = self.engine.put(new.reshape(-1), np.float64)
            else:
                self.cost_device.upload(new.reshape(-1))
        self._states = self._best = self._info = None
        e = self.engine
        e.turn_field_repair(self.cost_device, self.turn_weight, changed, self.set_off, self.ids, self.sbuf, self.bbuf, self.allow_diagonal_moves,
                            self.restrict_diagonal_near_obstacle, self.ibuf)
        self.grid = grid
        if cost is not None:
            self.cost = new
        self.work = e.turn_field_work()
        self.kernel_ms = e.last_kernel_ms()
        return self
