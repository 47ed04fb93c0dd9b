"""CostField: exact weighted shortest paths over a per-cell cost map (pf_cost_field) -- cells that are passable but expensive: rough
terrain, a lane next to a wall, a zone to avoid unless there is no other way.  A move between two cells weighs the mean of their
costs, times sqrt(2) for a diagonal; with cost == 1 everywhere the field is NearestSourceField's bit for bit.  Everything a
NearestSourceField offers (parents, next_hop, owners, territory_sizes, nearest, paths) works on the weighted field through the same
trace and owner kernels; `path_costs` scores any path rows under the cost map (pf_cost_paths).  The cost map stays in HBM
(`cost_device`); `refresh` recomputes after `engine.update_grid` or with a new cost map, `repair` updates the field it holds for the
cells that changed (pf_cost_field_repair), with the same result."""
import numpy as np

from .engine import DevBuf, Engine
from .nearest_field import NearestSourceField
from .paths import CellPath

COST_MAX = float(2 ** 20)


def checked_cost(who, grid, cost):
    """cost as a float64 [R, C] copy: the grid's shape, and finite in [1, 2^20] on every free cell (obstacle cells are not looked at)."""
    try:
        c = np.array(cost, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: cost must be an [R, C] array of numbers, got {cost!r}") from None
    if c.shape != grid.shape:
        raise ValueError(f"{who}: cost has shape {c.shape}, the grid has {grid.shape}")
    bad = np.argwhere((grid != 1) & ~((c >= 1.0) & (c <= COST_MAX)))            # (NaN fails both comparisons)
    if len(bad):
        r, k = (int(v) for v in bad[0])
        raise ValueError(f"{who}: cost[{r}, {k}] = {float(c[r, k])!r} on a free cell is not a finite number in [1, 2^20]")
    return np.ascontiguousarray(c)


def changed_cells(grid0, cost0, grid1, cost1):
    """int32 flat ids, ascending: the cells whose free / obstacle state differs between the two grids, or that are free in both
    with another cost (what lies under an obstacle is never compared: it may be NaN)."""
    free0, free1 = np.asarray(grid0) != 1, np.asarray(grid1) != 1
    if free0.shape != free1.shape or np.shape(cost0) != free0.shape or np.shape(cost1) != free0.shape:
        raise ValueError(f"changed_cells: the shapes differ ({free0.shape}, {np.shape(cost0)}, {free1.shape}, {np.shape(cost1)})")
    both = free0 & free1
    differs = (free0 != free1) | (both & (np.where(both, cost0, 0.0) != np.where(both, cost1, 0.0)))
    return np.flatnonzero(differs.reshape(-1)).astype(np.int32)


class CostField(NearestSourceField):
    """fields[b, r, c] = the cost of the cheapest walk into (r, c) from a source of source_sets[b] under the move policy (inf: an
    obstacle, or out of reach).  cost: an [R, C] array, finite in [1, 2^20] on every free cell (obstacle cells are ignored).  A legal
    move u -> v weighs m = 0.5 * (cost[u] + cost[v]) when straight and sqrt(2) * m when diagonal; a walk's cost is the sum of its
    moves' weights taken left to right in float64, and fields hold exactly what a heap Dijkstra leaves, bit for bit, whatever the
    timing of the device.  parents / paths follow the smallest-(D[u], u) rule of DistanceField under these weights.

    info: int64 [B, 4] = (sources that counted, cells reached, the cell id with the largest finite cost -- the smallest on a tie, -1
    when nothing is reached --, 0).  work: (launches of the tile kernel, tile visits, words lowered, 0) of the last computation."""
    _bufs = ("cost_device",) + NearestSourceField._bufs
    _info_bounds_chains = False             # info[b, 0] counts sources here: the owner kernel takes its R * C bound

    def __init__(self, grid, cost, source_sets, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        self._set_grid(grid)
        self._set_source_sets(source_sets, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        self.cost = checked_cost(type(self).__name__, self.grid, cost)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        self.cost_device = self.engine.put(self.cost.reshape(-1), np.float64)
        self._start()

    def _compute_fields(self):
        e = self.engine
        e.cost_field(self.cost_device, self.set_off, self.ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle, self.ibuf)
        self.work = e.cost_field_work()

    def _compute_parents(self, pbuf):
        self.engine.cost_field_parents(self.cost_device, self.K, self.buf, pbuf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)

    @property
    def info(self):
        """int64 [B, 4]: sources that counted, cells reached, the cell with the largest finite cost (-1: nothing reached), 0."""
        return super().info

    def refresh(self, cost=None):
        """Compute the field again on the map the engine holds now (after engine.update_grid) and, when given, under a new cost map;
        everything downloaded or derived before (fields, parents, owners) is dropped."""
        self._check_open()
        held = getattr(self.engine, "grid_u8", None)
        grid = np.array(held, dtype=int) if held is not None else self.grid
        new = checked_cost(type(self).__name__, grid, self.cost if cost is None else cost)
        self.grid = grid
        if cost is not None:
            self.cost = new
            self.cost_device.upload(new.reshape(-1))
        for name in ("pbuf", "obuf", "cbuf"):
            buf = getattr(self, name)
            setattr(self, name, None)
            if buf is not None:
                buf.free()
        self._fields = self._parents = self._owners = self._counts = self._info = None
        self.chosen = np.zeros(0, np.int32)
        self._compute_fields()
        self.kernel_ms = self.engine.last_kernel_ms()
        return self

    def repair(self, cost=None):
        """refresh(cost), done incrementally (pf_cost_field_repair): the field held here is repaired for the map the engine holds now
        (after engine.update_grid) and, when given, a new cost map.  The cells that differ (changed_cells) are found here; the labels
        that lost their support are raised to inf on the device and lowered again from there, at a cost that follows the tiles the
        invalid region crosses instead of the map.  The fields are bit for bit refresh's.  With nothing changed it returns at once and
        keeps everything derived; otherwise fields, parents and owners are dropped as refresh drops them.  work: (launches of both
        phases, tile visits of both, words lowered, words raised).  A change next to a source may invalidate most of the field: the
        repair then crosses the same tiles twice and can take as long as refresh, or longer (DESIGN.md 4.22 has the figures)."""
        self._check_open()
        held = getattr(self.engine, "grid_u8", None)
        grid = np.array(held, dtype=int) if held is not None else self.grid
        new = checked_cost(type(self).__name__, grid, self.cost if cost is None else cost)
        changed = changed_cells(self.grid, self.cost, grid, new)
        if changed.size == 0:
            return self
        if cost is not None:
            self.cost_device.upload(new.reshape(-1))
        for name in ("pbuf", "obuf", "cbuf"):
            buf = getattr(self, name)
            setattr(self, name, None)
            if buf is not None:
                buf.free()
        self._fields = self._parents = self._owners = self._counts = self._info = None
        self.chosen = np.zeros(0, np.int32)
        e = self.engine
        e.cost_field_repair(self.cost_device, changed, self.set_off, self.ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle,
                            self.ibuf)
        self.grid, self.cost = grid, new
        self.work = e.cost_field_work()
        self.kernel_ms = e.last_kernel_ms()
        return self

    def path_costs(self, paths):
        """paths: a sequence of CellPath, lists of (r, c) or integer cell arrays -- or rows already in HBM as a tuple (d_cells int32
        [n, path_cap], d_len int32 [n], n, path_cap), which are not downloaded -> (float64 [n], int32 [n]): each row's cost under the
        cost map, summed left to right (0 for a one-cell row), and -1; for a row with a step that is no king move between cells of
        the grid NaN and the index of the first such step (0 for an empty row).  Obstacles are not consulted."""
        who = type(self).__name__
        if isinstance(paths, tuple) and len(paths) == 4 and isinstance(paths[0], DevBuf):
            dc, dl, n, cap = paths
            n, cap = int(n), int(cap)
            if n < 1 or cap < 1:
                raise ValueError(f"{who}: path_costs needs n >= 1 and path_cap >= 1 for device rows (got {n}, {cap})")
            self._check_open()
            return self._path_costs(dc, dl, n, cap)
        try:
            paths = list(paths)
        except TypeError:
            raise ValueError(f"{who}: paths must be a sequence of paths or a (d_cells, d_len, n, path_cap) tuple, got {paths!r}") from None
        rows = []
        for i, p in enumerate(paths):
            if isinstance(p, CellPath):
                if p.C != self.cols:
                    raise ValueError(f"{who}: paths[{i}] belongs to a grid of {p.C} columns, not {self.cols}")
                rows.append(np.asarray(p.cells, np.int32))
            elif isinstance(p, np.ndarray) and p.ndim == 1 and p.dtype.kind in "iu":
                rows.append(np.clip(p.astype(np.int64), -1, self.rows * self.cols).astype(np.int32))
            else:
                try:
                    rows.append(np.array([self._cell(f"paths[{i}][{j}]", q, False) for j, q in enumerate(p)], np.int32).reshape(-1))
                except TypeError:
                    raise ValueError(f"{who}: paths[{i}] must be a CellPath, a list of (r, c) pairs or an integer cell array, got {p!r}") from None
        n = len(rows)
        if n == 0:
            return np.zeros(0, np.float64), np.zeros(0, np.int32)
        cap = max(max(len(r) for r in rows), 1)
        cells, lens = np.zeros((n, cap), np.int32), np.zeros(n, np.int32)
        for i, r in enumerate(rows):
            cells[i, :len(r)] = r
            lens[i] = len(r)
        self._check_open()
        dc, dl = self.engine.put(cells), self.engine.put(lens)
        try:
            return self._path_costs(dc, dl, n, cap)
        finally:
            dc.free()
            dl.free()

    def _path_costs(self, d_cells, d_len, n, cap):
        e = self.engine
        dt, db = e.buf(n, np.float64), e.buf(n, np.int32)
        try:
            e.cost_paths(self.cost_device, n, cap, d_cells, d_len, dt, db)
            self.path_costs_kernel_ms = e.last_kernel_ms()
            return dt.download(), db.download()
        finally:
            dt.free()
            db.free()
