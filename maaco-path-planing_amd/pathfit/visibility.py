"""Visibility: what a viewpoint sees (pf_visibility_field), how many of a set of watchers see every cell (pf_visibility_count),
the exposure of path rows (pf_visibility_paths) and a cost map that makes CostField / TurnField route out of sight where they can.
The rule is PathSmoother.visible's, exact integer geometry on the segment between the cell centres, evaluated from one cell to all;
it is symmetric, an obstacle is never seen and a viewpoint on an obstacle sees nothing.  The occupancy is the engine's at call
time: Engine.update_grid is seen by the next call."""
import math
from fractions import Fraction

import numpy as np

from ._field import Field
from ._lib import PathfitError
from .engine import DevBuf, Engine
from .paths import CellPath

COST_MAX = float(2 ** 20)                                             # CostField's largest cost of a free cell
RANGE_SQ_MAX = 2 ** 31 - 2                                            # R^2 + C^2 stays below: a larger range is no limit


def range_to_sq(max_range):
    """max_range, a distance in cells between cell centres (None: no limit) -> max_range_sq = floor(max_range^2), or -1.  The
    square is taken in exact rational arithmetic (a float is a rational), so an integer n gives n^2 and a half-integer n + 1/2 gives
    n^2 + n exactly: a cell is within range iff dr^2 + dc^2 <= max_range^2."""
    if max_range is None:
        return -1
    try:
        m = float(max_range)
    except (TypeError, ValueError):
        m = math.nan
    if isinstance(max_range, bool) or not (0.0 <= m < math.inf):
        raise ValueError(f"Visibility: max_range must be None or a finite number >= 0, got {max_range!r}")
    f = Fraction(max_range) if isinstance(max_range, (int, Fraction)) else Fraction(m)
    return min(int(f * f // 1), RANGE_SQ_MAX)


def cost_map_of(exposure, grid, weight):
    """Visibility.cost_map on an exposure map and its grid, both [R, C] (numpy alone: no device)."""
    try:
        w = float(weight)
    except (TypeError, ValueError):
        w = math.nan
    if isinstance(weight, bool) or not (0.0 <= w < math.inf):
        raise ValueError(f"Visibility: weight must be a finite number >= 0, got {weight!r}")
    exposure, grid = np.asarray(exposure), np.asarray(grid)
    if exposure.shape != grid.shape or exposure.ndim != 2:
        raise ValueError(f"Visibility: the exposure map has shape {exposure.shape}, the grid has {grid.shape}")
    out = np.ones(grid.shape, np.float64)
    free = grid != 1
    out[free] = 1.0 + w * exposure[free].astype(np.float64)
    bad = np.argwhere(free & ~((out >= 1.0) & (out <= COST_MAX)))
    if len(bad):
        r, c = (int(v) for v in bad[0])
        raise ValueError(f"Visibility: the cost of the free cell ({r}, {c}), 1 + {w!r} * {int(exposure[r, c])}, leaves [1, 2^20]")
    return out


class Visibility(Field):
    """restrict_diagonal_near_obstacle: a sight line that only touches an obstacle's corner is blocked too (PathSmoother's strict
    rule); False is the permissive one.  `info`, `coverage` and `kernel_ms` describe the last call."""
    _bufs = ("counts_device",)

    def __init__(self, grid, restrict_diagonal_near_obstacle=True, engine=None):
        self._set_grid(grid)
        if self.rows * self.rows + self.cols * self.cols >= 2 ** 31 - 1:
            raise ValueError("Visibility: R^2 + C^2 must stay below 2^31 - 1")
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self.counts_device, self.info, self.coverage, self.status, self.kernel_ms = None, None, None, np.zeros(0, np.int32), 0.0
        self._closed = False
        self._set_engine(engine, Engine)                             # every argument is checked: the device

    def _check_open(self):
        if getattr(self, "_closed", True) or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the field is closed")

    def _views(self, viewpoints):
        """(r, c) pairs, or a CellPath (a patrol route) -> int32 cell ids, at least one."""
        if isinstance(viewpoints, CellPath):
            if viewpoints.C != self.cols:
                raise ValueError(f"Visibility: viewpoints belongs to a grid of {viewpoints.C} columns, not {self.cols}")
            ids = np.asarray(viewpoints.cells, np.int64)
            bad = np.flatnonzero((ids < 0) | (ids >= self.rows * self.cols))
            if len(bad):
                raise ValueError(f"Visibility: viewpoints[{int(bad[0])}] = cell {int(ids[bad[0]])} is outside the {self.rows}x{self.cols} grid")
            ids = ids.astype(np.int32)
        else:
            if isinstance(viewpoints, (str, bytes)):
                raise ValueError(f"Visibility: viewpoints must be a list of (r, c) pairs, got {viewpoints!r}")
            ids = self._cell_ids("viewpoints", viewpoints)
        if len(ids) == 0:
            raise ValueError("Visibility: viewpoints is empty")
        return ids

    # ------------------------------------------------------------------ one mask per viewpoint
    def seen(self, viewpoints, max_range=None):
        """-> bool [K, R, C]: [k, r, c] is True where viewpoints[k] sees (r, c) and the distance between the two centres is at most
        max_range cells (range_to_sq: dr^2 + dc^2 <= floor(max_range^2), exact for integer and half-integer ranges; None: no limit).
        `info` int64 [K, 4] = (cells seen, the largest dr^2 + dc^2 among them, the smallest cell id that attains it, 0);
        (0, -1, -1, 0) for a viewpoint on an obstacle."""
        ids, rsq = self._views(viewpoints), range_to_sq(max_range)
        self._check_open()
        e, K, RC = self.engine, len(ids), self.rows * self.cols
        ds, di = e.buf(K * RC, np.uint8), e.buf(K * 4, np.int64)
        try:
            e.visibility_field(ids, ds, self.restrict_diagonal_near_obstacle, rsq, di)
            self.kernel_ms = e.last_kernel_ms()
            self.info = di.download().reshape(K, 4)
            return ds.download().reshape(K, self.rows, self.cols) != 0
        finally:
            ds.free()
            di.free()

    # ------------------------------------------------------------------ exposure
    def exposure_device(self, viewpoints, max_range=None):
        """The exposure counts left in HBM -> the DevBuf int32 [R * C] (`counts_device`: the object's own, rewritten by the next
        exposure call and freed by close()), for path_exposure and for callers that go on working on the device.  Sets `info` int64
        [4] = (free cells seen, free cells, the largest count, the smallest cell id that attains it) and `coverage`."""
        ids, rsq = self._views(viewpoints), range_to_sq(max_range)
        self._check_open()
        e = self.engine
        if self.counts_device is None:
            self.counts_device = e.buf(self.rows * self.cols, np.int32)
        di = e.buf(4, np.int64)
        try:
            e.visibility_count(ids, self.counts_device, self.restrict_diagonal_near_obstacle, rsq, di)
            self.kernel_ms = e.last_kernel_ms()
            self.info = di.download()
        finally:
            di.free()
        self.coverage = float(self.info[0]) / float(self.info[1]) if self.info[1] > 0 else 0.0
        return self.counts_device

    def exposure(self, viewpoints, max_range=None):
        """-> int32 [R, C]: how many of the viewpoints see each cell (one listed twice counts twice; a CellPath is a patrol route).
        `coverage` = the free cells at least one viewpoint sees / the free cells."""
        return self.exposure_device(viewpoints, max_range).download().reshape(self.rows, self.cols)

    def cost_map(self, viewpoints, weight, max_range=None):
        """float64 [R, C] for CostField(cost=...) and TurnField: 1 + weight * exposure on a free cell, 1 on obstacles: a route's cost
        is its length plus weight per watcher and unit of length spent in sight.  weight must be finite and >= 0 and every free
        cell must stay within CostField's [1, 2^20]: ValueError otherwise.  The sum runs in numpy on the downloaded counts."""
        cost_map_of(np.zeros((1, 1), np.int32), np.zeros((1, 1), int), weight)   # the weight, before the device
        return cost_map_of(self.exposure(viewpoints, max_range), self.grid_now(), weight)

    def grid_now(self):
        held = getattr(self.engine, "grid_u8", None)
        return np.array(held, dtype=int) if held is not None else self.grid

    # ------------------------------------------------------------------ path rows
    def _rows(self, paths):
        try:
            paths = list(paths)
        except TypeError:
            raise ValueError(f"Visibility: paths must be a sequence of paths, got {paths!r}") from None
        RC, out = self.rows * self.cols, []
        for i, p in enumerate(paths):
            if isinstance(p, CellPath):
                if p.C != self.cols:
                    raise ValueError(f"Visibility: paths[{i}] belongs to a grid of {p.C} columns, not {self.cols}")
                a = np.asarray(p.cells, np.int64)
            elif isinstance(p, np.ndarray) and p.ndim == 1 and p.dtype.kind in "iu":
                a = p.astype(np.int64)
            else:
                try:
                    a = np.array([self._cell(f"paths[{i}][{j}]", q) for j, q in enumerate(p)], np.int64)
                except TypeError:
                    raise ValueError(f"Visibility: paths[{i}] must be a CellPath, a list of (r, c) pairs or an int32 cell array, got {p!r}") from None
            bad = np.flatnonzero((a < 0) | (a >= RC))
            if len(bad):
                raise ValueError(f"Visibility: paths[{i}][{int(bad[0])}] = cell {int(a[bad[0]])} is outside the {self.rows}x{self.cols} grid")
            out.append(a.astype(np.int32))
        return out

    def path_exposure(self, paths, counts=None):
        """paths: a sequence of CellPath, lists of (r, c) or int32 cell arrays, scored against `counts` (None: what the last exposure
        call left in HBM; else a DevBuf int32 [R * C] or an integer array [R, C]) -> (totals int64 [n], peaks int64 [n], peak positions
        int64 [n], exposed cells int64 [n]): the sum of the counts over the path's cells, the largest count, the position of the first
        cell that attains it and the number of cells at least one viewpoint sees.  `status` int32 [n]: 0, or 1 for an empty path
        (0, -1, -1, 0)."""
        rows = self._rows(paths)
        own = None
        if counts is None:
            if self.counts_device is None:
                raise ValueError("Visibility: path_exposure needs counts, or an exposure call before it")
            dcount = self.counts_device
        elif isinstance(counts, DevBuf):
            if counts.nbytes != 4 * self.rows * self.cols:
                raise ValueError(f"Visibility: counts holds {counts.nbytes} bytes, the grid needs {4 * self.rows * self.cols}")
            dcount = counts
        else:
            own = np.asarray(counts)
            if own.shape != (self.rows, self.cols) or own.dtype.kind not in "iu":
                raise ValueError(f"Visibility: counts must be an integer array of shape {(self.rows, self.cols)}, got {getattr(own, 'shape', None)} {own.dtype}")
            dcount = None
        n = len(rows)
        if n == 0:
            self.status = np.zeros(0, np.int32)
            return tuple(np.zeros(0, np.int64) for _ in range(4))
        cap = max(max(len(r) for r in rows), 1)
        cells, lens = np.zeros((n, cap), np.int32), np.zeros(n, np.int32)
        for i, r in enumerate(rows):
            cells[i, :len(r)] = r
            lens[i] = len(r)
        self._check_open()
        e = self.engine
        bufs = [e.put(cells), e.put(lens), e.buf((n, 4), np.int64), e.buf(n, np.int32)]
        if dcount is None:
            dcount = e.put(own.astype(np.int32).reshape(-1))
            bufs.append(dcount)
        try:
            e.visibility_paths(dcount, n, cap, bufs[0], bufs[1], bufs[2], bufs[3])
            self.kernel_ms = e.last_kernel_ms()
            out, self.status = bufs[2].download(), bufs[3].download()
        finally:
            for b in bufs:
                b.free()
        return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy()

    def close(self):
        self._closed = True
        super().close()
