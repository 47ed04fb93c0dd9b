"""What MAACOBatch, MPABatch and GABatch share: the argument checks of their constructors (all of them run before the device is touched;
`who` is the class name every message starts with) and the ownership of an object the library keeps on an Engine."""
import numpy as np

from ._lib import PathfitError
from .env import OBSTACLE, START_NODE_VAL, TARGET_NODE_VAL, find_marker


def check_grid_and_seeds(who, grid, seeds, unit, count_name, count):
    """-> (2-D int grid, K seeds in [0, 2^64)); `count` (ants / predators per `unit`) must be >= 1."""
    grid = np.array(grid, dtype=int)
    if grid.ndim != 2:
        raise ValueError(f"{who}: grid must be 2-D")
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError(f"{who}: seeds is empty (one seed per {unit})")
    if any(s < 0 or s >= 1 << 64 for s in seeds):
        raise ValueError(f"{who}: seeds must be in [0, 2^64)")
    if int(count) < 1:
        raise ValueError(f"{who}: {count_name} must be >= 1")
    return grid, seeds


def _cells(who, name, pts, K, grid):
    R, Cc = grid.shape
    out = []
    for k, p in enumerate(pts):
        try:
            r, c = (int(v) for v in p)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {name}[{k}] must be an (r, c) pair, got {p!r}") from None
        if not (0 <= r < R and 0 <= c < Cc):
            raise ValueError(f"{who}: {name}[{k}] = {(r, c)} is outside the {R}x{Cc} grid")
        if grid[r, c] == OBSTACLE:
            raise ValueError(f"{who}: {name}[{k}] = {(r, c)} is on an obstacle")
        out.append((r, c))
    if len(out) != K:
        raise ValueError(f"{who}: {len(out)} {name} for {K} seeds")
    return out


def check_endpoints(who, solver, grid, starts, targets, K):
    """-> (K starts, K targets) as (r, c) pairs; None = the grid's marker for every one (`solver` names it in find_marker's error)."""
    if starts is None:
        starts = [find_marker(grid, START_NODE_VAL, solver)] * K
    if targets is None:
        targets = [find_marker(grid, TARGET_NODE_VAL, solver)] * K
    return _cells(who, "starts", list(starts), K, grid), _cells(who, "targets", list(targets), K, grid)


def cell_ids(engine, who, grid, starts, targets):
    """-> the flat int32 ids of the start and of the target cells, once the engine is known to hold a grid of this shape."""
    if (engine.R, engine.C) != grid.shape:
        raise ValueError(f"{who}: the engine's grid has another shape")
    return tuple(np.array([r * grid.shape[1] + c for r, c in cells], np.int32) for cells in (starts, targets))


class EngineOwned:
    """An object the library owns on `self.engine`: `self._b` is its handle (None before creation and once closed), `_destroy`
    the library symbol that frees it."""
    _destroy = None

    def _ck(self, rc):
        if rc != 0:
            raise PathfitError(self.engine.L.pf_last_error(self.engine.h).decode())

    def _handle(self):
        if not self._b or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the batch is closed")
        return self._b

    def close(self):
        # (a closed Engine has freed its batches already)
        if getattr(self, "_b", None) and getattr(self.engine, "h", None):
            getattr(self.engine.L, self._destroy)(self._b)
        self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
