"""DistanceField: exact shortest-path lengths from K source cells to every cell of a grid (pf_dist_field_batch) -- the cost-to-go
map of many agents walking to one goal, reachability masks, admissible heuristics, a choice among targets.  The fields stay in HBM
(`buf`); `fields` downloads them once."""
import numpy as np

from ._batch import _cells
from ._lib import PathfitError
from .engine import Engine
from .env import TARGET_NODE_VAL, find_marker


class DistanceField:
    """fields[k, r, c] = the length of the shortest path from sources[k] to (r, c) under the move policy (inf: an obstacle, or out
    of reach), bit for bit what DijkstraSolver's relaxation leaves.  sources: (r, c) pairs, None = the grid's target marker."""

    def __init__(self, grid, sources=None, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        who = type(self).__name__
        self.grid = np.array(grid, dtype=int)
        if self.grid.ndim != 2:
            raise ValueError(f"{who}: grid must be 2-D")
        self.rows, self.cols = self.grid.shape
        if sources is None:
            try:
                sources = [find_marker(self.grid, TARGET_NODE_VAL, who)]
            except ValueError as ex:
                raise ValueError(str(ex) if str(ex).startswith(f"{who}:") else f"{who}: {ex}") from None
        try:
            sources = list(sources)
        except TypeError:
            raise ValueError(f"{who}: sources must be a list of (r, c) pairs, got {sources!r}") from None
        if not sources:
            raise ValueError(f"{who}: sources is empty")
        self.sources = _cells(who, "sources", sources, len(sources), self.grid)
        self.K = len(self.sources)
        self.allow_diagonal_moves = bool(allow_diagonal_moves)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        if engine is not None and (engine.R, engine.C) != self.grid.shape:
            raise ValueError(f"{who}: the engine's grid has another shape")
        # every argument is checked: the device
        self._own_engine = engine is None
        self.engine = engine if engine is not None else Engine(self.grid)
        self._fields = None
        self.buf = self.engine.buf((self.K, self.rows, self.cols), np.float64)
        ids = np.array([r * self.cols + c for r, c in self.sources], np.int32)
        self.engine.dist_field_batch(ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        self.kernel_ms = self.engine.last_kernel_ms()

    def _check_open(self):
        if self.buf is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the field is closed")

    @property
    def fields(self):
        """float64 [K, R, C], downloaded on first use."""
        if self._fields is None:
            self._check_open()
            self._fields = self.buf.download()
        return self._fields

    def length(self, k, cell):
        """The path length from sources[k] to cell (r, c)."""
        r, c = (int(v) for v in cell)
        if not (0 <= int(k) < self.K and 0 <= r < self.rows and 0 <= c < self.cols):
            raise IndexError(f"{type(self).__name__}: no entry [{k}][{r}, {c}]")
        if self._fields is not None:
            return float(self._fields[int(k), r, c])
        self._check_open()
        return float(self.buf.read((int(k) * self.rows + r) * self.cols + c, 1)[0])

    def reachable(self, k):
        """bool [R, C]: the cells sources[k] can reach."""
        return np.isfinite(self.fields[int(k)])

    def close(self):
        buf, self.buf = getattr(self, "buf", None), None
        if buf is not None:
            buf.free()
        if getattr(self, "_own_engine", False) and getattr(self, "engine", None) is not None:
            self.engine.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
