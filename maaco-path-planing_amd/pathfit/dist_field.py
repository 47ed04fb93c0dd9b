"""DistanceField: exact shortest-path lengths from K source cells to every cell of a grid (pf_dist_field_batch) -- the cost-to-go
map of many agents walking to one goal, reachability masks, admissible heuristics, a choice among targets.  The fields stay in HBM
(`buf`); `fields` downloads them once.  `paths` turns a field into routes: DijkstraSolver.solve()'s path from a source to each
of many targets, cell for cell, out of one parent map (`parents`, pf_dist_field_parents) and one pointer chase per target
(pf_dist_field_paths)."""
import numpy as np

from ._batch import _cells
from ._field import Field
from ._lib import PathfitError
from .engine import Engine
from .env import TARGET_NODE_VAL, find_marker
from .paths import CellPath

MOVE_DR = (0, 0, 1, -1, 1, 1, -1, -1)      # helper.py:30-36 move order: parent code k means cell = parent + (MOVE_DR[k], MOVE_DC[k])
MOVE_DC = (1, -1, 0, 0, 1, -1, 1, -1)
PARENT_SOURCE, PARENT_NONE = 8, 255


class DistanceField(Field):
    """fields[k, r, c] = the length of the shortest path from sources[k] to (r, c) under the move policy (inf: an obstacle, or out
    of reach), bit for bit what DijkstraSolver's relaxation leaves.  sources: (r, c) pairs, None = the grid's target marker."""
    _bufs = ("buf", "pbuf")

    def __init__(self, grid, sources=None, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        who = type(self).__name__
        self._set_grid(grid)
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
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        self._fields = None
        self._parents, self.pbuf = None, None
        self.chosen = np.zeros(0, np.int32)
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

    # ------------------------------------------------------------------ routing trees
    def _parent_buf(self):
        """The parent maps in HBM (uint8 [K, R, C]), computed on first use."""
        self._check_open()
        if self.pbuf is None:
            pbuf = self.engine.buf((self.K, self.rows, self.cols), np.uint8)
            try:
                self._compute_parents(pbuf)
            except Exception:
                pbuf.free()
                raise
            self.pbuf = pbuf
            self.parents_kernel_ms = self.engine.last_kernel_ms()
        return self.pbuf

    def _compute_parents(self, pbuf):
        """The parent maps of `buf` into pbuf (CostField computes them under its cost map)."""
        self.engine.dist_field_parents(self.K, self.buf, pbuf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)

    @property
    def parents(self):
        """uint8 [K, R, C], computed and downloaded on first use: 0..7 the move (helper.py:30-36 order) of the last step of
        DijkstraSolver.solve()'s path from sources[k] into the cell (cell = parent + move), 8 at the source, 255 where no route ends."""
        if self._parents is None:
            self._parents = self._parent_buf().download()
        return self._parents

    def _k_checked(self, k):
        return self._index("k", k, self.K)

    def _target_ids(self, targets):
        return self._cell_ids("targets", targets)

    def next_hop(self, k, cell):
        """The cell before `cell` (r, c) on the path from sources[k], i.e. an agent's next step towards that source; None at the
        source itself and where no route ends (an obstacle, out of reach)."""
        k = self._k_checked(k)
        cid = int(self._target_ids([cell])[0])
        if self._parents is not None:
            code = int(self._parents.reshape(-1)[k * self.rows * self.cols + cid])
        else:
            code = int(self._parent_buf().read(k * self.rows * self.cols + cid, 1)[0])
        if code > 7:
            return None
        return (cid // self.cols - MOVE_DR[code], cid % self.cols - MOVE_DC[code])

    def _trace(self, ids, kidx, reverse, path_cap):
        """One trace of the cells `ids` (kidx: int32 field per query, or None = the nearest source), once more at R * C cells per row
        if a path outgrows the row (a Dijkstra path visits a cell once) -> (cells, len, status, chosen) device buffers, row capacity."""
        e, n, full = self.engine, len(ids), self.rows * self.cols
        pbuf = self._parent_buf()
        dt = e.put(ids, np.int32)
        dk = e.put(kidx, np.int32) if kidx is not None else None
        dl, dst, dch = e.buf(n, np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
        cap = int(path_cap) if path_cap else e.default_path_cap()
        while True:
            dc = e.buf((n, cap), np.int32)
            e.dist_field_paths(self.K, pbuf, dt, n, cap, dc, dl, dst, dk, self.buf, reverse, dch)
            self.trace_kernel_ms = e.last_kernel_ms()
            if path_cap or cap >= full or not (dst.download() == 3).any():
                break
            dc.free()
            cap = full
        dt.free()
        if dk is not None:
            dk.free()
        return dc, dl, dst, dch, cap

    def paths(self, targets, k=None, reverse=False, path_cap=None):
        """DijkstraSolver.solve()'s path from a source to each of `targets` ((r, c) pairs) -> a list of CellPath, empty where no
        route ends (an obstacle, out of reach).  k: an int (every target from sources[k]), a sequence (one per target) or None (each
        target from its nearest source, the lowest k on a tie); `chosen` holds the k's of the last call.  reverse: target -> source,
        the order an agent walks to the goal.  path_cap: cells per row (default: the engine's, and once more at R * C where a path
        outgrows it); a path longer than a given path_cap is a PathfitError."""
        who = type(self).__name__
        ids = self._target_ids(targets)
        n = len(ids)
        if k is None:
            kidx = None
        elif np.ndim(k) == 0:
            kidx = np.full(n, self._k_checked(k), np.int32)
        else:
            ks = list(k)
            if len(ks) != n:
                raise ValueError(f"{who}: {len(ks)} k for {n} targets")
            kidx = np.array([self._k_checked(v) for v in ks], np.int32).reshape(n)
        if path_cap is not None and int(path_cap) < 1:
            raise ValueError(f"{who}: path_cap must be >= 1")
        return self._paths_of(ids, kidx, reverse, path_cap)

    def _paths_of(self, ids, kidx, reverse, path_cap):
        """paths() once every argument is checked: the device."""
        who, n = type(self).__name__, len(ids)
        self._check_open()
        if n == 0:
            self.chosen = np.zeros(0, np.int32)
            return []
        dc, dl, dst, dch, cap = self._trace(ids, kidx, reverse, path_cap)
        try:
            st, lens = dst.download(), dl.download()
            if (st == 3).any():
                raise PathfitError(f"{who}: {int((st == 3).sum())} paths hold more than path_cap = {cap} cells")
            self.chosen = dch.download()
            self.status = st
            cells = dc.download() if lens.any() else np.zeros((n, 1), np.int32)
            return [CellPath(cells[i, :lens[i]].copy(), self.cols) for i in range(n)]
        finally:
            for b in (dc, dl, dst, dch):
                b.free()
