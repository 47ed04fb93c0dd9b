"""PathSmoother: any-angle smoothing of the 8-connected staircases every solver returns.  `visible` answers "does cell a see cell b?"
(pf_line_of_sight_batch: exact integer geometry on the segment between the cell centres), `smooth` keeps the cells of a path that
forward string pulling needs (pf_smooth_batch) and `smooth_device` does the same on rows that are already in HBM, without a download.
The occupancy is the engine's at call time: Engine.update_grid is seen by the next call."""
import numpy as np

from ._field import Field
from ._lib import PathfitError
from .engine import Engine
from .paths import CellPath


class PathSmoother(Field):
    """restrict_diagonal_near_obstacle: a segment that only touches an obstacle's corner is blocked too (on a single diagonal step
    this is the move policy's corner-cut rule); False is the permissive policy."""

    def __init__(self, grid, restrict_diagonal_near_obstacle=True, engine=None):
        self._set_grid(grid)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self._closed = False
        self.first_block = []
        self.indices, self.lengths, self.turns, self.status = [], np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int32)
        self.kernel_ms = 0.0
        self._set_engine(engine, Engine)                             # every argument is checked: the device

    def _check_open(self):
        if getattr(self, "_closed", True):
            raise ValueError(f"{type(self).__name__}: the smoother is closed")

    # ------------------------------------------------------------------ line of sight
    def visible(self, pairs):
        """pairs ((r, c), (r, c)) -> bool array; `first_block` then holds, per pair, the blocking cell nearest the first endpoint as
        (r, c), or None where the pair is visible.  An endpoint outside the grid sees nothing and has no blocker."""
        self._check_open()
        try:
            pairs = list(pairs)
        except TypeError:
            raise ValueError(f"PathSmoother: pairs must be a list of ((r, c), (r, c)), got {pairs!r}") from None
        n = len(pairs)
        ids = np.empty((2, max(n, 1)), np.int32)
        for i, pr in enumerate(pairs):
            try:
                a, b = pr
            except (TypeError, ValueError):
                raise ValueError(f"PathSmoother: pairs[{i}] must be two (r, c) pairs, got {pr!r}") from None
            if isinstance(pr, (str, bytes)):
                raise ValueError(f"PathSmoother: pairs[{i}] must be two (r, c) pairs, got {pr!r}")
            ids[0, i], ids[1, i] = self._cell(f"pairs[{i}][0]", a, False), self._cell(f"pairs[{i}][1]", b, False)
        if n == 0:
            self.first_block = []
            return np.zeros(0, bool)
        e = self.engine
        bufs = [e.put(ids[0, :n]), e.put(ids[1, :n]), e.buf(n, np.int32), e.buf(n, np.int32)]
        try:
            e.line_of_sight_batch(bufs[0], bufs[1], n, bufs[2], bufs[3], self.restrict_diagonal_near_obstacle)
            self.kernel_ms = e.last_kernel_ms()
            vis, fb = bufs[2].download(), bufs[3].download()
        finally:
            for b in bufs:
                b.free()
        C = self.cols
        self.first_block = [None if x < 0 else (int(x) // C, int(x) % C) for x in fb]
        return vis != 0

    # ------------------------------------------------------------------ string pulling
    def _rows(self, paths):
        """The paths as int32 cell arrays, every cell checked against the grid."""
        try:
            paths = list(paths)
        except TypeError:
            raise ValueError(f"PathSmoother: paths must be a sequence of paths, got {paths!r}") from None
        RC, out = self.rows * self.cols, []
        for i, p in enumerate(paths):
            if isinstance(p, CellPath):
                if p.C != self.cols:
                    raise ValueError(f"PathSmoother: paths[{i}] belongs to a grid of {p.C} columns, not {self.cols}")
                a = p.cells
            elif isinstance(p, np.ndarray) and p.ndim == 1 and p.dtype.kind in "iu":
                a = p.astype(np.int64)
            else:
                try:
                    a = np.array([self._cell(f"paths[{i}][{j}]", q) for j, q in enumerate(p)], np.int64)
                except TypeError:
                    raise ValueError(f"PathSmoother: paths[{i}] must be a CellPath, a list of (r, c) pairs or an int32 cell array, got {p!r}") from None
            bad = np.flatnonzero((a < 0) | (a >= RC))
            if len(bad):
                raise ValueError(f"PathSmoother: paths[{i}][{int(bad[0])}] = cell {int(a[bad[0]])} is outside the {self.rows}x{self.cols} grid")
            out.append(np.asarray(a, np.int32))
        return out

    def smooth(self, paths):
        """paths: a sequence of CellPath, lists of (r, c) or int32 cell arrays -> a list of CellPath holding the waypoints kept.
        `indices` (their positions in each input), `lengths`, `turns`, `status` and `kernel_ms` describe the last call.  An empty
        path gives an empty CellPath and status 1."""
        self._check_open()
        rows = self._rows(paths)
        n = len(rows)
        if n == 0:
            self.indices, self.lengths, self.turns, self.status = [], np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int32)
            return []
        cap = max(max(len(r) for r in rows), 1)
        cells, lens = np.zeros((n, cap), np.int32), np.zeros(n, np.int32)
        for i, r in enumerate(rows):
            cells[i, :len(r)] = r
            lens[i] = len(r)
        e = self.engine
        dc, dl = e.put(cells), e.put(lens)
        try:
            dw, dwl, dst, dss, didx = self._launch(dc, dl, n, cap, cap, True)
            try:
                way, idx, wl = dw.download(), didx.download(), dwl.download()
                stats = dst.download().reshape(n, 2)
                self.status = dss.download()
            finally:
                for b in (dw, dwl, dst, dss, didx):
                    b.free()
        finally:
            dc.free()
            dl.free()
        if (self.status == 3).any():
            raise PathfitError("PathSmoother: internal: a waypoint row overflowed")
        self.indices = [idx[i, :wl[i]].copy() for i in range(n)]
        self.lengths, self.turns = stats[:, 0].copy(), stats[:, 1].astype(np.int64)
        return [CellPath(way[i, :wl[i]].copy(), self.cols) for i in range(n)]

    def smooth_device(self, d_cells, d_len, n, path_cap, way_cap=None):
        """Rows already in HBM (d_cells int32 [n, path_cap], d_len int32 [n]: a solver's population rows, a trace's output) ->
        (d_way_cells [n, way_cap], d_way_len [n], d_stats [n, 2], d_status [n], way_cap), new DevBufs the caller frees; nothing is
        downloaded.  way_cap defaults to path_cap, which cannot overflow."""
        self._check_open()
        n, path_cap = int(n), int(path_cap)
        way_cap = path_cap if way_cap is None else int(way_cap)
        if n < 1 or path_cap < 1 or way_cap < 1:
            raise ValueError(f"PathSmoother: smooth_device needs n >= 1, path_cap >= 1 and way_cap >= 1 (got {n}, {path_cap}, {way_cap})")
        return self._launch(d_cells, d_len, n, path_cap, way_cap, False)[:4] + (way_cap,)

    def _launch(self, d_cells, d_len, n, path_cap, way_cap, want_idx):
        """-> (d_way_cells, d_way_len, d_stats, d_status, d_way_idx or None)"""
        e = self.engine
        made = [e.buf((n, way_cap), np.int32), e.buf(n, np.int32), e.buf((n, 2), np.float64), e.buf(n, np.int32)]
        made.append(e.buf((n, way_cap), np.int32) if want_idx else None)
        try:
            e.smooth_batch(n, path_cap, d_cells, d_len, way_cap, made[0], made[1], made[3], made[4], made[2], self.restrict_diagonal_near_obstacle)
        except Exception:
            for b in made:
                if b is not None:
                    b.free()
            raise
        self.kernel_ms = e.last_kernel_ms()
        return tuple(made)

    def close(self):
        self._closed = True
        super().close()
