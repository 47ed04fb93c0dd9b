"""Clearance: the exact distance from every cell of a grid to the nearest obstacle (pf_clearance_field), obstacles inflated by a
robot's radius, and how close path rows (pf_clearance_paths) and straight segments (pf_clearance_segments) pass.  The field stays
in HBM (`d2_device`); `d2` downloads it once.  `refresh` computes it again after `engine.update_grid`.  Everything is integer:
squared distances between cell centres, no tolerance anywhere.  `widest` turns the field into widest-path fields
(pf_clearance_widest): how large a robot gets from a source to every cell, which cells a robot of a given radius reaches, and
(`widest_path`) the shortest route among those that keep furthest from the walls."""
import math

import numpy as np

from ._field import Field
from ._lib import PathfitError
from .dist_field import DistanceField
from .engine import Engine
from .paths import CellPath

PF_CLEAR_NONE = 2 ** 31 - 1                                           # d2 on a map without an obstacle (include/pathfit.h)


def margin_to_sq(margin):
    """The smallest integer n with math.sqrt(n) >= margin: d2 < n exactly where sqrt(d2) < margin, which is helper.py:76-78's test
    for a safety penalty at min_safe_distance = margin."""
    try:
        m = float(margin)
    except (TypeError, ValueError):
        m = math.nan
    if isinstance(margin, bool) or not (0.0 < m < 46340.0):
        raise ValueError(f"Clearance: margin must be a number in (0, 46340), got {margin!r}")
    n = int(math.ceil(m * m))
    while n > 0 and math.sqrt(n - 1) >= m:
        n -= 1
    while math.sqrt(n) < m:
        n += 1
    return n


def cost_map_of(d2, grid, margin=None, margin_sq=None, weight=1.0):
    """Clearance.cost_map on a squared-distance field d2 and its grid, both [R, C] (numpy alone: no device)."""
    if (margin is None) == (margin_sq is None):
        raise ValueError("Clearance: give exactly one of margin and margin_sq")
    if margin is not None:
        try:
            m = float(margin)
        except (TypeError, ValueError):
            m = math.nan
        if isinstance(margin, bool) or not (0.0 < m < 46340.0):
            raise ValueError(f"Clearance: margin must be a number in (0, 46340), got {margin!r}")
    else:
        m = math.sqrt(Clearance._margin_sq(None, margin_sq, 1))
    try:
        w = float(weight)
    except (TypeError, ValueError):
        w = math.nan
    if isinstance(weight, bool) or not (0.0 <= w < math.inf):
        raise ValueError(f"Clearance: weight must be a finite number >= 0, got {weight!r}")
    d2, grid = np.asarray(d2), np.asarray(grid)
    if d2.shape != grid.shape or d2.ndim != 2:
        raise ValueError(f"Clearance: the field has shape {d2.shape}, the grid has {grid.shape}")
    out = np.ones(d2.shape, np.float64)
    near = (grid != 1) & (d2 != PF_CLEAR_NONE)
    out[near] = np.minimum(1.0 + w * np.maximum(0.0, m - np.sqrt(d2[near].astype(np.float64))) ** 2, float(2 ** 20))
    return out


class WidestField(Field):
    """What Clearance.widest returns: w[b, r, c] = the largest margin_sq with which a robot gets from a source of set b to (r, c)
    (0: not at all), kept in HBM (`w_device`, int32 [B, R * C]); `info` int64 [B, 4] = (sources that counted, cells reached, the
    smallest w >= 1, the smallest cell id that attains it; -1, -1 when nothing is reached)."""
    _bufs = ("w_device",)

    def __init__(self, clearance, w_device, info, kernel_ms):
        self.clearance, self.w_device, self.info, self.kernel_ms = clearance, w_device, info, kernel_ms
        self.B, self.rows, self.cols = int(info.shape[0]), clearance.rows, clearance.cols
        self._w = None

    @property
    def w(self):
        """int32 [B, R, C], downloaded on first use."""
        if self._w is None:
            if self.w_device is None:
                raise PathfitError("Clearance: the widest-path field is closed")
            self._w = self.w_device.download().reshape(self.B, self.rows, self.cols)
        return self._w

    @property
    def radius(self):
        """float64 [B, R, C]: the square root of w, inf where w is PF_CLEAR_NONE (a map without an obstacle)."""
        w = self.w
        out = np.sqrt(w.astype(np.float64))
        out[w == PF_CLEAR_NONE] = np.inf
        return out

    def at(self, b, cell):
        """w[b] at one cell id, read from HBM alone when nothing was downloaded yet."""
        if self._w is not None:
            return int(self._w.reshape(self.B, -1)[int(b), int(cell)])
        if self.w_device is None:
            raise PathfitError("Clearance: the widest-path field is closed")
        return int(self.w_device.read(int(b) * self.rows * self.cols + int(cell), 1)[0])

    def reachable(self, margin=None, margin_sq=None):
        """bool [B, R, C]: the cells a robot of that margin reaches from a source of the set, w >= margin_sq (margin as in
        Clearance.inflated)."""
        return self.w >= Clearance._margin_sq(margin, margin_sq, 1)


class Clearance(Field):
    """d2[r, c] = the squared Euclidean distance between cell centres to the nearest obstacle cell (grid value 1), 0 on an obstacle,
    PF_CLEAR_NONE on a map without one.  border=True: the cells just outside the grid count as obstacles too (the reference's
    safety term does not: helper.py:67-80).  nearest=True also keeps the nearest obstacle cell per cell (the smallest id on a tie);
    it never names the border."""
    _bufs = ("d2_device", "near_device", "ibuf")

    def __init__(self, grid, border=False, nearest=False, engine=None):
        self._set_grid(grid)
        self.border, self.want_nearest = bool(border), bool(nearest)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        self.d2_device = self.near_device = self.ibuf = None
        self.d2_device = self.engine.buf(self.rows * self.cols, np.int32)
        if self.want_nearest:
            self.near_device = self.engine.buf(self.rows * self.cols, np.int32)
        self.ibuf = self.engine.buf(4, np.int64)
        self.refresh()

    def refresh(self):
        """Compute the field of the map the engine holds now (after engine.update_grid); everything downloaded before is dropped."""
        self._check_open()
        self._d2 = self._near = None
        held = getattr(self.engine, "grid_u8", None)
        if held is not None:
            self.grid = np.array(held, dtype=int)
        self.engine.clearance_field(self.d2_device, self.border, self.near_device, self.ibuf)
        self.kernel_ms = self.engine.last_kernel_ms()
        self.info = self.ibuf.download()
        self.obstacle_cells, self.free_cells = int(self.info[0]), int(self.info[1])
        v = int(self.info[3])
        self.most_open = ((v // self.cols, v % self.cols), int(self.info[2])) if v >= 0 else (None, -1)   # ((r, c), d2) of the free cell furthest from any obstacle
        return self

    def _check_open(self):
        if self.d2_device is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the field is closed")

    @property
    def d2(self):
        """int32 [R, C], downloaded on first use."""
        if self._d2 is None:
            self._check_open()
            self._d2 = self.d2_device.download().reshape(self.rows, self.cols)
        return self._d2

    @property
    def distance(self):
        """float64 [R, C]: the square root of d2, inf where d2 is PF_CLEAR_NONE."""
        d2 = self.d2
        out = np.sqrt(d2.astype(np.float64))
        out[d2 == PF_CLEAR_NONE] = np.inf
        return out

    @property
    def nearest(self):
        """int32 [R, C]: the id of the nearest obstacle cell inside the grid (-1 without any); needs nearest=True."""
        if not self.want_nearest:
            raise PathfitError(f"{type(self).__name__}: the nearest obstacles were not asked for (construct with nearest=True)")
        if self._near is None:
            self._check_open()
            self._near = self.near_device.download().reshape(self.rows, self.cols)
        return self._near

    # ------------------------------------------------------------------ margins
    @staticmethod
    def _margin_sq(margin, margin_sq, least):
        if (margin is None) == (margin_sq is None):
            raise ValueError("Clearance: give exactly one of margin and margin_sq")
        if margin is not None:
            return max(margin_to_sq(margin), least)
        try:
            ok = not isinstance(margin_sq, bool) and int(margin_sq) == margin_sq and least <= int(margin_sq) <= PF_CLEAR_NONE
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"Clearance: margin_sq must be an integer in [{least}, 2^31 - 1], got {margin_sq!r}")
        return int(margin_sq)

    def inflated(self, margin=None, margin_sq=None):
        """The grid with 1 wherever d2 < margin_sq (a marker 2 / 3 on such a cell becomes 1) and the original value elsewhere: the
        map a robot of that radius plans on, for Engine(...) or update_grid.  margin (a distance) means margin_sq = the smallest n
        with sqrt(n) >= margin; margin_sq = 1 returns the original obstacle set.  Runs in numpy on the downloaded field."""
        msq = self._margin_sq(margin, margin_sq, 1)
        out = self.grid.copy()
        out[self.d2 < msq] = 1
        return out

    def cost_map(self, margin=None, margin_sq=None, weight=1.0):
        """float64 [R, C] for CostField: 1 + weight * max(0, m - sqrt(d2))^2 on a free cell, clipped to 2^20, with m = margin when
        given, else sqrt(margin_sq); 1 on obstacles and on a map without obstacles.  Cells nearer than m to an obstacle grow dearer
        with the square of the shortfall; cells at least m away cost 1.  This is the ADDITIVE form of the safety term: a route's
        cost is its length plus the penalties it collects.  It is NOT the reference's fitness, which divides the safety penalty by
        the path length (helper.py:67-80).  Runs in numpy on the downloaded field."""
        return cost_map_of(self.d2, self.grid, margin, margin_sq, weight)

    # ------------------------------------------------------------------ path rows
    def _rows(self, paths):
        try:
            paths = list(paths)
        except TypeError:
            raise ValueError(f"Clearance: paths must be a sequence of paths, got {paths!r}") from None
        RC, out = self.rows * self.cols, []
        for i, p in enumerate(paths):
            if isinstance(p, CellPath):
                if p.C != self.cols:
                    raise ValueError(f"Clearance: paths[{i}] belongs to a grid of {p.C} columns, not {self.cols}")
                a = np.asarray(p.cells, np.int64)
            elif isinstance(p, np.ndarray) and p.ndim == 1 and p.dtype.kind in "iu":
                a = p.astype(np.int64)
            else:
                try:
                    a = np.array([self._cell(f"paths[{i}][{j}]", q, True) for j, q in enumerate(p)], np.int64)
                except TypeError:
                    raise ValueError(f"Clearance: paths[{i}] must be a CellPath, a list of (r, c) pairs or an int32 cell array, got {p!r}") from None
            bad = np.flatnonzero((a < 0) | (a >= RC))
            if len(bad):
                raise ValueError(f"Clearance: paths[{i}][{int(bad[0])}] = cell {int(a[bad[0]])} is outside the {self.rows}x{self.cols} grid")
            out.append(a.astype(np.int32))
        return out

    def path_clearance(self, paths, margin=None, margin_sq=None):
        """paths: a sequence of CellPath, lists of (r, c) or int32 cell arrays -> (int32 [n, 4], status int32 [n]).  Per path: the
        smallest d2 over its cells, the position of the first cell that attains it, the number of cells with d2 < margin_sq and the
        position of the first such cell (-1: none).  An empty path gives (PF_CLEAR_NONE, -1, 0, -1) and status 1."""
        msq = self._margin_sq(margin, margin_sq, 0)
        rows = self._rows(paths)
        n = len(rows)
        if n == 0:
            return np.zeros((0, 4), np.int32), np.zeros(0, np.int32)
        cap = max(max(len(r) for r in rows), 1)
        cells, lens = np.zeros((n, cap), np.int32), np.zeros(n, np.int32)
        for i, r in enumerate(rows):
            cells[i, :len(r)] = r
            lens[i] = len(r)
        self._check_open()
        e = self.engine
        dc, dl = e.put(cells), e.put(lens)
        try:
            return self._paths(dc, dl, n, cap, msq)
        finally:
            dc.free()
            dl.free()

    def path_clearance_device(self, d_cells, d_len, n, path_cap, margin=None, margin_sq=None):
        """path_clearance on rows already in HBM (d_cells int32 [n, path_cap], d_len int32 [n]: a solver's population rows, a trace's
        output); the rows are not downloaded.  A row with a length outside [1, path_cap] or a cell outside the grid has status 1."""
        msq = self._margin_sq(margin, margin_sq, 0)
        n, path_cap = int(n), int(path_cap)
        if n < 1 or path_cap < 1:
            raise ValueError(f"Clearance: path_clearance_device needs n >= 1 and path_cap >= 1 (got {n}, {path_cap})")
        self._check_open()
        return self._paths(d_cells, d_len, n, path_cap, msq)

    def _paths(self, d_cells, d_len, n, path_cap, msq):
        e = self.engine
        do, ds = e.buf((n, 4), np.int32), e.buf(n, np.int32)
        try:
            e.clearance_paths(self.d2_device, n, path_cap, d_cells, d_len, msq, do, ds)
            self.paths_kernel_ms = e.last_kernel_ms()
            return do.download(), ds.download()
        finally:
            do.free()
            ds.free()

    # ------------------------------------------------------------------ segments
    def segment_clearance(self, pairs, touched=False):
        """pairs ((r, c), (r, c)) -> (int32 [n], list): the smallest d2 over the cells the straight segment between the two centres
        crosses (touched=True: and the cells it only touches in a corner), and the cell of smallest id that attains it as (r, c).
        An endpoint outside the grid gives PF_CLEAR_NONE and None."""
        try:
            pairs = list(pairs)
        except TypeError:
            raise ValueError(f"Clearance: pairs must be a list of ((r, c), (r, c)), got {pairs!r}") from None
        n = len(pairs)
        ids = np.empty((2, max(n, 1)), np.int32)
        for i, pr in enumerate(pairs):
            try:
                ok = not isinstance(pr, (str, bytes)) and len(pr) == 2
            except TypeError:
                ok = False
            if not ok:
                raise ValueError(f"Clearance: pairs[{i}] must be two (r, c) pairs, got {pr!r}")
            ids[0, i], ids[1, i] = self._cell(f"pairs[{i}][0]", pr[0], False), self._cell(f"pairs[{i}][1]", pr[1], False)
        if n == 0:
            return np.zeros(0, np.int32), []
        self._check_open()
        e = self.engine
        bufs = [e.put(ids[0, :n]), e.put(ids[1, :n]), e.buf(n, np.int32), e.buf(n, np.int32)]
        try:
            e.clearance_segments(self.d2_device, bufs[0], bufs[1], n, bufs[2], bufs[3], touched)
            self.segments_kernel_ms = e.last_kernel_ms()
            dmin, at = bufs[2].download(), bufs[3].download()
        finally:
            for b in bufs:
                b.free()
        return dmin, [None if x < 0 else (int(x) // self.cols, int(x) % self.cols) for x in at]

    # ------------------------------------------------------------------ widest paths
    def _source_sets(self, sources):
        """One (r, c), a list of cells (one set) or a list of lists (B sets) -> a list of int32 id arrays."""
        def is_seq(x):
            return not isinstance(x, (str, bytes)) and hasattr(x, "__len__") and hasattr(x, "__getitem__")

        def is_num(x):
            return isinstance(x, (int, np.integer)) and not isinstance(x, bool)
        bad = ValueError(f"Clearance: sources must be an (r, c) pair, a list of such pairs or a list of such lists, got {sources!r}")
        if not is_seq(sources):
            raise bad
        if len(sources) == 0:
            raise ValueError("Clearance: sources is empty")
        first = sources[0]
        if is_num(first):
            return [np.array([self._pair("sources", sources)], np.int32)]
        if not is_seq(first):
            raise bad
        if len(first) == 0 or is_seq(first[0]):
            sets, names = list(sources), [f"sources[{b}]" for b in range(len(sources))]
        elif is_num(first[0]):
            sets, names = [sources], ["sources"]
        else:
            raise bad
        out = []
        for name, cells in zip(names, sets):
            if not is_seq(cells):
                raise ValueError(f"Clearance: {name} must be a list of (r, c) pairs, got {cells!r}")
            if len(cells) == 0:
                raise ValueError(f"Clearance: {name} is empty")
            out.append(np.array([self._pair(f"{name}[{j}]", p) for j, p in enumerate(cells)], np.int32))
        return out

    def _pair(self, what, p):
        try:
            ok = not isinstance(p, (str, bytes)) and len(p) == 2
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f"Clearance: {what} must be an (r, c) pair, got {p!r}")
        return self._cell(what, p, True)

    def widest(self, sources, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True):
        """sources: one (r, c), a list of cells (one set) or a list of lists (B sets) -> a WidestField: w[b, r, c] = the largest
        margin_sq with which a robot gets from a source of set b to (r, c) under the move policy, 0 where none does.  A move's
        capacity is the smaller d2 of its two cells (and of the two side cells, for a diagonal near an obstacle under the restricted
        policy); a walk's is its smallest move's.  w >= t exactly where Components(inflated(margin_sq=t)) joins the cell to a source."""
        sets = self._source_sets(sources)
        off = np.zeros(len(sets) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in sets])
        # every argument is checked: the device
        self._check_open()
        e, B = self.engine, len(sets)
        wbuf = e.buf(B * self.rows * self.cols, np.int32)
        ibuf = e.buf(B * 4, np.int64)
        try:
            e.clearance_widest(self.d2_device, off, np.concatenate(sets), wbuf, allow_diagonal_moves, restrict_diagonal_near_obstacle, ibuf)
            return WidestField(self, wbuf, ibuf.download().reshape(B, 4), e.last_kernel_ms())
        except Exception:
            wbuf.free()
            raise
        finally:
            ibuf.free()

    def max_margin(self, source, target, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True):
        """-> (w, sqrt(w)): the largest margin_sq with which a robot gets from source to target (0: not at all; PF_CLEAR_NONE and
        inf on a map without an obstacle).  A robot fits iff its margin_sq <= w."""
        s, t = self._pair("source", source), self._pair("target", target)
        f = self.widest([(s // self.cols, s % self.cols)], allow_diagonal_moves, restrict_diagonal_near_obstacle)
        try:
            w = f.at(0, t)
        finally:
            f.close()
        return w, (math.inf if w == PF_CLEAR_NONE else math.sqrt(w))

    def _routes(self, msq, source, targets, ad, rs):
        """DijkstraSolver.solve()'s paths from cell id `source` to the cell ids `targets` on inflated(margin_sq=msq) with the START
        marker on the source (the TARGET marker too, for one target): a temporary engine, one DistanceField, one trace."""
        g = self.inflated(margin_sq=msq)
        g[g > 1] = 0
        g.reshape(-1)[source] = 2
        if len(targets) == 1 and targets[0] != source:
            g.reshape(-1)[targets[0]] = 3
        e = Engine(g)
        try:
            df = DistanceField(g, [(source // self.cols, source % self.cols)], ad, rs, engine=e)
            try:
                return df.paths([(int(t) // self.cols, int(t) % self.cols) for t in targets], k=0)
            finally:
                df.close()
        finally:
            e.close()

    def widest_paths(self, source, targets, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True):
        """-> (a list of CellPath, int32 [n]): for each target the shortest route among the widest ones from source -- the path
        DijkstraSolver(...).solve() returns on inflated(margin_sq=w[target]), cell for cell -- and its w; an empty path and 0 where no
        robot gets through.  One widest-path field serves every target; targets that share a threshold w share one distance field
        on one inflated map, so the cost grows with the number of DISTINCT thresholds among the targets (a temporary engine, a
        field and a trace each)."""
        s = self._pair("source", source)
        try:
            targets = list(targets)
        except TypeError:
            raise ValueError(f"Clearance: targets must be a list of (r, c) pairs, got {targets!r}") from None
        ids = [self._pair(f"targets[{i}]", p) for i, p in enumerate(targets)]
        ad, rs = bool(allow_diagonal_moves), bool(restrict_diagonal_near_obstacle)
        if not ids:
            return [], np.zeros(0, np.int32)
        f = self.widest([(s // self.cols, s % self.cols)], ad, rs)
        try:
            ws = np.array([f.at(0, t) for t in ids], np.int32) if len(ids) <= 4 else f.w.reshape(-1)[ids].astype(np.int32)
        finally:
            f.close()
        paths = [CellPath(np.zeros(0, np.int32), self.cols) for _ in ids]
        for msq in sorted(set(int(x) for x in ws if x > 0)):
            group = [i for i, x in enumerate(ws) if x == msq]
            for i, p in zip(group, self._routes(msq, s, [ids[i] for i in group], ad, rs)):
                paths[i] = p
        return paths, ws

    def widest_path(self, source, target, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True):
        """-> (CellPath, w): widest_paths for one target; ([], 0) when no robot gets through, the one-cell path when source ==
        target (on a free cell)."""
        self._pair("source", source)
        self._pair("target", target)
        paths, ws = self.widest_paths(source, [target], allow_diagonal_moves, restrict_diagonal_near_obstacle)
        return (paths[0], int(ws[0])) if ws[0] > 0 else ([], 0)
