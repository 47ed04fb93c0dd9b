"""SpaceTime: planning through a map that changes during the walk.  Time runs in ticks 0..horizon; in a tick a robot waits or makes
one move of the policy.  Moving obstacles (a patrol, a door that is shut for some ticks, another robot whose route is fixed) are
stamped into dynamic occupancy planes in HBM (pf_spacetime_stamp); pf_spacetime_field gives the earliest tick a robot can be on
every cell, pf_spacetime_paths the routes, pf_spacetime_conflicts checks any route against the planes, and plan_fleet plans a
fleet robot by robot.  The static occupancy is the engine's at call time: Engine.update_grid is seen by the next call.  The rule
is DESIGN.md 4.25's: vertex, swap and -- under restrict_diagonal_near_obstacle -- corner conflicts, all tested on the planes."""
import numpy as np

from ._field import Field
from ._lib import PathfitError
from .engine import ST_OK, DevBuf, Engine
from .paths import CellPath

HORIZON_MAX = 2 ** 20
KIND_STATIC, KIND_VERTEX, KIND_SWAP, KIND_CORNER = 1, 2, 3, 4
TICK_EARLIEST, TICK_HOLD = -1, -2


def unpack_planes(words, C):
    """uint64 [..., Wc] plane words -> bool [..., C]: cell c of a row is bit c & 63 of its word c >> 6."""
    w = np.ascontiguousarray(np.asarray(words, np.uint64).astype("<u8"))
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :C].astype(bool)


class SpaceTime(Field):
    """horizon: the last tick T.  restrict_diagonal_near_obstacle / allow_diagonal: the move policy, as DistanceField's.  `info`,
    `status`, `ticks` and `kernel_ms` describe the last call."""
    _bufs = ("occ_device", "reach_device")

    def __init__(self, grid, horizon, restrict_diagonal_near_obstacle=True, allow_diagonal=True, engine=None):
        self._set_grid(grid)
        try:
            ok = int(horizon) == horizon and not isinstance(horizon, bool) and 0 <= int(horizon) <= HORIZON_MAX
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"SpaceTime: horizon must be an integer in [0, 2^20], got {horizon!r}")
        self.horizon = int(horizon)
        self.words_per_row = (self.cols + 63) // 64
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self.allow_diagonal = bool(allow_diagonal)
        self.occ_device, self.reach_device, self.sets = None, None, 0
        self.info, self.status, self.ticks, self.kernel_ms = None, np.zeros(0, np.int32), np.zeros(0, np.int32), 0.0
        self._closed = False
        self._set_engine(engine, Engine)                             # every argument is checked: the device

    # ------------------------------------------------------------------ helpers
    def _check_open(self):
        if getattr(self, "_closed", True) or not getattr(self.engine, "h", None):
            raise PathfitError("SpaceTime: the field is closed")

    def _policy(self):
        return dict(allow_diag=self.allow_diagonal, restrict_corner=self.restrict_diagonal_near_obstacle)

    def _planes(self):
        """The dynamic planes uint64 [T + 1, R, Wc] in HBM, allocated zeroed on first use."""
        self._check_open()
        if self.occ_device is None:
            self.occ_device = self.engine.buf((self.horizon + 1, self.rows, self.words_per_row), np.uint64).zero()
        return self.occ_device

    def _rows(self, what, paths):
        try:
            paths = list(paths)
        except TypeError:
            raise ValueError(f"SpaceTime: {what} must be a sequence of paths, got {paths!r}") from None
        RC, out = self.rows * self.cols, []
        for i, p in enumerate(paths):
            if isinstance(p, CellPath):
                if p.C != self.cols:
                    raise ValueError(f"SpaceTime: {what}[{i}] belongs to a grid of {p.C} columns, not {self.cols}")
                a = np.asarray(p.cells, np.int64)
            elif isinstance(p, np.ndarray) and p.ndim == 1 and p.dtype.kind in "iu":
                a = p.astype(np.int64)
            else:
                try:
                    a = np.array([self._cell(f"{what}[{i}][{j}]", q) for j, q in enumerate(p)], np.int64)
                except TypeError:
                    raise ValueError(f"SpaceTime: {what}[{i}] must be a CellPath, a list of (r, c) pairs or an int32 cell array, got {p!r}") from None
            if len(a) == 0:
                raise ValueError(f"SpaceTime: {what}[{i}] is empty")
            bad = np.flatnonzero((a < 0) | (a >= RC))
            if len(bad):
                raise ValueError(f"SpaceTime: {what}[{i}][{int(bad[0])}] = cell {int(a[bad[0]])} is outside the {self.rows}x{self.cols} grid")
            out.append(a.astype(np.int32))
        return out

    def _start_ticks(self, start_ticks, n):
        if start_ticks is None:
            return np.zeros(n, np.int32)
        try:
            t = np.asarray(start_ticks)
            ok = t.shape == (n,) and t.dtype.kind in "iu"
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"SpaceTime: start_ticks must be {n} integers, one per path, got {start_ticks!r}")
        bad = np.flatnonzero((t < 0) | (t > self.horizon))
        if len(bad):
            raise ValueError(f"SpaceTime: start_ticks[{int(bad[0])}] = {int(t[bad[0]])} is outside [0, {self.horizon}]")
        return t.astype(np.int32)

    @staticmethod
    def _after_end(after_end):
        if after_end not in ("stay", "vanish"):
            raise ValueError(f"SpaceTime: after_end must be 'stay' or 'vanish', got {after_end!r}")
        return after_end == "stay"

    @staticmethod
    def _pad(rows):
        cap = max(len(r) for r in rows)
        cells, lens = np.zeros((len(rows), cap), np.int32), np.zeros(len(rows), np.int32)
        for i, r in enumerate(rows):
            cells[i, :len(r)] = r
            lens[i] = len(r)
        return cells, lens, cap

    # ------------------------------------------------------------------ the planes
    def add(self, obstacles, start_ticks=None, after_end="stay", corners=False):
        """obstacles: a sequence of CellPath, lists of (r, c) or int32 cell arrays; obstacle i is on its cell j at tick start_ticks[i]
        + j (None: 0) and need not move by adjacent cells.  after_end "stay": it keeps its last cell to the horizon; "vanish": it
        leaves the map.  corners: a diagonal step also takes its two corner cells at both ticks (a robot's swept footprint)."""
        rows = self._rows("obstacles", obstacles)
        t0, stay = self._start_ticks(start_ticks, len(rows)), self._after_end(after_end)
        if not rows:
            self.status = np.zeros(0, np.int32)
            return self
        cells, lens, cap = self._pad(rows)
        occ, e = self._planes(), self.engine
        bufs = [e.put(cells), e.put(lens), e.put(t0), e.buf(len(rows), np.int32)]
        try:
            e.spacetime_stamp(self.horizon, occ, len(rows), cap, bufs[0], bufs[1], bufs[3], bufs[2], stay, bool(corners), False)
            self.kernel_ms, self.status = e.last_kernel_ms(), bufs[3].download()
        finally:
            for b in bufs:
                b.free()
        return self

    def add_rows(self, d_cells, d_len, n, path_cap, d_start_ticks=None, after_end="stay", corners=False):
        """Rows where a solver left them in HBM (astar_batch's layout: d_cells int32 [n, path_cap], d_len int32 [n]; d_start_ticks
        int32 [n] or None) -> `status` int32 [n]: 0, or 1 for a bad row (empty, too long, a cell or a start tick out of range), of
        which nothing is stamped."""
        n, path_cap, stay = self._index("n", n, 2 ** 31), self._index("path_cap", path_cap, 2 ** 31), self._after_end(after_end)
        for name, b, need in (("d_cells", d_cells, 4 * n * path_cap), ("d_len", d_len, 4 * n), ("d_start_ticks", d_start_ticks, 4 * n)):
            if b is None and name == "d_start_ticks":
                continue
            if not isinstance(b, DevBuf) or b.nbytes < need:
                raise ValueError(f"SpaceTime: {name} must be a DevBuf of at least {need} bytes")
        if n == 0 or path_cap == 0:
            if n:
                raise ValueError("SpaceTime: path_cap = 0 is outside [1, 2^31)")
            self.status = np.zeros(0, np.int32)
            return self.status
        occ, e = self._planes(), self.engine
        dst = e.buf(n, np.int32)
        try:
            e.spacetime_stamp(self.horizon, occ, n, path_cap, d_cells, d_len, dst, d_start_ticks, stay, bool(corners), False)
            self.kernel_ms, self.status = e.last_kernel_ms(), dst.download()
        finally:
            dst.free()
        return self.status

    def clear(self):
        """Every dynamic obstacle leaves the planes."""
        self._check_open()
        if self.occ_device is not None:
            self.occ_device.zero()
        return self

    def occupancy(self):
        """-> bool [T + 1, R, C]: the dynamic planes (the static map is not in them)."""
        return unpack_planes(self._planes().download().reshape(self.horizon + 1, self.rows, self.words_per_row), self.cols)

    # ------------------------------------------------------------------ arrival fields
    def _sets(self, sources):
        """One set (a list of (r, c) pairs) or a list of sets -> the CSR arrays."""
        if isinstance(sources, (str, bytes)):
            raise ValueError(f"SpaceTime: sources must be a list of (r, c) pairs or a list of such lists, got {sources!r}")
        try:
            sources = list(sources)
        except TypeError:
            raise ValueError(f"SpaceTime: sources must be a list of (r, c) pairs or a list of such lists, got {sources!r}") from None
        if not sources:
            raise ValueError("SpaceTime: sources is empty")
        first = sources[0]
        one = False
        try:
            one = len(first) == 2 and all(int(v) == v for v in first)
        except (TypeError, ValueError):
            pass
        sets = [sources] if one else sources
        off, ids = [0], []
        for b, s in enumerate(sets):
            ids.append(self._cell_ids("sources" if one else f"sources[{b}]", s))
            off.append(off[-1] + len(ids[-1]))
        return np.array(off, np.int32), np.concatenate(ids).astype(np.int32) if off[-1] else np.zeros(0, np.int32)

    def arrival(self, sources, keep=True):
        """sources: one set of (r, c) pairs or a list of sets -> int32 [B, R, C]: the least tick at which a robot that starts on a
        cell of the set at tick 0 can be on the cell, -1 where it cannot within the horizon.  A source on a cell occupied at tick 0
        is skipped.  `info` int64 [B, 4] = (cells reached, the largest arrival tick, the smallest cell id that attains it, 0).
        keep: the reach planes stay in HBM (`reach_device`, B * (T + 1) * R * ceil(C / 64) words) for paths()."""
        off, ids = self._sets(sources)
        occ, e = self._planes(), self.engine
        B, RC, W = len(off) - 1, self.rows * self.cols, self.rows * self.words_per_row
        if self.reach_device is not None:
            self.reach_device.free()
        self.reach_device, self.sets = None, 0
        da, di = e.buf((B, RC), np.int32), e.buf((B, 4), np.int64)
        try:
            dr = e.buf((B, self.horizon + 1, W), np.uint64) if keep else None
            try:
                e.spacetime_field(self.horizon, occ, off, ids, da, d_reach=dr, d_info=di, **self._policy())
            except Exception:
                if dr is not None:
                    dr.free()
                raise
            self.reach_device, self.sets = dr, (B if keep else 0)
            self.kernel_ms = e.last_kernel_ms()
            self.info = di.download().reshape(B, 4)
            return da.download().reshape(B, self.rows, self.cols)
        finally:
            da.free()
            di.free()

    def paths(self, targets, ticks=None, k=None):
        """targets: (r, c) pairs; ticks: None the earliest arrival, "hold" the first tick at which the robot can arrive and stay to
        the horizon, an int or one int per target that tick; k: the source set of each query (None: set 0 when the last arrival
        call had one set, else query q takes set q) -> a list of CellPath (tick + 1 cells, cell j the position at tick j) or None.
        `status` int32 [n]: 0, 1 infeasible, 3 the planes do not belong to this map; `ticks` int32 [n]: the tick used, -1 if none."""
        tg = self._cell_ids("targets", targets)
        n, T = len(tg), self.horizon
        if ticks is None or (isinstance(ticks, str) and ticks == "hold"):
            tk = np.full(n, TICK_EARLIEST if ticks is None else TICK_HOLD, np.int32)
        else:
            try:
                tk = np.asarray(ticks)
                if tk.ndim == 0:
                    tk = np.full(n, tk)
                ok = tk.shape == (n,) and tk.dtype.kind in "iu" and bool(((tk >= 0) & (tk <= T)).all())
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"SpaceTime: ticks must be None, 'hold', an integer in [0, {T}] or one per target, got {ticks!r}")
            tk = tk.astype(np.int32)
        if self.reach_device is None:
            raise ValueError("SpaceTime: paths needs an arrival call with keep=True before it")
        B = self.sets
        if k is None:
            if B != 1 and n != B:
                raise ValueError(f"SpaceTime: k is needed: the last arrival call had {B} sets and there are {n} targets")
            ks = np.zeros(n, np.int32) if B == 1 else np.arange(n, dtype=np.int32)
        else:
            ks = np.full(n, self._index("k", k, B), np.int32) if np.ndim(k) == 0 else np.array([self._index(f"k[{i}]", v, B) for i, v in enumerate(k)], np.int32)
            if len(ks) != n:
                raise ValueError(f"SpaceTime: k must be one set index or {n} of them")
        if n == 0:
            self.status, self.ticks = np.zeros(0, np.int32), np.zeros(0, np.int32)
            return []
        occ, e = self._planes(), self.engine
        cap = T + 1
        bufs = [e.put(ks), e.put(tg), e.put(tk), e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32), e.buf(n, np.int32)]
        try:
            e.spacetime_paths(T, occ, B, self.reach_device, n, bufs[0], bufs[1], cap, bufs[3], bufs[4], bufs[5], bufs[2], bufs[6], **self._policy())
            self.kernel_ms = e.last_kernel_ms()
            lens, self.status, self.ticks = bufs[4].download(), bufs[5].download(), bufs[6].download()
            cells = bufs[3].download().reshape(n, cap)
        finally:
            for b in bufs:
                b.free()
        return [CellPath(cells[q, :lens[q]].copy(), self.cols) if self.status[q] == ST_OK else None for q in range(n)]

    # ------------------------------------------------------------------ conflicts
    def conflicts(self, paths, start_ticks=None, hold=False):
        """paths (as add's obstacles: an A* / MPA / CostField route) walked from start_ticks against the static map, the planes and the
        policy -> (first conflicting tick or -1, kind, the cell entered or -1, conflicting steps), int32 [n] each.  Kinds: 1 static
        (a static obstacle, or a step the policy does not have on the static map), 2 vertex, 3 swap, 4 corner.  hold: the last
        cell is checked at every later tick too.  `status`: 0, or 2 where the path runs past the horizon (checked up to it)."""
        rows = self._rows("paths", paths)
        t0 = self._start_ticks(start_ticks, len(rows))
        n = len(rows)
        if n == 0:
            self.status = np.zeros(0, np.int32)
            return tuple(np.zeros(0, np.int32) for _ in range(4))
        cells, lens, cap = self._pad(rows)
        occ, e = self._planes(), self.engine
        bufs = [e.put(cells), e.put(lens), e.put(t0), e.buf((n, 4), np.int32), e.buf(n, np.int32)]
        try:
            e.spacetime_conflicts(self.horizon, occ, n, cap, bufs[0], bufs[1], bufs[3], bufs[4], bufs[2], bool(hold), **self._policy())
            self.kernel_ms = e.last_kernel_ms()
            out, self.status = bufs[3].download().reshape(n, 4), bufs[4].download()
        finally:
            for b in bufs:
                b.free()
        return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy()

    # ------------------------------------------------------------------ fleets
    def plan_fleet(self, starts, goals, order=None):
        """Prioritised planning: each robot, in `order` (None: as listed), takes the arrival field from its start against the planes
        so far and the route to its goal at the hold tick; the route is stamped with after_end "stay" and corners =
        restrict_diagonal_near_obstacle, so the robots after it keep out of its way and out of its diagonal steps' corners.  A
        robot without a hold tick within the horizon gets None, is not stamped, and the rest go on.  -> (routes, status int32 [n])."""
        s, g = self._cell_ids("starts", starts), self._cell_ids("goals", goals)
        if len(s) != len(g):
            raise ValueError(f"SpaceTime: {len(s)} starts and {len(g)} goals")
        n = len(s)
        if order is None:
            order = list(range(n))
        else:
            try:
                order = [self._index(f"order[{i}]", v, n) for i, v in enumerate(order)]
            except TypeError:
                raise ValueError(f"SpaceTime: order must be a permutation of 0..{n - 1}, got {order!r}") from None
            if sorted(order) != list(range(n)):
                raise ValueError(f"SpaceTime: order must be a permutation of 0..{n - 1}, got {order!r}")
        self._check_open()
        C = self.cols
        routes, status, ms = [None] * n, np.ones(n, np.int32), 0.0
        for i in order:
            self.arrival([(int(s[i]) // C, int(s[i]) % C)])
            ms += self.kernel_ms
            got = self.paths([(int(g[i]) // C, int(g[i]) % C)], "hold")[0]
            ms += self.kernel_ms
            status[i] = self.status[0]
            if got is not None:
                routes[i] = got
                self.add([got], after_end="stay", corners=self.restrict_diagonal_near_obstacle)
                ms += self.kernel_ms
        self.status, self.kernel_ms = status, ms
        return routes, status

    def close(self):
        self._closed = True
        super().close()
