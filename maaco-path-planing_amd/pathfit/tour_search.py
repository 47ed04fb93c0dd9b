"""TourSearch: a good order through up to 1024 stops, and the route that follows it -- a pick list, an inspection round, the task
list an Assignment hands one robot -- where Tour's exact optimum stops at 16.  The fields come from the stops chunk by chunk
(pf_dist_field_batch, or pf_cost_field under a cost map), each chunk is gathered into its row block of the stop-to-stop matrix in HBM
(pf_assign_matrix), and the order is searched on the device by pf_tour_improve: best-improvement 2-opt from the nearest-neighbour
order, then rounds of double-bridge perturbations of the incumbent, all starts of a round improved in one call over the one shared
matrix.  The rule reads the matrix's upper triangle only and is identical run to run for a given seed; `route_cost` holds any other
order against it.  `legs` / `path` trace the route through the parent maps of the same fields."""
import collections

import numpy as np

from ._field import Field
from ._lib import PathfitError
from .assignment import chunk_rows
from .cost_field import checked_cost
from .engine import Engine
from .paths import CellPath
from .tour import _mode, join_legs, route_cost

STOPS_MAX = 1024                                                     # PF_TOUR_SEARCH_MAX
MOVES_MAX = 1 << 20
STARTS_MAX = 1 << 16
BIG = 2.0 ** 1000

Improved = collections.namedtuple("Improved", "order value status info")


def mirrored(d):
    """The weights pf_tour_improve reads: the upper triangle of d on both sides, the diagonal 0."""
    u = np.triu(np.asarray(d, np.float64), 1)
    return u + u.T


def last_movable(n, mode):
    return n - 2 if mode == 2 else n - 1


def nearest_neighbour(w, mode):
    """The greedy order over w: from the node it stands on to the nearest middle node not yet visited, the smallest index on a tie."""
    n = len(w)
    left = np.arange(1, n - 1 if mode == 2 else n)
    order = [0]
    while len(left):
        k = int(np.argmin(w[order[-1], left]))                        # (the first smallest: left is ascending)
        order.append(int(left[k]))
        left = np.delete(left, k)
    return order + ([n - 1] if mode == 2 and n > 1 else [])


def double_bridge(order, a, b, d):
    o = [int(v) for v in order]
    return o[:a] + o[b:d] + o[a:b] + o[d:]


def _int_in(who, name, v, lo, hi, none_ok=False):
    if v is None and none_ok:
        return None
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= int(v) <= hi:
        raise ValueError(f"{who}: {name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def _count_check(who, n, mode):
    if n < 1:
        raise ValueError(f"{who}: stops is empty")
    if mode == 2 and n < 2:
        raise ValueError(f"{who}: end='last' needs at least two stops")
    if n > STOPS_MAX:
        raise ValueError(f"{who}: {n} stops; at most {STOPS_MAX} are searched")


def _improve(e, mode, n, dm, shared, orders, cap):
    """One pf_tour_improve call over the start rows `orders` [B, n] -> (Improved, kernel ms)."""
    orders = np.ascontiguousarray(orders, np.int32).reshape(-1, n)
    B = len(orders)
    do = e.put(orders.reshape(-1), np.int32)
    dv, ds, di = e.buf((B, 2), np.float64), e.buf(B, np.int32), e.buf((B, 4), np.int64)
    try:
        e.tour_improve(mode, n, B, shared, dm, cap, do, dv, ds, di)
        ms = e.last_kernel_ms()
        return Improved(do.download().reshape(B, n).astype(np.int32), dv.download().reshape(B, 2), ds.download().reshape(B), di.download().reshape(B, 4)), ms
    finally:
        for b in (do, dv, ds, di):
            b.free()


def search(e, mode, n, dm, w, starts, rounds, seed, cap):
    """The search over the matrix dm holds (w: its mirrored copy on the host) -> dict(order, total, feasible, start_total, history,
    moves, kernel_ms).  Round 0 improves the nearest-neighbour order; each later round improves `starts` double-bridge
    perturbations of the incumbent in one call and keeps the strictly smallest total at the smallest start index."""
    got, ms = _improve(e, mode, n, dm, True, [nearest_neighbour(w, mode)], cap)
    if int(got.status[0]) == 1:
        return dict(order=got.order[0], total=float("inf"), feasible=False, start_total=float("inf"), history=[float("inf")], moves=0, kernel_ms=ms)
    order, best, first = got.order[0], float(got.value[0, 0]), float(got.value[0, 1])
    history, moves = [best], int(got.info[0, 0])
    hi = last_movable(n, mode)
    rng = np.random.default_rng(seed)
    if hi >= 3:
        for _ in range(rounds):
            cuts = [np.sort(rng.choice(np.arange(1, hi + 2), 3, replace=False)) for _ in range(starts)]
            got, t = _improve(e, mode, n, dm, True, [double_bridge(order, *c) for c in cuts], cap)
            ms += t
            moves += int(got.info[:, 0].sum())
            k = int(np.argmin(got.value[:, 0]))                       # (the first smallest)
            if got.value[k, 0] < best:
                best, order = float(got.value[k, 0]), got.order[k]
            history.append(best)
    return dict(order=order, total=best, feasible=True, start_total=first, history=history, moves=moves, kernel_ms=ms)


class TourSearch(Field):
    """stops: (r, c) pairs, at most 1024, stops[0] the start.  end: "open" (the tour ends anywhere), "return" (back to the start) or
    "last" (it ends at stops[-1]).  cost: None (path lengths, pf_dist_field_batch) or an [R, C] cost map as CostField's
    (pf_cost_field).  starts, rounds, seed: `rounds` rounds of `starts` perturbed restarts drawn from np.random.default_rng(seed).
    max_moves: the moves one start may take (None: 16 per stop).

    order: int32 stop indices in visiting order (it begins with 0, does not repeat 0 for "return"); total: its left-to-right sum
    under `matrix`; feasible: False where some stop cannot be reached from another (order is then all -1, total inf: the rule needs
    finite weights).  start_total: the nearest-neighbour order's total; history: the incumbent's total after round 0, 1, ...;
    moves: the 2-opt moves of all starts; matrix: float64 [n, n], the upper triangle of the gathered matrix on both sides (downloaded
    when the search is computed, not on first use: the nearest-neighbour start is found on the host from it)."""
    _bufs = ("buf", "pbuf", "mbuf", "cost_device")
    CHUNK_BYTES = 256 << 20

    def __init__(self, grid, stops, end="open", cost=None, starts=32, rounds=8, seed=0, max_moves=None, allow_diagonal_moves=True,
                 restrict_diagonal_near_obstacle=True, engine=None):
        who = type(self).__name__
        self._set_grid(grid)
        self.mode = _mode(who, end)
        self.end = end
        self.ids = self._cell_ids("stops", stops)
        self.n = len(self.ids)
        _count_check(who, self.n, self.mode)
        self.stops = [(int(v) // self.cols, int(v) % self.cols) for v in self.ids]
        self.cost = None if cost is None else checked_cost(who, self.grid, cost)
        self.starts = _int_in(who, "starts", starts, 1, STARTS_MAX)
        self.rounds = _int_in(who, "rounds", rounds, 0, 1 << 20)
        self.seed = _int_in(who, "seed", seed, 0, (1 << 63) - 1)
        cap = _int_in(who, "max_moves", max_moves, 0, MOVES_MAX, none_ok=True)
        self.max_moves = 16 * self.n if cap is None else cap
        self.allow_diagonal_moves = bool(allow_diagonal_moves)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self.chunk = chunk_rows(self.n, self.rows * self.cols, self.CHUNK_BYTES)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        e = self.engine
        self.cost_device = None if self.cost is None else e.put(self.cost.reshape(-1), np.float64)
        self.buf = e.buf((self.chunk, self.rows, self.cols), np.float64)
        self.mbuf = e.buf((self.n, self.n), np.float64)
        self.pbuf = None
        self._compute()

    def _check_open(self):
        if self.buf is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the tour search is closed")

    def _fields(self, r0):
        """The fields of stops r0 .. r0 + k - 1 into buf (k = the chunk's rows) -> k."""
        e, k = self.engine, min(self.chunk, self.n - r0)
        ids = self.ids[r0:r0 + k]
        if self.cost_device is None:
            e.dist_field_batch(ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        else:
            e.cost_field(self.cost_device, np.arange(k + 1, dtype=np.int32), ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        self._held = r0
        return k

    def _compute(self):
        e, n = self.engine, self.n
        ms = 0.0
        for r0 in range(0, n, self.chunk):
            k = self._fields(r0)
            ms += e.last_kernel_ms()
            e.assign_matrix(k, self.ids, self.buf, self.mbuf, r0, n, False)
            ms += e.last_kernel_ms()
        self.matrix = mirrored(self.mbuf.download().reshape(n, n))
        got = search(e, self.mode, n, self.mbuf, self.matrix, self.starts, self.rounds, self.seed, self.max_moves)
        self.order = np.asarray(got["order"], np.int32)
        self.total, self.feasible, self.start_total = got["total"], got["feasible"], got["start_total"]
        self.history, self.moves = got["history"], got["moves"]
        self.solve_kernel_ms = got["kernel_ms"]
        self.kernel_ms = ms + self.solve_kernel_ms

    def route_cost(self, order):
        """The left-to-right sum of the legs of any order of stop indices under `matrix` (closed by the leg back to its first stop
        for end="return"): what another heuristic's order is compared with; route_cost(self.order) == total.  Host side."""
        who = type(self).__name__
        try:
            seq = [self._index("order[%d]" % i, v, self.n) for i, v in enumerate(order)]
        except TypeError:
            raise ValueError(f"{who}: order must be a sequence of stop indices, got {order!r}") from None
        return route_cost(self.matrix, seq, self.mode)

    def legs(self):
        """One CellPath per leg of the tour in visiting order (for end="return" the last one leads back to the start); [] where the
        tour is infeasible.  Each leg is DistanceField.paths' route from its first stop to its second, cell for cell.  The legs
        are grouped by the chunk of fields their first stop lies in: a parent-map call per chunk and one trace call with a field
        index per query.  A chunk of fields that was released for a later one is computed again."""
        self._check_open()
        if not self.feasible:
            return []
        seq = [int(v) for v in self.order] + ([0] if self.mode == 1 and self.n > 1 else [])
        if len(seq) < 2:
            return []
        e, full = self.engine, self.rows * self.cols
        ad, rs = self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle
        out = {}
        for r0 in sorted(range(0, self.n, self.chunk), key=lambda r: r != self._held):      # the chunk held first: it is not computed again
            mine = [x for x in range(len(seq) - 1) if r0 <= seq[x] < r0 + self.chunk]
            if not mine:
                continue
            k = min(self.chunk, self.n - r0)
            if self._held != r0:
                self._fields(r0)
                if self.pbuf is not None:
                    self.pbuf.free()
                    self.pbuf = None
            if self.pbuf is None:
                pbuf = e.buf((self.chunk, self.rows, self.cols), np.uint8)
                try:
                    if self.cost_device is None:
                        e.dist_field_parents(k, self.buf, pbuf, ad, rs)
                    else:
                        e.cost_field_parents(self.cost_device, k, self.buf, pbuf, ad, rs)
                except Exception:
                    pbuf.free()
                    raise
                self.pbuf = pbuf
            q = len(mine)
            dk = e.put(np.array([seq[x] - r0 for x in mine], np.int32))
            dt = e.put(self.ids[np.array([seq[x + 1] for x in mine])].astype(np.int32))
            dl, dst = e.buf(q, np.int32), e.buf(q, np.int32)
            dcl, cap = None, e.default_path_cap()
            try:
                while True:
                    dcl = e.buf((q, cap), np.int32)
                    e.dist_field_paths(k, self.pbuf, dt, q, cap, dcl, dl, dst, dk, self.buf, False, None)
                    st = dst.download()
                    if cap >= full or not (st == 3).any():
                        break
                    dcl.free()
                    dcl, cap = None, full
                if (st == 3).any():
                    raise PathfitError(f"{type(self).__name__}: {int((st == 3).sum())} legs hold more than {cap} cells")
                lens, cells = dl.download(), dcl.download().reshape(q, cap)
                for y, x in enumerate(mine):
                    out[x] = CellPath(cells[y, :lens[y]].copy(), self.cols)
            finally:
                for b in (dk, dt, dl, dst, dcl):
                    if b is not None:
                        b.free()
        return [out[x] for x in range(len(seq) - 1)]

    def path(self):
        """The legs joined into one CellPath (a shared stop cell is not repeated); empty where the tour is infeasible."""
        return join_legs(self.legs(), self.cols)

    def refresh(self, cost=None):
        """Search the tour again on the map the engine holds now (after engine.update_grid) and, when given, under a new cost map
        (for a search built with one)."""
        who = type(self).__name__
        self._check_open()
        if cost is not None and self.cost is None:
            raise ValueError(f"{who}: refresh(cost) needs a tour search built with a cost map")
        held = getattr(self.engine, "grid_u8", None)
        grid = np.array(held, dtype=int) if held is not None else self.grid
        if self.cost is not None:
            new = checked_cost(who, grid, self.cost if cost is None else cost)
            if cost is not None:
                self.cost = new
                self.cost_device.upload(new.reshape(-1))
        self.grid = grid
        if self.pbuf is not None:
            self.pbuf.free()
            self.pbuf = None
        self._compute()
        return self

    @classmethod
    def solve_matrices(cls, engine, mats, orders=None, end="open", shared=False, max_moves=None):
        """For callers with their own matrices and starts: mats float64 [B, n, n] -- or, with `shared`, one [n, n] for all starts --
        of which the upper triangles are read (entries in [0, 2^1000] or +inf, node 0 the start); orders int [B, n], the start
        rows (None: the nearest-neighbour order of each matrix); one `end` for all -> Improved(order int32 [B, n], value float64
        [B, 2] = (total after, total before), status int32 [B]: 0 a local optimum, 1 not searched (a +inf entry), 2 stopped by
        max_moves (None: 16 n), info int64 [B, 4] = (moves, sweeps, 0, 0))."""
        who = cls.__name__
        mode = _mode(who, end)
        try:
            m = np.ascontiguousarray(mats, np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: mats must be a [B, n, n] array of numbers") from None
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[1] != m.shape[2] or m.shape[0] < 1:
            raise ValueError(f"{who}: mats has shape {m.shape}, not [B, n, n] with B >= 1")
        n = int(m.shape[1])
        _count_check(who, n, mode)
        if shared and m.shape[0] != 1:
            raise ValueError(f"{who}: shared=True takes one [n, n] matrix, got {m.shape[0]}")
        cap = _int_in(who, "max_moves", max_moves, 0, MOVES_MAX, none_ok=True)
        cap = 16 * n if cap is None else cap
        up = np.triu(np.ones((n, n), bool), 1)
        with np.errstate(invalid="ignore"):
            bad = np.argwhere(~(((m >= 0.0) & ((m <= BIG) | (m == np.inf))) | ~up[None]))    # (NaN fails the comparisons)
        if len(bad):
            b, i, j = (int(v) for v in bad[0])
            raise ValueError(f"{who}: mats[{b}, {i}, {j}] = {float(m[b, i, j])!r} is neither +inf nor a number in [0, 2^1000]")
        if orders is None:
            o = np.array([nearest_neighbour(mirrored(a), mode) for a in m], np.int64).reshape(len(m), n)
        else:
            try:
                o = np.array(orders)
                o = o[None] if o.ndim == 1 else o
                ok = o.ndim == 2 and o.shape[1] == n and o.shape[0] >= 1 and o.dtype.kind in "iu"
            except (TypeError, ValueError):
                ok = False
            if not ok or (not shared and o.shape[0] != m.shape[0]):
                raise ValueError(f"{who}: orders must be an integer array [B, n] with a row per matrix (any B >= 1 with shared=True)")
            for b, row in enumerate(o):
                seen = set()
                for p, v in enumerate(row):
                    v = int(v)
                    if not 0 <= v < n or v in seen or (p == 0 and v != 0) or (mode == 2 and p == n - 1 and v != n - 1):
                        raise ValueError(f"{who}: orders[{b}, {p}] = {v}: a start is a permutation of the nodes with node 0 first" +
                                         (" and node n - 1 last" if mode == 2 else ""))
                    seen.add(v)
        dm = engine.put(m.reshape(-1), np.float64)
        try:
            return _improve(engine, mode, n, dm, bool(shared), o, cap)[0]
        finally:
            dm.free()
