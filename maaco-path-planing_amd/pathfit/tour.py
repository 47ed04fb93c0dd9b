"""Tour: the exact best order through up to 16 stops besides the start, and the route that follows it -- a robot's task list, some
of it ordered (pick up before delivery).  The legs come from one pf_dist_field_batch call (or one pf_cost_field call under a cost
map), the stop-to-stop matrix is gathered out of the fields in HBM (pf_tour_matrix), and the order is the Held-Karp optimum
(pf_tour_solve): bit for bit the minimum over all admissible orders of the legs' left-to-right sum, identical run to run, which a
heuristic's order can be held against (`route_cost`).  `legs` / `path` trace the route through the parent maps of the same fields."""
import numpy as np

from ._planner import Planner, as_matrices, no_bad_entry
from .engine import Engine
from .paths import CellPath

ENDS = {"open": 0, "return": 1, "last": 2}
MIDDLE_MAX = 16


def _mode(who, end):
    if not isinstance(end, str) or end not in ENDS:
        raise ValueError(f"{who}: end must be 'open', 'return' or 'last', got {end!r}")
    return ENDS[end]


def _need(who, n, mode, before):
    """(a, b) pairs, stop a before stop b -> uint32 [n]: bit a of need[b]."""
    try:
        pairs = [tuple(p) for p in before]
    except TypeError:
        raise ValueError(f"{who}: before must be a list of (a, b) index pairs, got {before!r}") from None
    need = np.zeros(n, np.uint32)
    for i, p in enumerate(pairs):
        ok = len(p) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in p)
        if not ok or not (0 <= p[0] < n and 0 <= p[1] < n):
            raise ValueError(f"{who}: before[{i}] = {p!r} is no pair of stop indices in [0, {n})")
        a, b = int(p[0]), int(p[1])
        if a == b:
            raise ValueError(f"{who}: before[{i}] = {(a, b)} puts a stop before itself")
        if b == 0:
            raise ValueError(f"{who}: before[{i}] = {(a, b)} puts a stop before the start")
        if mode == 2 and a == n - 1:
            raise ValueError(f"{who}: before[{i}] = {(a, b)} puts the last stop of end='last' before another")
        need[b] |= np.uint32(1 << a)
    return need


def _count_check(who, n, mode):
    if n < 1:
        raise ValueError(f"{who}: stops is empty")
    if mode == 2 and n < 2:
        raise ValueError(f"{who}: end='last' needs at least two stops")
    most = MIDDLE_MAX + (2 if mode == 2 else 1)
    if n > most:
        raise ValueError(f"{who}: {n} stops; at most {most} are solved exactly with end={[k for k, v in ENDS.items() if v == mode][0]!r}")


def route_cost(matrix, order, mode):
    """The left-to-right float64 sum of the legs of `order` (node indices) under `matrix`, closed by the leg back to order[0] in
    mode 1; 0.0 for fewer than two nodes (and no closing leg)."""
    d = np.asarray(matrix, np.float64)
    seq = [int(v) for v in order]
    if mode == 1 and len(seq) > 1:
        seq = seq + [seq[0]]
    if len(seq) < 2:
        return 0.0
    t = d[seq[0], seq[1]]
    for a, b in zip(seq[1:-1], seq[2:]):
        t = t + d[a, b]
    return float(t)


def join_legs(legs, cols):
    """The legs as one CellPath: a leg that starts on the cell the route stands on does not repeat it."""
    out = []
    for leg in legs:
        cells = [int(v) for v in leg.cells]
        if out and cells and cells[0] == out[-1]:
            cells = cells[1:]
        out.extend(cells)
    return CellPath(np.array(out, np.int32), cols)


class Tour(Planner):
    """stops: (r, c) pairs, stops[0] the start.  end: "open" (the tour ends anywhere), "return" (back to the start) or "last" (it
    ends at stops[-1]).  before: (a, b) index pairs, stop a is visited before stop b.  cost: None (path lengths, pf_dist_field_batch)
    or an [R, C] cost map as CostField's (pf_cost_field).

    order: int32 stop indices in visiting order (it begins with 0, does not repeat 0 for "return"); total: the exact optimum;
    feasible: False where a stop is out of reach or `before` is cyclic (order is then all -1, total inf).  matrix: float64 [n, n],
    downloaded on first use; info: int64 [4] = (finite states of the table, the last middle stop or -1, 0, 0)."""
    _closed, _built = "the tour is closed", "a tour"

    def __init__(self, grid, stops, end="open", before=(), cost=None, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        who = type(self).__name__
        self._set_grid(grid)
        self.mode = _mode(who, end)
        self.end = end
        self.ids = self._cell_ids("stops", stops)
        self.n = len(self.ids)
        _count_check(who, self.n, self.mode)
        self.stops = [(int(v) // self.cols, int(v) % self.cols) for v in self.ids]
        self.need = _need(who, self.n, self.mode, before)
        self._set_cost_and_moves(cost, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        e = self._open(engine, Engine, self.ids, self.n)             # every argument is checked: the device; the fields are one chunk
        self.mbuf = e.buf((self.n, self.n), np.float64)
        self._compute()

    def _compute(self):
        e, n = self.engine, self.n
        ms = self._gather(lambda k, r0: e.tour_matrix(self.ids, self.buf, self.mbuf))
        dt, do, ds, di = e.buf(1, np.float64), e.buf(n, np.int32), e.buf(1, np.int32), e.buf(4, np.int64)
        try:
            e.tour_solve(self.mode, n, 1, self.mbuf, dt, do, ds, self.need, di)
            self.solve_kernel_ms = e.last_kernel_ms()
            self.total = float(dt.download()[0])
            self.order = do.download().astype(np.int32)
            self.feasible = int(ds.download()[0]) == 0
            self.info = di.download().astype(np.int64)
        finally:
            for b in (dt, do, ds, di):
                b.free()
        self.kernel_ms = ms + self.solve_kernel_ms
        self._matrix = None

    @property
    def matrix(self):
        """float64 [n, n], downloaded on first use: matrix[i, j] = the field from stop i at stop j."""
        if self._matrix is None:
            self._check_open()
            self._matrix = self.mbuf.download().reshape(self.n, self.n)
        return self._matrix

    def route_cost(self, order):
        """The left-to-right sum of the legs of any order of stop indices under `matrix` (closed by the leg back to its first stop
        for end="return"): what a heuristic's order is compared with.  Host side."""
        who = type(self).__name__
        try:
            seq = [self._index("order[%d]" % i, v, self.n) for i, v in enumerate(order)]
        except TypeError:
            raise ValueError(f"{who}: order must be a sequence of stop indices, got {order!r}") from None
        return route_cost(self.matrix, seq, self.mode)

    def legs(self):
        """One CellPath per leg of the tour in visiting order (for end="return" the last one leads back to the start); [] where the
        tour is infeasible (Planner._trace: all legs come from one parent-map call over the fields and one trace call)."""
        self._check_open()
        if not self.feasible:
            return []
        seq = [int(v) for v in self.order] + ([0] if self.mode == 1 and self.n > 1 else [])
        return self._trace([(a, int(self.ids[b])) for a, b in zip(seq[:-1], seq[1:])], "legs")

    def path(self):
        """The legs joined into one CellPath (a shared stop cell is not repeated); empty where the tour is infeasible."""
        return join_legs(self.legs(), self.cols)

    @classmethod
    def solve_matrices(cls, engine, mats, end="open", before=()):
        """For callers with their own matrices: mats float64 [B, n, n] (entries >= 0 or +inf, node 0 the start), one `end` and one
        `before` for all -> (totals float64 [B], orders int32 [B, n], status int32 [B] with 1 = infeasible, info int64 [B, 4])."""
        who = cls.__name__
        mode = _mode(who, end)
        m = as_matrices(who, "mats", mats, "n", "n")
        B, n = int(m.shape[0]), int(m.shape[1])
        _count_check(who, n, mode)
        need = _need(who, n, mode, before)
        off = ~np.eye(n, dtype=bool)
        no_bad_entry(who, "mats", m, ~((m >= 0.0) | ~off[None]), "neither >= 0 nor +inf")      # (NaN fails the comparison)
        dm = engine.put(m.reshape(-1), np.float64)
        dt, do, ds, di = engine.buf(B, np.float64), engine.buf((B, n), np.int32), engine.buf(B, np.int32), engine.buf((B, 4), np.int64)
        try:
            engine.tour_solve(mode, n, B, dm, dt, do, ds, need, di)
            return dt.download().reshape(B), do.download().reshape(B, n), ds.download().reshape(B), di.download().reshape(B, 4)
        finally:
            for b in (dm, dt, do, ds, di):
                b.free()
