"""TourSearch: a good order through up to 1024 stops, and the route that follows it -- a pick list, an inspection round, the task
list an Assignment hands one robot -- where Tour's exact optimum stops at 16.  The fields come from the stops chunk by chunk
(pf_dist_field_batch, or pf_cost_field under a cost map), each chunk is gathered into its row block of the stop-to-stop matrix in HBM
(pf_assign_matrix), and the order is searched on the device by pf_tour_improve: best-improvement 2-opt from the nearest-neighbour
order, then rounds of double-bridge perturbations of the incumbent, all starts of a round improved in one call over the one shared
matrix.  The rule reads the matrix's upper triangle only and is identical run to run for a given seed; `route_cost` holds any other
order against it.  `legs` / `path` trace the route through the parent maps of the same fields."""
import collections

import numpy as np

from ._planner import BIG, MOVES_MAX, STARTS_MAX, _int_in  # noqa: F401  (they are imported from here)
from ._planner import Planner, as_matrices, improve_call, move_limit, no_bad_entry, one_if_shared, restarts, start_rows
from .engine import Engine
from .tour import _mode, join_legs, route_cost

STOPS_MAX = 1024                                                     # PF_TOUR_SEARCH_MAX

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
    return improve_call(e, Improved, orders, (((B, 2), np.float64), (B, np.int32), ((B, 4), np.int64)),
                        lambda do, dv, ds, di: e.tour_improve(mode, n, B, shared, dm, cap, do, dv, ds, di))


def search(e, mode, n, dm, w, starts, rounds, seed, cap):
    """The search over the matrix dm holds (w: its mirrored copy on the host) -> dict(order, total, feasible, start_total, history,
    moves, kernel_ms).  Round 0 improves the nearest-neighbour order; each later round improves `starts` double-bridge
    perturbations of the incumbent in one call and keeps the strictly smallest total at the smallest start index (restarts)."""
    got, ms = _improve(e, mode, n, dm, True, [nearest_neighbour(w, mode)], cap)
    if int(got.status[0]) == 1:
        return dict(order=got.order[0], total=float("inf"), feasible=False, start_total=float("inf"), history=[float("inf")], moves=0, kernel_ms=ms)
    first, hi = float(got.value[0, 1]), last_movable(n, mode)

    def perturb(rng, order):
        cuts = [np.sort(rng.choice(np.arange(1, hi + 2), 3, replace=False)) for _ in range(starts)]
        return [double_bridge(order, *c) for c in cuts]
    got, at, history, moves, t = restarts(got, rounds if hi >= 3 else 0, seed, perturb, lambda rows: _improve(e, mode, n, dm, True, rows, cap),
                                          lambda g, x: float(g.value[x, 0]))
    return dict(order=got.order[at], total=history[-1], feasible=True, start_total=first, history=history, moves=moves, kernel_ms=ms + t)


class TourSearch(Planner):
    """stops: (r, c) pairs, at most 1024, stops[0] the start.  end: "open" (the tour ends anywhere), "return" (back to the start) or
    "last" (it ends at stops[-1]).  cost: None (path lengths, pf_dist_field_batch) or an [R, C] cost map as CostField's
    (pf_cost_field).  starts, rounds, seed: `rounds` rounds of `starts` perturbed restarts drawn from np.random.default_rng(seed).
    max_moves: the moves one start may take (None: 16 per stop).

    order: int32 stop indices in visiting order (it begins with 0, does not repeat 0 for "return"); total: its left-to-right sum
    under `matrix`; feasible: False where some stop cannot be reached from another (order is then all -1, total inf: the rule needs
    finite weights).  start_total: the nearest-neighbour order's total; history: the incumbent's total after round 0, 1, ...;
    moves: the 2-opt moves of all starts; matrix: float64 [n, n], the upper triangle of the gathered matrix on both sides (downloaded
    when the search is computed, not on first use: the nearest-neighbour start is found on the host from it)."""
    _closed, _built = "the tour search is closed", "a tour search"

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
        self._set_cost_and_moves(cost, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        self._set_search(starts, rounds, seed, max_moves, self.n)
        e = self._open(engine, Engine, self.ids)                             # every argument is checked: the device
        self.mbuf = e.buf((self.n, self.n), np.float64)
        self._compute()

    def _compute(self):
        e, n = self.engine, self.n
        ms = self._gather(lambda k, r0: e.assign_matrix(k, self.ids, self.buf, self.mbuf, r0, n, False))
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
        tour is infeasible (Planner._trace: the legs are grouped by the chunk of fields their first stop lies in)."""
        self._check_open()
        if not self.feasible:
            return []
        seq = [int(v) for v in self.order] + ([0] if self.mode == 1 and self.n > 1 else [])
        return self._trace([(a, int(self.ids[b])) for a, b in zip(seq[:-1], seq[1:])], "legs")

    def path(self):
        """The legs joined into one CellPath (a shared stop cell is not repeated); empty where the tour is infeasible."""
        return join_legs(self.legs(), self.cols)

    @classmethod
    def solve_matrices(cls, engine, mats, orders=None, end="open", shared=False, max_moves=None):
        """For callers with their own matrices and starts: mats float64 [B, n, n] -- or, with `shared`, one [n, n] for all starts --
        of which the upper triangles are read (entries in [0, 2^1000] or +inf, node 0 the start); orders int [B, n], the start
        rows (None: the nearest-neighbour order of each matrix); one `end` for all -> Improved(order int32 [B, n], value float64
        [B, 2] = (total after, total before), status int32 [B]: 0 a local optimum, 1 not searched (a +inf entry), 2 stopped by
        max_moves (None: 16 n), info int64 [B, 4] = (moves, sweeps, 0, 0))."""
        who = cls.__name__
        mode = _mode(who, end)
        m = as_matrices(who, "mats", mats, "n", "n")
        n = int(m.shape[1])
        _count_check(who, n, mode)
        one_if_shared(who, shared, m, "[n, n] matrix")
        cap = move_limit(who, max_moves, n)
        up = np.triu(np.ones((n, n), bool), 1)
        with np.errstate(invalid="ignore"):                           # (NaN fails the comparisons)
            no_bad_entry(who, "mats", m, ~(((m >= 0.0) & ((m <= BIG) | (m == np.inf))) | ~up[None]), "neither +inf nor a number in [0, 2^1000]")
        if orders is None:
            o = np.array([nearest_neighbour(mirrored(a), mode) for a in m], np.int64).reshape(len(m), n)
        else:
            o = start_rows(who, "orders", orders, m, shared, "n", n)
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
