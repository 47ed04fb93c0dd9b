"""FleetTours: which robot takes which tasks, and in which order -- k robots, n tasks with n >> k, each task done once by some robot,
where Assignment hands every robot one task and TourSearch orders the stops of one robot.  The fields come from the k + n cells
chunk by chunk (pf_dist_field_batch, or pf_cost_field under a cost map), each chunk is gathered into its row block of the
node-to-node matrix in HBM (pf_assign_matrix), and the routes are searched on the device by pf_fleet_improve: best-improvement 2-opt
inside a route and relocation of segments of one to three tasks within a route or to another robot's, from a greedy start, then
rounds of perturbed restarts of the incumbent, all starts of a round improved in one call over the one shared matrix.  Capacities
bound the tasks a robot may hold.  The rule reads the matrix's upper triangle only and is identical run to run for a given seed;
`route_cost` holds any other routes against it.  `legs` / `paths` trace the routes through the parent maps of the same fields.
objective="makespan" searches for the routes whose LONGEST is shortest instead (pf_fleet_balance: the same candidates, priced by the
largest length they leave): the greedy start is improved under the sum rule, then balanced, and the rounds balance the perturbed
restarts, keeping the strictly smallest (makespan, total)."""
import collections

import numpy as np

from ._field import Field
from ._lib import PathfitError
from .assignment import chunk_rows
from .cost_field import checked_cost
from .engine import Engine
from .paths import CellPath
from .tour import join_legs
from .tour_search import BIG, MOVES_MAX, STARTS_MAX, _int_in, mirrored

NODES_MAX = 1024                                                     # PF_FLEET_MAX
ENDS = {"open": 0, "return": 1}
OBJECTIVES = ("sum", "makespan")
PERTURB_MOVES = 3                                                    # the relocations drawn per perturbed start

Improved = collections.namedtuple("Improved", "route lengths value status info")


def _mode(who, end):
    if not isinstance(end, str) or end not in ENDS:
        raise ValueError(f"{who}: end must be 'open' or 'return', got {end!r}")
    return ENDS[end]


def _objective(who, objective):
    if not isinstance(objective, str) or objective not in OBJECTIVES:
        raise ValueError(f"{who}: objective must be 'sum' or 'makespan', got {objective!r}")
    return objective


def _count_check(who, k, n):
    if k < 1:
        raise ValueError(f"{who}: robots is empty")
    if n < 1:
        raise ValueError(f"{who}: tasks is empty")
    if k + n > NODES_MAX:
        raise ValueError(f"{who}: {k} robots and {n} tasks; at most {NODES_MAX} cells together are searched")


def _capacity(who, capacity, k, n):
    """None, one int for every robot or k ints -> None or int32 [k]; the capacities must hold the n tasks."""
    if capacity is None:
        return None
    if isinstance(capacity, (int, np.integer)) and not isinstance(capacity, bool):
        cap = [capacity] * k
    else:
        try:
            cap = list(capacity)
        except TypeError:
            cap = None
        if cap is None or len(cap) != k:
            raise ValueError(f"{who}: capacity must be None, an integer or a list of {k} integers (one per robot), got {capacity!r}")
    for r, c in enumerate(cap):
        if not isinstance(c, (int, np.integer)) or isinstance(c, bool) or not 0 <= int(c) < (1 << 30):
            raise ValueError(f"{who}: capacity[{r}] must be an integer in [0, 2^30), got {c!r}")
    if sum(int(c) for c in cap) < n:
        raise ValueError(f"{who}: the capacities hold {sum(int(c) for c in cap)} tasks, fewer than the {n} given")
    return np.array([int(c) for c in cap], np.int32)


def split(route, k):
    """A route row -> one list of task nodes per robot."""
    out, r = [[] for _ in range(k)], -1
    for v in route:
        if int(v) < k:
            r += 1
        else:
            out[r].append(int(v))
    return out


def row_of(lists):
    """One list of task nodes per robot -> the route row."""
    out = []
    for r, tasks in enumerate(lists):
        out.append(r)
        out.extend(int(v) for v in tasks)
    return out


def lengths(w, lists, mode):
    """Each robot's length under w: its legs summed left to right from its start on, the leg home last for mode 1 -> (len list,
    their left-to-right sum, the largest)."""
    lens = []
    for r, tasks in enumerate(lists):
        seq = [r] + [int(v) for v in tasks]
        t = 0.0 if len(seq) == 1 else float(w[seq[0], seq[1]])
        for a, b in zip(seq[1:-1], seq[2:]):
            t = t + float(w[a, b])
        if len(seq) > 1:
            t = t + (float(w[seq[-1], r]) if mode == 1 else 0.0)
        lens.append(t)
    total = lens[0]
    for x in lens[1:]:
        total = total + x
    return lens, total, max(lens)


def start_row(w, k, cap=None):
    """The start: the tasks in index order, each to the robot with room that has the smallest w(robot, task), the smallest index on a
    tie; then every route in nearest-neighbour order from its robot, the smallest task index on a tie."""
    N = len(w)
    held = np.zeros(k, np.int64)
    room = np.full(k, N, np.int64) if cap is None else np.asarray(cap, np.int64)
    lists = [[] for _ in range(k)]
    for t in range(k, N):
        d = np.where(held < room, w[:k, t], np.inf)
        free = np.flatnonzero(held < room)
        r = int(free[int(np.argmin(d[free]))])                        # (the first smallest: free is ascending)
        lists[r].append(t)
        held[r] += 1
    for r in range(k):
        left, at, out = np.array(lists[r], np.int64), r, []
        while len(left):
            x = int(np.argmin(w[at, left]))
            at = int(left[x])
            out.append(at)
            left = np.delete(left, x)
        lists[r] = out
    return row_of(lists)


def relocated(o, L, i, j):
    """The segment at positions i .. i + L - 1 taken out and put back, in the same direction, directly behind position j's node."""
    seg = o[i:i + L]
    if j < i:
        return o[:j + 1] + seg + o[j + 1:i] + o[i + L:]
    return o[:i] + o[i + L:j + 1] + seg + o[j + 1:]


def perturbed(route, k, cap, draws):
    """A perturbed start: per draw (x, i, j) the segment of x % 3 + 1 tasks at position i goes behind position j where the rule
    admits that relocation (the segment all tasks of one route, j outside i - 1 .. i + L - 1, room in j's route); else the draw is
    dropped."""
    o = [int(v) for v in route]
    N = len(o)
    for x, i, j in draws:
        L, i, j = int(x) % 3 + 1, int(i), int(j)
        if i < 1 or i + L > N or min(o[i:i + L]) < k or i - 1 <= j <= i + L - 1:
            continue
        rob = np.cumsum(np.array(o) < k) - 1
        if rob[j] != rob[i] and cap is not None and int(np.sum((rob == rob[j]) & (np.array(o) >= k))) + L > int(cap[rob[j]]):
            continue
        o = relocated(o, L, i, j)
    return o


def perturbations(rng, route, k, cap, starts):
    """`starts` perturbed starts of a row: one rng.integers(0, N, (starts, PERTURB_MOVES, 3)) draw."""
    draws = rng.integers(0, len(route), (starts, PERTURB_MOVES, 3))
    return [perturbed(route, k, cap, draws[s]) for s in range(starts)]


def _improve(e, mode, k, n, dm, shared, dcap, routes, limit, balance=False):
    """One pf_fleet_improve call (pf_fleet_balance with `balance`: four values and five infos a start) over the start rows `routes`
    [B, k + n] -> (Improved, kernel ms)."""
    N = k + n
    routes = np.ascontiguousarray(routes, np.int32).reshape(-1, N)
    B = len(routes)
    nv, ni = (4, 5) if balance else (3, 4)
    do = e.put(routes.reshape(-1), np.int32)
    dl, dv, ds, di = e.buf((B, k), np.float64), e.buf((B, nv), np.float64), e.buf(B, np.int32), e.buf((B, ni), np.int64)
    try:
        (e.fleet_balance if balance else e.fleet_improve)(mode, k, n, B, shared, dm, dcap, limit, do, dl, dv, ds, di)
        ms = e.last_kernel_ms()
        return Improved(do.download().reshape(B, N).astype(np.int32), dl.download().reshape(B, k), dv.download().reshape(B, nv), ds.download().reshape(B),
                        di.download().reshape(B, ni)), ms
    finally:
        for b in (do, dl, dv, ds, di):
            b.free()


def search(e, mode, k, n, dm, w, cap, dcap, starts, rounds, seed, limit):
    """The search over the matrix dm holds (w: its mirrored copy on the host) -> dict(route, lengths, total, makespan, feasible,
    start_total, history, moves, kernel_ms).  Round 0 improves the start row; each later round improves `starts` perturbations of the
    incumbent in one call and keeps the strictly smallest total at the smallest start index."""
    inf = float("inf")
    got, ms = _improve(e, mode, k, n, dm, True, dcap, [start_row(w, k, cap)], limit)
    if int(got.status[0]) == 1:
        return dict(route=got.route[0], lengths=[inf] * k, total=inf, makespan=inf, feasible=False, start_total=inf, history=[inf], moves=0, kernel_ms=ms)
    route, lens, best, span, first = got.route[0], got.lengths[0], float(got.value[0, 0]), float(got.value[0, 2]), float(got.value[0, 1])
    history, moves = [best], int(got.info[0, 0])
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        got, t = _improve(e, mode, k, n, dm, True, dcap, perturbations(rng, route, k, cap, starts), limit)
        ms += t
        moves += int(got.info[:, 0].sum())
        x = int(np.argmin(got.value[:, 0]))                           # (the first smallest)
        if got.value[x, 0] < best:
            best, span, route, lens = float(got.value[x, 0]), float(got.value[x, 2]), got.route[x], got.lengths[x]
        history.append(best)
    return dict(route=route, lengths=[float(x) for x in lens], total=best, makespan=span, feasible=True, start_total=first, history=history, moves=moves,
                kernel_ms=ms)


def search_makespan(e, mode, k, n, dm, w, cap, dcap, starts, rounds, seed, limit):
    """The min-max search over the matrix dm holds -> search's dict, and total_history.  Round 0 improves the
    start row under the sum rule (pf_fleet_improve), then balances the result (pf_fleet_balance); each later round balances
    `starts` perturbations of the incumbent in one call and keeps the strictly smallest (makespan, total) at the smallest start
    index.  history holds the incumbent's makespan per round, total_history its total."""
    inf = float("inf")
    got, ms = _improve(e, mode, k, n, dm, True, dcap, [start_row(w, k, cap)], limit)
    if int(got.status[0]) == 1:
        return dict(route=got.route[0], lengths=[inf] * k, total=inf, makespan=inf, feasible=False, start_total=inf, history=[inf], total_history=[inf], moves=0,
                    kernel_ms=ms)
    first, moves = float(got.value[0, 1]), int(got.info[0, 0])
    got, t = _improve(e, mode, k, n, dm, True, dcap, got.route, limit, balance=True)
    ms += t
    moves += int(got.info[0, 0])
    route, lens, best = got.route[0], got.lengths[0], (float(got.value[0, 0]), float(got.value[0, 1]))
    history, totals = [best[0]], [best[1]]
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        got, t = _improve(e, mode, k, n, dm, True, dcap, perturbations(rng, route, k, cap, starts), limit, balance=True)
        ms += t
        moves += int(got.info[:, 0].sum())
        x = min(range(len(got.value)), key=lambda b: (float(got.value[b, 0]), float(got.value[b, 1]), b))      # (the first smallest pair)
        if (float(got.value[x, 0]), float(got.value[x, 1])) < best:
            best, route, lens = (float(got.value[x, 0]), float(got.value[x, 1])), got.route[x], got.lengths[x]
        history.append(best[0])
        totals.append(best[1])
    return dict(route=route, lengths=[float(x) for x in lens], total=best[1], makespan=best[0], feasible=True, start_total=first, history=history,
                total_history=totals, moves=moves, kernel_ms=ms)


class FleetTours(Field):
    """robots, tasks: (r, c) pairs, at most 1024 together; robot r starts on robots[r].  end: "open" (a route ends at its last task)
    or "return" (every robot comes back to its own start).  capacity: None, the most tasks any robot may hold, or one number per
    robot.  cost: None (path lengths, pf_dist_field_batch) or an [R, C] cost map as CostField's (pf_cost_field).  starts, rounds,
    seed: `rounds` rounds of `starts` perturbed restarts drawn from np.random.default_rng(seed).  max_moves: the moves one start may
    take (None: 16 per cell).  objective: "sum" (the smallest total) or "makespan" (the smallest largest length, then the smallest
    total: pf_fleet_balance).

    routes: per robot the list of task indices in visiting order (a route may be empty); lengths: per robot its route's length;
    total: their left-to-right sum under `matrix`; makespan: the largest (reported, not optimised, under objective="sum"; what
    is searched under "makespan"); feasible: False where some cell cannot be reached from another (routes are then empty, total inf:
    the rule needs finite weights).  start_total, start_makespan: the greedy start's; history: the incumbent's objective (the total,
    or the makespan) after round 0, 1, ...; total_history: its total; moves: the moves of all starts; matrix: float64 [N, N],
    N = k + n, robots first, the upper triangle of the gathered matrix on both sides."""
    _bufs = ("buf", "pbuf", "mbuf", "cost_device", "cap_device")
    CHUNK_BYTES = 256 << 20

    def __init__(self, grid, robots, tasks, end="open", capacity=None, cost=None, starts=8, rounds=3, seed=0, max_moves=None,
                 allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None, objective="sum"):
        who = type(self).__name__
        self._set_grid(grid)
        self.mode = _mode(who, end)
        self.objective = _objective(who, objective)
        self.end = end
        rid, tid = self._cell_ids("robots", robots), self._cell_ids("tasks", tasks)
        self.k, self.n = len(rid), len(tid)
        _count_check(who, self.k, self.n)
        self.ids = np.concatenate([rid, tid]).astype(np.int32)
        self.N = self.k + self.n
        self.robots = [(int(v) // self.cols, int(v) % self.cols) for v in rid]
        self.tasks = [(int(v) // self.cols, int(v) % self.cols) for v in tid]
        self.capacity = _capacity(who, capacity, self.k, self.n)
        self.cost = None if cost is None else checked_cost(who, self.grid, cost)
        self.starts = _int_in(who, "starts", starts, 1, STARTS_MAX)
        self.rounds = _int_in(who, "rounds", rounds, 0, 1 << 20)
        self.seed = _int_in(who, "seed", seed, 0, (1 << 63) - 1)
        limit = _int_in(who, "max_moves", max_moves, 0, MOVES_MAX, none_ok=True)
        self.max_moves = 16 * self.N if limit is None else limit
        self.allow_diagonal_moves = bool(allow_diagonal_moves)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self.chunk = chunk_rows(self.N, self.rows * self.cols, self.CHUNK_BYTES)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        e = self.engine
        self.cost_device = None if self.cost is None else e.put(self.cost.reshape(-1), np.float64)
        self.cap_device = None if self.capacity is None else e.put(self.capacity, np.int32)
        self.buf = e.buf((self.chunk, self.rows, self.cols), np.float64)
        self.mbuf = e.buf((self.N, self.N), np.float64)
        self.pbuf = None
        self._compute()

    def _check_open(self):
        if self.buf is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the fleet tours are closed")

    def _fields(self, r0):
        """The fields of the cells r0 .. r0 + c - 1 into buf (c = the chunk's rows) -> c."""
        e, c = self.engine, min(self.chunk, self.N - r0)
        ids = self.ids[r0:r0 + c]
        if self.cost_device is None:
            e.dist_field_batch(ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        else:
            e.cost_field(self.cost_device, np.arange(c + 1, dtype=np.int32), ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        self._held = r0
        return c

    def _compute(self):
        e, N = self.engine, self.N
        ms = 0.0
        for r0 in range(0, N, self.chunk):
            c = self._fields(r0)
            ms += e.last_kernel_ms()
            e.assign_matrix(c, self.ids, self.buf, self.mbuf, r0, N, False)
            ms += e.last_kernel_ms()
        self.matrix = mirrored(self.mbuf.download().reshape(N, N))
        find = search_makespan if self.objective == "makespan" else search
        got = find(e, self.mode, self.k, self.n, self.mbuf, self.matrix, self.capacity, self.cap_device, self.starts, self.rounds, self.seed, self.max_moves)
        self.feasible = got["feasible"]
        self.route = np.asarray(got["route"], np.int32)
        self.routes = [[v - self.k for v in tasks] for tasks in split(self.route, self.k)] if self.feasible else [[] for _ in range(self.k)]
        self.lengths, self.total, self.makespan, self.start_total = list(got["lengths"]), got["total"], got["makespan"], got["start_total"]
        self.history, self.moves = got["history"], got["moves"]
        self.total_history = got.get("total_history", self.history)
        start = split(start_row(self.matrix, self.k, self.capacity), self.k)
        self.start_makespan = lengths(self.matrix, start, self.mode)[2] if self.feasible else float("inf")
        self.solve_kernel_ms = got["kernel_ms"]
        self.kernel_ms = ms + self.solve_kernel_ms

    def _nodes(self, routes):
        """Routes of task indices -> lists of task nodes, every index checked and no task twice."""
        who = type(self).__name__
        try:
            lists = [list(r) for r in routes]
        except TypeError:
            lists = None
        if lists is None or len(lists) != self.k:
            raise ValueError(f"{who}: routes must be {self.k} sequences of task indices (one per robot), got {routes!r}")
        seen = set()
        for r, tasks in enumerate(lists):
            for x, v in enumerate(tasks):
                t = self._index(f"routes[{r}][{x}]", v, self.n)
                if t in seen:
                    raise ValueError(f"{who}: routes[{r}][{x}] = {t} is visited twice")
                seen.add(t)
        return [[int(v) + self.k for v in tasks] for tasks in lists]

    def route_cost(self, routes):
        """The total of any routes (k lists of task indices, no task twice; tasks may be left out) under `matrix`: each robot's legs
        summed left to right, then the robots' lengths: what another heuristic's routes are compared with;
        route_cost(self.routes) == total.  Host side."""
        return lengths(self.matrix, self._nodes(routes), self.mode)[1]

    def route_makespan(self, routes):
        """The largest length of any routes (as route_cost's) under `matrix`; route_makespan(self.routes) == makespan.  Host side."""
        return lengths(self.matrix, self._nodes(routes), self.mode)[2]

    def legs(self):
        """Per robot the list of CellPaths of its route's legs in visiting order (for end="return" the last one leads back to its
        start; [] for an empty route); [] where the problem is infeasible.  Each leg is DistanceField.paths' route from its first
        cell to its second, cell for cell.  The legs are grouped by the chunk of fields their first cell lies in: a parent-map call per
        chunk and one trace call with a field index per query.  A chunk of fields that was released for a later one is computed again."""
        self._check_open()
        if not self.feasible:
            return []
        pairs, owner = [], []
        for r, tasks in enumerate(split(self.route, self.k)):
            seq = [r] + tasks + ([r] if self.mode == 1 and tasks else [])
            pairs += list(zip(seq[:-1], seq[1:]))
            owner += [r] * (len(seq) - 1)
        out = {}
        e, full = self.engine, self.rows * self.cols
        ad, rs = self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle
        for r0 in sorted(range(0, self.N, self.chunk), key=lambda r: r != self._held):      # the chunk held first: it is not computed again
            mine = [x for x in range(len(pairs)) if r0 <= pairs[x][0] < r0 + self.chunk]
            if not mine:
                continue
            c = min(self.chunk, self.N - r0)
            if self._held != r0:
                self._fields(r0)
                if self.pbuf is not None:
                    self.pbuf.free()
                    self.pbuf = None
            if self.pbuf is None:
                pbuf = e.buf((self.chunk, self.rows, self.cols), np.uint8)
                try:
                    if self.cost_device is None:
                        e.dist_field_parents(c, self.buf, pbuf, ad, rs)
                    else:
                        e.cost_field_parents(self.cost_device, c, self.buf, pbuf, ad, rs)
                except Exception:
                    pbuf.free()
                    raise
                self.pbuf = pbuf
            q = len(mine)
            dk = e.put(np.array([pairs[x][0] - r0 for x in mine], np.int32))
            dt = e.put(self.ids[np.array([pairs[x][1] for x in mine])].astype(np.int32))
            dl, dst = e.buf(q, np.int32), e.buf(q, np.int32)
            dcl, cap = None, e.default_path_cap()
            try:
                while True:
                    dcl = e.buf((q, cap), np.int32)
                    e.dist_field_paths(c, self.pbuf, dt, q, cap, dcl, dl, dst, dk, self.buf, False, None)
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
        legs = [[] for _ in range(self.k)]
        for x, r in enumerate(owner):
            legs[r].append(out[x])
        return legs

    def paths(self):
        """Per robot its legs joined into one CellPath (a shared cell is not repeated; a robot without tasks stays on its start
        cell); [] where the problem is infeasible."""
        return [join_legs(legs, self.cols) if legs else CellPath(np.array([self.ids[r]], np.int32), self.cols) for r, legs in enumerate(self.legs())]

    def refresh(self, cost=None):
        """Search the routes again on the map the engine holds now (after engine.update_grid) and, when given, under a new cost map
        (for a search built with one)."""
        who = type(self).__name__
        self._check_open()
        if cost is not None and self.cost is None:
            raise ValueError(f"{who}: refresh(cost) needs fleet tours built with a cost map")
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
    def solve_matrices(cls, engine, mats, k, routes=None, end="open", capacity=None, shared=False, max_moves=None):
        """For callers with their own matrices and starts: mats float64 [B, N, N] -- or, with `shared`, one [N, N] for all starts --
        of which the upper triangles are read (nodes 0 .. k - 1 the robots, the rest the tasks; readable entries in [0, 2^1000] or
        +inf); routes int [B, N], the start rows (None: the greedy start of each matrix); one `end` and `capacity` for all ->
        Improved(route int32 [B, N], lengths float64 [B, k], value float64 [B, 3] = (total after, total before, makespan after),
        status int32 [B]: 0 no improving move is left, 1 not searched (a +inf entry), 2 stopped by max_moves (None: 16 N), info
        int64 [B, 4] = (moves, sweeps, 2-opt moves, relocate moves))."""
        return cls._matrices(engine, False, mats, k, routes, end, capacity, shared, max_moves)

    @classmethod
    def balance_matrices(cls, engine, mats, k, routes=None, end="open", capacity=None, shared=False, max_moves=None):
        """solve_matrices under the min-max rule (pf_fleet_balance) -> Improved(route int32 [B, N], lengths float64 [B, k], value
        float64 [B, 4] = (makespan after, total after, makespan before, total before), status int32 [B] as solve_matrices', info
        int64 [B, 5] = (moves, sweeps, 2-opt moves, relocate moves, moves that lowered the span))."""
        return cls._matrices(engine, True, mats, k, routes, end, capacity, shared, max_moves)

    @classmethod
    def _matrices(cls, engine, balance, mats, k, routes, end, capacity, shared, max_moves):
        """solve_matrices and balance_matrices: the checks, the uploads and the one call."""
        who = cls.__name__
        mode = _mode(who, end)
        try:
            m = np.ascontiguousarray(mats, np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: mats must be a [B, N, N] array of numbers") from None
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[1] != m.shape[2] or m.shape[0] < 1:
            raise ValueError(f"{who}: mats has shape {m.shape}, not [B, N, N] with B >= 1")
        N = int(m.shape[1])
        k = _int_in(who, "k", k, 1, NODES_MAX)
        _count_check(who, k, N - k)
        n = N - k
        if shared and m.shape[0] != 1:
            raise ValueError(f"{who}: shared=True takes one [N, N] matrix, got {m.shape[0]}")
        cap = _capacity(who, capacity, k, n)
        limit = _int_in(who, "max_moves", max_moves, 0, MOVES_MAX, none_ok=True)
        limit = 16 * N if limit is None else limit
        read = np.triu(np.ones((N, N), bool), 1)
        read[:, :k] = False
        with np.errstate(invalid="ignore"):
            bad = np.argwhere(~(((m >= 0.0) & ((m <= BIG) | (m == np.inf))) | ~read[None]))      # (NaN fails the comparisons)
        if len(bad):
            b, i, j = (int(v) for v in bad[0])
            raise ValueError(f"{who}: mats[{b}, {i}, {j}] = {float(m[b, i, j])!r} is neither +inf nor a number in [0, 2^1000]")
        if routes is None:
            o = np.array([start_row(mirrored(a), k, cap) for a in m], np.int64).reshape(len(m), N)
        else:
            try:
                o = np.array(routes)
                o = o[None] if o.ndim == 1 else o
                ok = o.ndim == 2 and o.shape[1] == N and o.shape[0] >= 1 and o.dtype.kind in "iu"
            except (TypeError, ValueError):
                ok = False
            if not ok or (not shared and o.shape[0] != m.shape[0]):
                raise ValueError(f"{who}: routes must be an integer array [B, N] with a row per matrix (any B >= 1 with shared=True)")
            for b, row in enumerate(o):
                seen = set()
                for p, v in enumerate(row):
                    v = int(v)
                    if not 0 <= v < N or v in seen or (p == 0 and v != 0) or (1 <= v < k and v - 1 not in seen):
                        raise ValueError(f"{who}: routes[{b}, {p}] = {v}: a start is a permutation of the nodes with node 0 first and the robots in "
                                         "increasing order")
                    seen.add(v)
                if cap is not None:
                    for r, tasks in enumerate(split(row, k)):
                        if len(tasks) > int(cap[r]):
                            raise ValueError(f"{who}: routes[{b}] gives robot {r} {len(tasks)} tasks, more than its capacity {int(cap[r])}")
        dm = engine.put(m.reshape(-1), np.float64)
        dcap = None if cap is None else engine.put(cap, np.int32)
        try:
            return _improve(engine, mode, k, n, dm, bool(shared), dcap, o, limit, balance)[0]
        finally:
            dm.free()
            if dcap is not None:
                dcap.free()
