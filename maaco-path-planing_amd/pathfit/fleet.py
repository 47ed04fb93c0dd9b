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

from ._planner import BIG, Planner, _int_in, as_matrices, improve_call, move_limit, no_bad_entry, one_if_shared, restarts, start_rows
from .engine import Engine
from .paths import CellPath
from .tour import join_legs
from .tour_search import mirrored

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
    routes = np.ascontiguousarray(routes, np.int32).reshape(-1, k + n)
    B = len(routes)
    nv, ni = (4, 5) if balance else (3, 4)
    call = e.fleet_balance if balance else e.fleet_improve
    return improve_call(e, Improved, routes, (((B, k), np.float64), ((B, nv), np.float64), (B, np.int32), ((B, ni), np.int64)),
                        lambda do, dl, dv, ds, di: call(mode, k, n, B, shared, dm, dcap, limit, do, dl, dv, ds, di))


def _infeasible(got, k, ms, **more):
    inf = float("inf")
    return dict(route=got.route[0], lengths=[inf] * k, total=inf, makespan=inf, feasible=False, start_total=inf, history=[inf], moves=0, kernel_ms=ms, **more)


def search(e, mode, k, n, dm, w, cap, dcap, starts, rounds, seed, limit):
    """The search over the matrix dm holds (w: its mirrored copy on the host) -> dict(route, lengths, total, makespan, feasible,
    start_total, history, moves, kernel_ms).  Round 0 improves the start row; each later round improves `starts` perturbations of the
    incumbent in one call and keeps the strictly smallest total at the smallest start index (restarts)."""
    got, ms = _improve(e, mode, k, n, dm, True, dcap, [start_row(w, k, cap)], limit)
    if int(got.status[0]) == 1:
        return _infeasible(got, k, ms)
    first = float(got.value[0, 1])
    got, x, history, moves, t = restarts(got, rounds, seed, lambda rng, route: perturbations(rng, route, k, cap, starts),
                                         lambda rows: _improve(e, mode, k, n, dm, True, dcap, rows, limit), lambda g, b: float(g.value[b, 0]))
    return dict(route=got.route[x], lengths=[float(v) for v in got.lengths[x]], total=history[-1], makespan=float(got.value[x, 2]), feasible=True,
                start_total=first, history=history, moves=moves, kernel_ms=ms + t)


def search_makespan(e, mode, k, n, dm, w, cap, dcap, starts, rounds, seed, limit):
    """The min-max search over the matrix dm holds -> search's dict, and total_history.  Round 0 improves the
    start row under the sum rule (pf_fleet_improve), then balances the result (pf_fleet_balance); each later round balances
    `starts` perturbations of the incumbent in one call and keeps the strictly smallest (makespan, total) at the smallest start
    index (restarts).  history holds the incumbent's makespan per round, total_history its total."""
    got, ms = _improve(e, mode, k, n, dm, True, dcap, [start_row(w, k, cap)], limit)
    if int(got.status[0]) == 1:
        return _infeasible(got, k, ms, total_history=[float("inf")])
    first, summed = float(got.value[0, 1]), int(got.info[0, 0])
    got, t0 = _improve(e, mode, k, n, dm, True, dcap, got.route, limit, balance=True)
    got, x, keys, moves, t = restarts(got, rounds, seed, lambda rng, route: perturbations(rng, route, k, cap, starts),
                                      lambda rows: _improve(e, mode, k, n, dm, True, dcap, rows, limit, balance=True),
                                      lambda g, b: (float(g.value[b, 0]), float(g.value[b, 1])))
    return dict(route=got.route[x], lengths=[float(v) for v in got.lengths[x]], total=keys[-1][1], makespan=keys[-1][0], feasible=True, start_total=first,
                history=[key[0] for key in keys], total_history=[key[1] for key in keys], moves=summed + moves, kernel_ms=ms + t0 + t)


class FleetTours(Planner):
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
    _bufs = Planner._bufs + ("cap_device",)
    _closed, _built = "the fleet tours are closed", "fleet tours"

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
        self._set_cost_and_moves(cost, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        self._set_search(starts, rounds, seed, max_moves, self.N)
        e = self._open(engine, Engine, self.ids)                             # every argument is checked: the device
        self.cap_device = None if self.capacity is None else e.put(self.capacity, np.int32)
        self.mbuf = e.buf((self.N, self.N), np.float64)
        self._compute()

    def _compute(self):
        e, N = self.engine, self.N
        ms = self._gather(lambda c, r0: e.assign_matrix(c, self.ids, self.buf, self.mbuf, r0, N, False))
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
        start; [] for an empty route); [] where the problem is infeasible (Planner._trace: the legs are grouped by the chunk of fields
        their first cell lies in)."""
        self._check_open()
        if not self.feasible:
            return []
        queries, owner = [], []
        for r, tasks in enumerate(split(self.route, self.k)):
            seq = [r] + tasks + ([r] if self.mode == 1 and tasks else [])
            queries += [(a, int(self.ids[b])) for a, b in zip(seq[:-1], seq[1:])]
            owner += [r] * (len(seq) - 1)
        legs = [[] for _ in range(self.k)]
        for r, leg in zip(owner, self._trace(queries, "legs")):
            legs[r].append(leg)
        return legs

    def paths(self):
        """Per robot its legs joined into one CellPath (a shared cell is not repeated; a robot without tasks stays on its start
        cell); [] where the problem is infeasible."""
        return [join_legs(legs, self.cols) if legs else CellPath(np.array([self.ids[r]], np.int32), self.cols) for r, legs in enumerate(self.legs())]

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
        m = as_matrices(who, "mats", mats, "N", "N")
        N = int(m.shape[1])
        k = _int_in(who, "k", k, 1, NODES_MAX)
        _count_check(who, k, N - k)
        n = N - k
        one_if_shared(who, shared, m, "[N, N] matrix")
        cap = _capacity(who, capacity, k, n)
        limit = move_limit(who, max_moves, N)
        read = np.triu(np.ones((N, N), bool), 1)
        read[:, :k] = False
        with np.errstate(invalid="ignore"):                           # (NaN fails the comparisons)
            no_bad_entry(who, "mats", m, ~(((m >= 0.0) & ((m <= BIG) | (m == np.inf))) | ~read[None]), "neither +inf nor a number in [0, 2^1000]")
        if routes is None:
            o = np.array([start_row(mirrored(a), k, cap) for a in m], np.int64).reshape(len(m), N)
        else:
            o = start_rows(who, "routes", routes, m, shared, "N", N)
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
