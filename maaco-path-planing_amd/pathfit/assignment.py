"""Assignment: which robot takes which task -- the exact best one-to-one matching of robots and tasks under path length (or a cost
map's weighted length).  The fields come from the robots in one pf_dist_field_batch call (or one pf_cost_field call with
single-source sets) per chunk of rows that fits 256 MiB, each chunk is gathered at the task cells into the robot-to-task matrix in HBM
(pf_assign_matrix), and the matching is pf_assign_solve's: the smallest total ("sum"), the smallest largest leg ("max", the makespan)
or the smallest total among the matchings with the best makespan ("max_sum"), by a rule that is identical run to run and that a
greedy pairing can be held against (`assignment_cost`).  `paths` traces the matched routes through the parent maps of the same
fields; `pairs` feeds SpaceTime.plan_fleet."""
import collections

import numpy as np

from ._planner import BIG, Planner, as_matrices, chunk_rows, no_bad_entry  # noqa: F401  (chunk_rows and BIG are imported from here)
from .engine import Engine

OBJECTIVES = {"sum": 0, "max": 1, "max_sum": 2}
SIDE_MAX = 1024                                                      # PF_ASSIGN_MAX: the solver's columns

Solved = collections.namedtuple("Solved", "task_of robot_of value status dual info")


def _mode(who, objective):
    if not isinstance(objective, str) or objective not in OBJECTIVES:
        raise ValueError(f"{who}: objective must be 'sum', 'max' or 'max_sum', got {objective!r}")
    return OBJECTIVES[objective]


def both_sides(col, n_cols):
    """The solver's columns per row -> (col as int32, the row of each column or -1)."""
    col = np.asarray(col, np.int32).reshape(-1)
    back = np.full(int(n_cols), -1, np.int32)
    hit = np.flatnonzero(col >= 0)
    back[col[hit]] = hit
    return col.copy(), back


def pairing_cost(matrix, task_of, by_task):
    """(left-to-right float64 sum, max) of matrix[i, task_of[i]] over the matched robots, in robot order -- in task order when
    `by_task`, the order the solver's rows have when robots outnumber tasks; (0.0, -inf) for an empty pairing."""
    a = np.asarray(matrix, np.float64)
    at = [(i, int(j)) for i, j in enumerate(task_of) if j >= 0]
    if by_task:
        at.sort(key=lambda ij: ij[1])
    xs = [float(a[i, j]) for i, j in at]
    if not xs:
        return 0.0, float("-inf")
    s = xs[0]
    for x in xs[1:]:
        s = s + x
    return s, max(xs)


class Assignment(Planner):
    """robots, tasks: (r, c) pairs, at most 1024 of each.  objective: "sum", "max" or "max_sum".  cost: None (path lengths,
    pf_dist_field_batch) or an [R, C] cost map as CostField's (pf_cost_field).

    task_of: int32, the task of each robot, -1 for a robot without one; robot_of: int32, the robot of each task or -1.  total,
    makespan: the left-to-right sum and the largest of the matched legs (inf where infeasible).  feasible: False where the smaller
    side cannot be matched completely (task_of and robot_of are then all -1).  duals: float64, the solver's u then v (its rows are
    the robots, or the tasks when robots outnumber tasks); info: int64 [4] = (tree steps of the sum phase, of the max phase, the
    first solver row that could not be placed or -1, 0).  matrix: float64 [robots, tasks], downloaded on first use."""
    _closed, _built = "the assignment is closed", "an assignment"

    def __init__(self, grid, robots, tasks, objective="sum", cost=None, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        who = type(self).__name__
        self._set_grid(grid)
        self.mode = _mode(who, objective)
        self.objective = objective
        self.robot_ids = self._cell_ids("robots", robots)
        self.task_ids = self._cell_ids("tasks", tasks)
        self.nr, self.nt = len(self.robot_ids), len(self.task_ids)
        for what, k in (("robots", self.nr), ("tasks", self.nt)):
            if k < 1:
                raise ValueError(f"{who}: {what} is empty")
            if k > SIDE_MAX:
                raise ValueError(f"{who}: {k} {what}; at most {SIDE_MAX} are matched")
        self.robots = [(int(v) // self.cols, int(v) % self.cols) for v in self.robot_ids]
        self.tasks = [(int(v) // self.cols, int(v) % self.cols) for v in self.task_ids]
        self._set_cost_and_moves(cost, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        self.transposed = self.nr > self.nt                           # the solver's rows are the tasks
        self.n, self.m = (self.nt, self.nr) if self.transposed else (self.nr, self.nt)
        e = self._open(engine, Engine, self.robot_ids)                             # every argument is checked: the device
        self.mbuf = e.buf((self.n, self.m), np.float64)
        self._compute()

    def _compute(self):
        e = self.engine
        ms = self._gather(lambda k, r0: e.assign_matrix(k, self.task_ids, self.buf, self.mbuf, r0, self.m, self.transposed))
        n, m = self.n, self.m
        dc, dv, ds, dd, di = e.buf(n, np.int32), e.buf(2, np.float64), e.buf(1, np.int32), e.buf(n + m, np.float64), e.buf(4, np.int64)
        try:
            e.assign_solve(self.mode, n, m, 1, self.mbuf, dc, dv, ds, dd, di)
            self.solve_kernel_ms = e.last_kernel_ms()
            col, back = both_sides(dc.download(), m)
            value = dv.download()
            self.feasible = int(ds.download()[0]) == 0
            self.duals = dd.download().astype(np.float64)
            self.info = di.download().astype(np.int64)
        finally:
            for b in (dc, dv, ds, dd, di):
                b.free()
        self.task_of, self.robot_of = (back, col) if self.transposed else (col, back)
        self.total, self.makespan = float(value[0]), float(value[1])
        self.kernel_ms = ms + self.solve_kernel_ms
        self._matrix = None

    @property
    def matrix(self):
        """float64 [robots, tasks], downloaded on first use: matrix[i, j] = the field from robot i at task j."""
        if self._matrix is None:
            self._check_open()
            a = self.mbuf.download().reshape(self.n, self.m)
            self._matrix = np.ascontiguousarray(a.T) if self.transposed else a
        return self._matrix

    def assignment_cost(self, task_of):
        """(left-to-right sum, max) of any pairing -- task_of[i] the task of robot i or -1, no task twice -- under `matrix`, summed
        in the solver's row order (robots; tasks when robots outnumber tasks), so that assignment_cost(self.task_of) is (total,
        makespan) to the word: what a greedy pairing is compared with.  Host side."""
        who = type(self).__name__
        try:
            seq = [-1 if (isinstance(v, (int, np.integer)) and v == -1) else self._index("task_of[%d]" % i, v, self.nt) for i, v in enumerate(task_of)]
        except TypeError:
            raise ValueError(f"{who}: task_of must be a sequence of task indices, got {task_of!r}") from None
        if len(seq) != self.nr:
            raise ValueError(f"{who}: task_of has {len(seq)} entries for {self.nr} robots")
        taken = [v for v in seq if v >= 0]
        if len(set(taken)) != len(taken):
            raise ValueError(f"{who}: task_of gives a task to two robots")
        return pairing_cost(self.matrix, seq, self.transposed)

    def pairs(self):
        """(starts, goals): the matched robots' cells and their tasks' cells as (r, c) lists in robot order, the form
        SpaceTime.plan_fleet takes."""
        on = [i for i in range(self.nr) if self.task_of[i] >= 0]
        return [self.robots[i] for i in on], [self.tasks[int(self.task_of[i])] for i in on]

    def paths(self):
        """One CellPath per matched robot in robot order, from the robot to its task; [] where nothing is matched (Planner._trace)."""
        self._check_open()
        return self._trace([(i, int(self.task_ids[self.task_of[i]])) for i in range(self.nr) if self.task_of[i] >= 0], "routes")

    @classmethod
    def solve_matrices(cls, matrices, objective="sum", engine=None):
        """For callers with their own matrices: float64 [B, n, m] (or one [n, m]), +inf = no way, every other entry finite within
        2^1000 -> Solved(task_of int32 [B, n], robot_of int32 [B, m], value float64 [B, 2] = (sum, max), status int32 [B] with
        1 = infeasible, dual float64 [B, n + m] = the solver's u then v, info int64 [B, 4]).  With n > m the matrices are
        transposed on the host: the solver's rows are then the columns given.  engine: any Engine (None: one of the call's own)."""
        who = cls.__name__
        mode = _mode(who, objective)
        a = as_matrices(who, "matrices", matrices, "n", "m")
        B, rows, cols = (int(v) for v in a.shape)
        if max(rows, cols) > SIDE_MAX:
            raise ValueError(f"{who}: matrices of {rows} x {cols}; at most {SIDE_MAX} rows and columns are matched")
        with np.errstate(invalid="ignore"):
            no_bad_entry(who, "matrices", a, ~((a == np.inf) | (np.abs(a) <= BIG)), "neither +inf nor finite within 2^1000")   # (NaN fails both)
        flip = rows > cols
        if flip:
            a = np.ascontiguousarray(a.transpose(0, 2, 1))
        n, m = (cols, rows) if flip else (rows, cols)
        own = engine is None
        e = Engine(np.zeros((1, 1), np.uint8)) if own else engine
        bufs = []
        try:
            bufs.append(e.put(a.reshape(-1), np.float64))
            for shape, dt in (((B, n), np.int32), ((B, 2), np.float64), (B, np.int32), ((B, n + m), np.float64), ((B, 4), np.int64)):
                bufs.append(e.buf(shape, dt))
            dm, dc, dv, ds, dd, di = bufs
            e.assign_solve(mode, n, m, B, dm, dc, dv, ds, dd, di)
            col = dc.download().reshape(B, n)
            sides = [both_sides(c, m) for c in col]
            fwd, back = np.array([s[0] for s in sides], np.int32), np.array([s[1] for s in sides], np.int32)
            return Solved(back if flip else fwd, fwd if flip else back, dv.download().reshape(B, 2), ds.download().reshape(B),
                          dd.download().reshape(B, n + m), di.download().reshape(B, 4))
        finally:
            for b in bufs:
                b.free()
            if own:
                e.close()
