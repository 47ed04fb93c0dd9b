"""What MAACOBatch, MPABatch, GABatch and PSOBatch share: the argument checks of their constructors (all of them run before the device
is touched; `who` is the class name every message starts with), the ownership of an object the library keeps on an Engine
(EngineOwned: MAACOBatch, MPABatch) and the host side of a batch of waypoint solvers (WaypointBatch: GABatch, PSOBatch)."""
import numpy as np

from ._lib import PathfitError
from .engine import score_params
from .env import OBSTACLE, START_NODE_VAL, TARGET_NODE_VAL, find_marker
from .solvers import decode_retry, ga_attempt_round, path_capacity


def check_grid_and_seeds(who, grid, seeds, unit, count_name, count):
    """-> (2-D int grid, K seeds in [0, 2^64)); `count` (ants / predators per `unit`) must be >= 1."""
    grid = np.array(grid, dtype=int)
    if grid.ndim != 2:
        raise ValueError(f"{who}: grid must be 2-D")
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError(f"{who}: seeds is empty (one seed per {unit})")
    if any(s < 0 or s >= 1 << 64 for s in seeds):
        raise ValueError(f"{who}: seeds must be in [0, 2^64)")
    if int(count) < 1:
        raise ValueError(f"{who}: {count_name} must be >= 1")
    return grid, seeds


def _cells(who, name, pts, K, grid):
    R, Cc = grid.shape
    out = []
    for k, p in enumerate(pts):
        try:
            r, c = (int(v) for v in p)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {name}[{k}] must be an (r, c) pair, got {p!r}") from None
        if not (0 <= r < R and 0 <= c < Cc):
            raise ValueError(f"{who}: {name}[{k}] = {(r, c)} is outside the {R}x{Cc} grid")
        if grid[r, c] == OBSTACLE:
            raise ValueError(f"{who}: {name}[{k}] = {(r, c)} is on an obstacle")
        out.append((r, c))
    if len(out) != K:
        raise ValueError(f"{who}: {len(out)} {name} for {K} seeds")
    return out


def check_endpoints(who, solver, grid, starts, targets, K):
    """-> (K starts, K targets) as (r, c) pairs; None = the grid's marker for every one (`solver` names it in find_marker's error)."""
    if starts is None:
        starts = [find_marker(grid, START_NODE_VAL, solver)] * K
    if targets is None:
        targets = [find_marker(grid, TARGET_NODE_VAL, solver)] * K
    return _cells(who, "starts", list(starts), K, grid), _cells(who, "targets", list(targets), K, grid)


def cell_ids(engine, who, grid, starts, targets):
    """-> the flat int32 ids of the start and of the target cells, once the engine is known to hold a grid of this shape."""
    if (engine.R, engine.C) != grid.shape:
        raise ValueError(f"{who}: the engine's grid has another shape")
    return tuple(np.array([r * grid.shape[1] + c for r, c in cells], np.int32) for cells in (starts, targets))


class EngineOwned:
    """An object the library owns on `self.engine`: `self._b` is its handle (None before creation and once closed), `_destroy`
    the library symbol that frees it."""
    _destroy = None

    def _ck(self, rc):
        if rc != 0:
            raise PathfitError(self.engine.L.pf_last_error(self.engine.h).decode())

    def _handle(self):
        if not self._b or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the batch is closed")
        return self._b

    def close(self):
        # (a closed Engine has freed its batches already)
        if getattr(self, "_b", None) and getattr(self.engine, "h", None):
            getattr(self.engine.L, self._destroy)(self._b)
        self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WaypointBatch:
    """K solo GA / PSO runs (`units`: populations, swarms) on one grid that own their buffers and share the engine's decode: the
    constructor's checks, the initialisation in rounds, the hand-off of a degenerate unit to the solo class, and the lifecycle.
    A subclass adds its own arguments, `_draw` / `_take` / `_solo_solver` / `_to_device` and its step."""
    _solver = None                          # the solo class's short name, as find_marker's errors say it ("GA", "PSO")
    _unit = None                            # what a seed stands for in the messages ("population", "swarm")
    _wp = None                              # decode_host's argument for what _draw returns first ("wp_cells", "wp_pos")
    _mirror = ()                            # attributes of a degenerate unit's solo solver that the unit shows as its own

    def _check_sizes(self, grid, seeds, count_name, count, wp_name, num_waypoints, iters_name, iterations):
        who = type(self).__name__
        self.grid, self.seeds = check_grid_and_seeds(who, grid, seeds, self._unit, count_name, count)
        if int(num_waypoints) < 1:
            raise ValueError(f"{who}: {wp_name} must be >= 1 (a {self._solver} without waypoints is one A* call: AStarSolver)")
        if int(iterations) < 0:
            raise ValueError(f"{who}: {iters_name} must be >= 0")
        self.rows, self.cols = self.grid.shape
        self.K, self._N, self.num_waypoints = len(self.seeds), int(count), int(num_waypoints)

    def _open(self, starts, targets, allow_diagonal_moves, restrict_diagonal_near_obstacle_policy, weights, engine, new_engine, unit_cls,
              verbose):
        """The endpoint checks, then -- every argument being checked -- the device: `engine`, or new_engine() for one of its own."""
        who = type(self).__name__
        try:
            self.starts, self.targets = check_endpoints(who, self._solver, self.grid, starts, targets, self.K)
        except ValueError as ex:                                       # (a missing marker is reported in the solo class's words)
            raise ValueError(str(ex) if str(ex).startswith(f"{who}:") else f"{who}: {ex}") from None
        self.allow_diagonal_moves = allow_diagonal_moves
        self.restrict_diagonal_near_obstacle_policy = restrict_diagonal_near_obstacle_policy
        self._weights = weights
        self.verbose = verbose
        self.engine = engine if engine is not None else new_engine()
        self._s, self._t = cell_ids(self.engine, who, self.grid, self.starts, self.targets)
        self._sp = score_params(0, restrict_diagonal_near_obstacle_policy, weights["turn_penalty_factor"], weights["safety_penalty_factor"],
                                weights["min_safe_distance"], weights["diagonal_obstacle_penalty_value"])
        self.path_cap = path_capacity(self.rows, self.cols, self.num_waypoints)
        self._units = [unit_cls(self, k) for k in range(self.K)]
        self.live = []                      # the units that run batched, in batch order (begin() fills it)
        self._d = None                      # the device state (begin())
        self._closed = False
        self.init_launches = 0              # multi-endpoint launches begin() made

    # ------------------------------------------------------------------ lifecycle
    def _check_open(self):
        if self._closed or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the batch is closed")

    def _check_begun(self):
        self._check_open()
        if self._d is None:
            raise PathfitError(f"{type(self).__name__}: begin() has not run")

    def close(self):
        d, self._d = getattr(self, "_d", None), None
        self._closed = True
        if d:
            for v in d.values():
                for b in (v if isinstance(v, list) else [v]):
                    if hasattr(b, "free"):
                        b.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ initialisation
    def _decode(self, wp, s_cells, t_cells):
        """_WaypointSolver._evaluate with per-agent endpoints."""
        cps, stats, feas, launches = decode_retry(self.engine, s_cells, t_cells, self.rows, self.cols, sp=self._sp,
                                                  allow_diag=self.allow_diagonal_moves,
                                                  restrict_corner=self.restrict_diagonal_near_obstacle_policy, **{self._wp: wp})
        self.init_launches += launches
        return cps, stats, feas

    def begin(self):
        """The solo class's initialisation for every unit, then the move into HBM (_to_device).  It runs in rounds: a round draws
        the next attempts of every unit that is still short of N feasible ones (_draw(unit, n) -> a tuple, the waypoints first)
        and decodes them all in ONE multi-endpoint launch; _take(unit, draw, paths, stats, feasible) keeps the feasible ones in
        `unit._init`.  A unit none of whose 20 N attempts decodes is degenerate: the solo class runs it whole."""
        self._check_open()
        if self._d is not None:
            raise PathfitError(f"{type(self).__name__}: begin() has already run")
        K, N, units = self.K, self._N, self._units
        have = [0] * K
        while True:
            short = [k for k in range(K) if have[k] < N and units[k].attempts < 20 * N]
            if not short:
                break
            sizes = [ga_attempt_round(N, have[k], units[k].attempts) for k in short]
            draws = [self._draw(units[k], n) for k, n in zip(short, sizes)]
            cps, stats, feas = self._decode(np.concatenate([d[0] for d in draws]), np.repeat(self._s[short], sizes), np.repeat(self._t[short], sizes))
            o = 0
            for k, n, draw in zip(short, sizes, draws):
                self._take(units[k], draw, cps[o:o + n], stats[o:o + n], feas[o:o + n])
                have[k] = min(N, have[k] + int(feas[o:o + n].sum()))
                units[k].attempts += n
                o += n
        self.live = [k for k in range(K) if have[k]]
        for p in (units[k] for k in range(K) if not have[k]):
            p._solo = self._solo_solver(p.k)
            p._result = p._solo.solve()
            for name in self._mirror:
                setattr(p, name, getattr(p._solo, name))
        self._to_device()
