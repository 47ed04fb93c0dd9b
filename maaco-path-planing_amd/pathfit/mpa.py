"""MPA with the reference's constructor / solve_path_planning() surface
(MPA.py:10-18, :320-448).  The population lives in HBM as strided paths and an
iteration never leaves it: the stable sort by fitness (:333,:412) is a device
radix sort of the list order, the elite (:334) is copied into a device buffer,
the phase sweep (:339-377: target-cell proposal, two A* stitches, scoring), the
memory step (:381-384) and the FADs sweep (:387-410) are device batches.  The
host keeps the scalars: CF (:336) and the 4-level best-so-far tie-break
(:415-437) on the 5 stats of the iteration's best predator; its path is read
only when the best improves.  Device-to-host traffic per iteration: the doubt
count of the proposals (4 B), the work counters (72 B), the best row (44 B).

Per-predator streams: (seed, DOM_MPA, iter, i) for the phase sweep and
(seed, DOM_MPA_FADS, iter, i) for FADs, with i the predator's index in the
fitness-sorted population of that iteration (the reference's loop index).
"""
import math

import numpy as np

from ._lib import MpaParams
from .engine import Engine, score_params
from .env import START_NODE_VAL, TARGET_NODE_VAL, find_marker
from .paths import CellPath

INF = float("inf")


def levy_sigma(beta):
    """MPA.py:251-253 (Mantegna)."""
    num = math.gamma(1 + beta) * math.sin(math.pi * beta / 2)
    den = math.gamma((1 + beta) / 2) * beta * (2 ** ((beta - 1) / 2))
    return (num / den) ** (1 / beta) if den > 1e-9 else 1.0


def cf_and_phase(it, num_iterations):
    """CF (MPA.py:336) and the phase (1, 2, 3: thirds of the run) of iteration `it` (1-based)."""
    ratio = it / num_iterations
    CF = 0.0 if ratio >= 1.0 else ((1.0 - ratio) ** (2.0 * ratio) if ratio > 0 else 1.0)
    phase = 1 if it <= num_iterations / 3 else (2 if it <= 2 * num_iterations / 3 else 3)
    return CF, phase


STALE = -1      # in an acceptance history: the level waiting for the iteration that follows was found stale


def lookahead_depth(history, cap, left, always=False):
    """How many consecutive iterations the next sweep covers (pf_mpa_iter_ahead): a pure function of the acceptance history
    (predators changed by each iteration so far, oldest first, with STALE before an iteration whose waiting level had to be
    thrown away), the option "mpa_lookahead" (`cap`, 0 = off) and the iterations left in the run, this one included.
    0: off -- the plain sweep.  1: this iteration alone.  An iteration that accepted nothing left the population, the list
    order and the elite as they were, so the iterations after it can be swept with it, up to `cap` and never past the run's
    end; after a stale level the run goes back to single sweeps until the next quiet iteration.  `always` (test hook
    "mpa_lookahead_always") treats every iteration as quiet."""
    if cap <= 0:
        return 0
    if left <= 1:
        return 1
    if history and history[-1] == STALE:
        return 1
    quiet = always or (len(history) > 0 and history[-1] == 0)
    return min(int(cap), int(left)) if quiet else 1


class BestSoFar:
    """The reference's best-so-far state of one population (MPA.py:30-36) and its rules.  `s` is the stats[5] of the best
    predator of an iteration (length, turns, safety penalty, diagonal penalty, fitness); `fetch()` brings its path as a
    list of (r, c) and is called only when that predator becomes the best so far."""

    def _init_best(self):
        self.best_path_overall = []
        self.best_path_length_overall = INF
        self.best_path_turns_overall = INF
        self.best_safety_penalty_overall = INF
        self.best_diag_penalty_overall = INF
        self.best_fitness_overall = INF
        self.convergence_curve_data = []

    def _update_best(self, s, fetch):
        self.best_fitness_overall = float(s[4])
        self.best_path_overall = fetch()
        self.best_path_length_overall = float(s[0])
        self.best_path_turns_overall = int(s[1])
        self.best_safety_penalty_overall = float(s[2])
        self.best_diag_penalty_overall = float(s[3])

    def _take_first(self, s, fetch):
        """MPA.py:322-330: the initial population's best and the first point of the curve."""
        self._update_best(s, fetch)
        self.convergence_curve_data.append(self.best_fitness_overall if self.best_fitness_overall != INF else None)

    def _take(self, s, fetch):
        """MPA.py:415-440: best-so-far with the 4-level tie-break, then the iteration's point of the curve."""
        if s[4] < self.best_fitness_overall:
            self._update_best(s, fetch)
        elif abs(s[4] - self.best_fitness_overall) < 1e-9:
            bl, bt, bs, bd = (self.best_path_length_overall, self.best_path_turns_overall,
                              self.best_safety_penalty_overall, self.best_diag_penalty_overall)
            if s[0] < bl:
                self._update_best(s, fetch)
            elif abs(s[0] - bl) < 1e-9 and s[1] < bt:
                self._update_best(s, fetch)
            elif abs(s[0] - bl) < 1e-9 and abs(s[1] - bt) < 1e-9 and s[2] < bs:
                self._update_best(s, fetch)
            elif abs(s[0] - bl) < 1e-9 and abs(s[1] - bt) < 1e-9 and abs(s[2] - bs) < 1e-9 and s[3] < bd:
                self._update_best(s, fetch)
        c = self.convergence_curve_data
        c.append(self.best_fitness_overall if self.best_fitness_overall != INF else
                 (c[-1] if c and c[-1] is not None else None))

    def result(self):
        return (self.best_path_overall, self.best_path_length_overall, self.best_path_turns_overall,
                self.best_safety_penalty_overall, self.best_diag_penalty_overall, self.best_fitness_overall)


class MPA(BestSoFar):
    def __init__(self, grid, num_predators, num_iterations, FADs_rate=0.2, P_const=0.5, levy_beta=1.5,
                 turn_penalty_factor=0.1, safety_penalty_factor=0.05, min_safe_distance=1.5, allow_diagonal_moves=True,
                 restrict_diagonal_near_obstacle=True, diagonal_obstacle_penalty=1000.0, engine=None, device=0, seed=0,
                 verbose=False, agent0=0, n_local=None, fused=True):
        self.grid = np.array(grid, dtype=int)
        self.rows, self.cols = self.grid.shape
        self.num_predators, self.num_iterations = num_predators, num_iterations
        self.FADs_rate, self.P_const, self.levy_beta = FADs_rate, P_const, levy_beta
        self.turn_penalty_factor_mpa = turn_penalty_factor
        self.safety_penalty_factor_mpa = safety_penalty_factor
        self.min_safe_distance_mpa = min_safe_distance
        self.allow_diagonal_moves = allow_diagonal_moves
        self.restrict_diagonal_near_obstacle = restrict_diagonal_near_obstacle
        self.diagonal_obstacle_penalty_val = diagonal_obstacle_penalty
        self.start_node = find_marker(self.grid, START_NODE_VAL, "MPA")
        self.target_node = find_marker(self.grid, TARGET_NODE_VAL, "MPA")
        self.obstacle_nodes = np.argwhere(self.grid == 1)
        self._init_best()
        self.seed, self.verbose = int(seed), verbose
        self.n_local = int(n_local) if n_local else int(num_predators)   # predators stored on this GPU (sharding)
        self.fused = bool(fused)   # one work queue for the phase sweep + FADs candidates (pf_mpa_iter_batch)
        self.engine = engine if engine is not None else Engine(self.grid, device)
        self._s = self.start_node[0] * self.cols + self.start_node[1]
        self._t = self.target_node[0] * self.cols + self.target_node[1]
        self._sp = score_params(1, restrict_diagonal_near_obstacle, turn_penalty_factor, safety_penalty_factor,
                                min_safe_distance, diagonal_obstacle_penalty)
        self._mp = MpaParams(float(P_const), float(levy_beta), levy_sigma(levy_beta), float(FADs_rate),
                             int(num_predators), self._s, self._t, int(bool(allow_diagonal_moves)),
                             int(bool(restrict_diagonal_near_obstacle)))
        self.engine.mpa_setup(self._mp, self._sp)
        if hasattr(self.engine, "mpa_set_owner"):
            self.engine.mpa_set_owner(self)
        self.path_cap = min(self.rows * self.cols, 8 * (self.rows + self.cols) + 64)
        self._init_population()

    # ------------------------------------------------------------------
    def _init_population(self):
        """MPA._initialize_population_with_safety (MPA.py:231-245): N identical A*(start, target) paths."""
        e, N = self.engine, self.n_local
        while True:
            paths, st = e.astar_host(1, [self._s], [self._t], None, path_cap=self.path_cap,
                                     allow_diag=self.allow_diagonal_moves, restrict_corner=self.restrict_diagonal_near_obstacle)
            if st[0] == 3 and self.path_cap < self.rows * self.cols:
                self.path_cap = min(self.rows * self.cols, self.path_cap * 4)
                continue
            if st[0] == 3:                                               # not the row: the open list's scratch ran out
                raise RuntimeError("pathfit: scratch/path capacity overflow in the initial search (path_cap=%d)" % self.path_cap)
            break
        p = paths[0]
        if len(p) == 0:                                                  # :235-236
            p = np.array([self._s, self._t] if self.grid[self.target_node] != 1 else [self._s], np.int32)
        stats = e.score_host([p], self._sp)[0]
        cap = self.path_cap
        cells = np.zeros((N, cap), np.int32)
        cells[:, :len(p)] = p
        self.d_cells = e.put(cells)
        self.d_len = e.put(np.full(N, len(p), np.int32))
        self.d_stats = e.put(np.tile(stats, (N, 1)))
        self.d_cand_cells, self.d_cand_len = e.buf((N, cap), np.int32), e.buf(N, np.int32)
        self.d_cand_stats, self.d_status = e.buf((N, 5), np.float64), e.buf(N, np.int32)
        self.d_c2_cells, self.d_c2_len, self.d_c2_stats = e.buf((N, cap), np.int32), e.buf(N, np.int32), e.buf((N, 5), np.float64)
        self.d_order = e.put(np.arange(N, dtype=np.int32))               # the list: sorted position -> storage slot
        self._sorted = False                                             # (see _sort)
        self.d_gidx = e.put(np.arange(N, dtype=np.int32))                # single GPU: every predator is local
        self._own_rows = (self.d_cand_cells, self.d_cand_len, self.d_cand_stats, self.d_c2_cells, self.d_c2_len, self.d_c2_stats,
                          self.d_status)
        self.drop_lookahead()
        self._el_cells, self._el_len, self._el_stats = e.mpa_elite_bufs()

    @property
    def order(self):
        """sorted position -> storage slot (host copy on demand)."""
        return self.d_order.download()

    @property
    def _stats_host(self):
        return self.d_stats.download()

    @property
    def population(self):
        """The reference's list of dicts, in the current (sorted) order; materialised on demand."""
        cells, lens, stats = self.d_cells.download(), self.d_len.download(), self.d_stats.download()
        out = []
        for slot in self.order:
            s = stats[slot]
            out.append({"path": CellPath(cells[slot, :lens[slot]].copy(), self.cols), "length": float(s[0]),
                        "turns": int(s[1]), "safety_penalty": float(s[2]), "diag_penalty": float(s[3]),
                        "fitness": float(s[4])})
        return out

    def _path_of_slot(self, slot):
        L = int(self.d_len.read(slot, 1)[0])
        return self.d_cells.read(slot * self.path_cap, L)

    def _fetch(self, slot):
        return lambda: CellPath(self._path_of_slot(slot), self.cols).tolist()

    def _sort(self):
        """list.sort(key=fitness) is stable (MPA.py:321,:333,:412): device sort of the list order.  The sort at the start of an
        iteration (:333) re-sorts the list the end of the previous one (:412) left sorted on the same keys -- nothing -- and is
        skipped while no sweep has touched the population since."""
        if getattr(self, "_sorted", False):
            return
        self.engine.sort_order_by_key(self.n_local, self.d_stats, 5, 4, self.d_order)
        self._sorted = True

    def _best_row(self):
        """(storage slot, stats[5]) of population[0] -- two small reads."""
        slot = int(self.d_order.read(0, 1)[0])
        return slot, self.d_stats.read(slot * 5, 5)

    def step(self, it):
        """One iteration of MPA.py:332-440 (it is 1-based)."""
        e, N, cap = self.engine, self.n_local, self.path_cap
        self._claim()
        self._sort()                                                     # :333
        e.mpa_pick_elite(cap, self.d_cells, self.d_len, self.d_stats, self.d_order)   # :334 elite = population[0].copy()
        CF, phase = cf_and_phase(it, self.num_iterations)                # :336
        el_c, el_s = self._el_cells.ptr, self._el_stats.ptr
        self._sorted = False                                             # the sweep rewrites the population
        if self.fused:
            self._sweep(it, N, self.d_gidx, self.d_order)                # :339-410 in one queue
            self._check_overflow()
        else:
            elite_len = int(self._el_len.read(0, 1)[0])
            e.mpa_phase(phase, CF, it, self.seed, N, cap, self.d_cells, self.d_len, self.d_stats, self.d_gidx, self.d_order,
                        el_c, elite_len, el_s, self.d_cand_cells, self.d_cand_len, self.d_cand_stats, self.d_status)
            self._check_overflow()
            e.mpa_memory(N, cap, self.d_order, self.d_cand_cells, self.d_cand_len, self.d_cand_stats,
                         self.d_cells, self.d_len, self.d_stats)            # :381-384
            e.mpa_fads(CF, it, self.seed, N, cap, self.d_gidx, self.d_order, self.d_cells, self.d_len, self.d_stats, self.d_status)   # :387-410
            self._check_overflow()
        self._sort()                                                     # :412
        slot, s = self._best_row()
        self._take(s, self._fetch(slot))                                 # :415-440
        return s

    def drop_lookahead(self):
        """Forget the iterations swept ahead and the acceptance history: the population has been (re)built or changed by
        something other than step()."""
        self.accept_history = []         # predators changed by every iteration so far (STALE marks a discarded level)
        self._ahead_left = 0             # levels of the last merged sweep still waiting
        if hasattr(self.engine, "mpa_ahead_drop"):
            self.engine.mpa_ahead_drop()

    def _claim(self):
        """The handle holds one solo MPA set-up (Engine.mpa_setup): if another MPA on this Engine has stepped since, or the map
        was set up anew, set this one up again.  That drops the levels swept ahead -- the next take finds nothing waiting, the
        history gets STALE -- and the other instance has copied the candidate rows it was reading out of the level buffers."""
        e = self.engine
        if hasattr(e, "mpa_owner") and e.mpa_owner() is not self:
            e.mpa_setup(self._mp, self._sp)
            e.mpa_set_owner(self)

    def _own_views(self):
        """Candidate rows that are views into the handle's level buffers (after a served or leading step) are copied into this
        instance's own rows, and d_cand_* / d_c2_* / d_status point there again: the level buffers are about to be rewritten,
        or freed, by another instance's sweep."""
        cur = (self.d_cand_cells, self.d_cand_len, self.d_cand_stats, self.d_c2_cells, self.d_c2_len, self.d_c2_stats, self.d_status)
        if cur[0] is self._own_rows[0]:
            return
        for own, view in zip(self._own_rows, cur):
            own.copy_from(0, view, 0, int(np.prod(view.shape)))
        (self.d_cand_cells, self.d_cand_len, self.d_cand_stats, self.d_c2_cells, self.d_c2_len, self.d_c2_stats,
         self.d_status) = self._own_rows

    def _sweep(self, it, n, d_gidx, d_slot, world=1):
        """The fused device work of iteration `it` for the n predators stored here (MPA.step and ShardedMPA.step).  With the
        look-ahead on (one rank only: another rank's acceptance changes the global list) an iteration that follows a quiet
        one is served from the sweep that already covered it, or sweeps the iterations after it along with its own."""
        e, cap, K = self.engine, self.path_cap, self.num_iterations
        self._claim()
        own = self._own_rows
        st = e.mpa_ahead_stats() if world == 1 else {"cap": 0, "always": 0}
        el_c, el_s = self._el_cells.ptr, self._el_stats.ptr
        CF, phase = cf_and_phase(it, K)
        acc, rows = -1, own                              # (rows: where this iteration's candidate rows end up)
        if st["cap"] > 0 and self._ahead_left > 0:
            acc = e.mpa_ahead_take(it, d_slot, self.d_cells, self.d_len, self.d_stats)
            self._ahead_left = self._ahead_left - 1 if acc >= 0 else 0
            if acc < 0:
                self.accept_history.append(STALE)
            else:
                rows = None                              # a level's
        if acc < 0:
            depth = lookahead_depth(self.accept_history, st["cap"], K - it + 1, bool(st["always"]))
            if depth == 0:                               # off: exactly the plain sweep
                self._ahead_left = 0
                e.mpa_iter(phase, CF, it, self.seed, n, cap, self.d_cells, self.d_len, self.d_stats, d_gidx, d_slot, el_c, -1, el_s, *own)
            else:
                levels = [(cf_and_phase(it + d, K)[1], cf_and_phase(it + d, K)[0], it + d) for d in range(depth)]
                acc = e.mpa_iter_ahead(levels, self.seed, n, cap, self.d_cells, self.d_len, self.d_stats, d_gidx, d_slot, el_c, -1,
                                       el_s, *own)
                self._ahead_left = depth - 1
                if depth > 1:
                    rows = None
        if acc >= 0:
            self.accept_history.append(acc)
        (self.d_cand_cells, self.d_cand_len, self.d_cand_stats, self.d_c2_cells, self.d_c2_len, self.d_c2_stats,
         self.d_status) = rows or e.mpa_ahead_level_bufs(n, cap)

    def _check_overflow(self):
        n = self.engine.counters()["overflow_agents"]      # counted on the device: no status column leaves HBM
        if n:
            raise RuntimeError("pathfit: scratch/path capacity overflow on %d predators (path_cap=%d)" % (n, self.path_cap))

    def solve_path_planning(self):
        self._sort()                                                     # :321
        slot, s0 = self._best_row()
        self._take_first(s0, self._fetch(slot))                          # :322-330
        for it in range(1, self.num_iterations + 1):
            s = self.step(it)
            if self.verbose and (it % 10 == 0 or it == 1 or it == self.num_iterations):
                print(f"MPA Iter {it}/{self.num_iterations}: IterBest Fit={s[4]:.2f}; OverallBest Fit={self.best_fitness_overall:.2f}")
        return self.result()
