"""K independent GA populations in one batched generation (pf_decode_batch_multi, pf_ga_*_batch).

A population is one GASolver run with its own seed, start cell and target cell; the populations of a batch share the grid,
`population_size` (N), `num_waypoints_per_chromosome` (W), `num_generations`, the rates and the score parameters.  One
generation of all of them is one selection launch (a wavefront per population), one breed launch, ONE decode launch over the
K * N children -- every child carries its own start and target, so the longest-first queue and the tail policy see the whole
batch and one population's tail is filled with the others' chains --, one assembly launch, one segmented sort and one gather
of the K best rows.  Population k computes bit for bit what `GASolver(grid_k, ..., seed=seeds[k]).solve()` computes, grid_k
being the grid with its START / TARGET markers moved to (starts[k], targets[k]).

Initialisation (ga_solver.py:95-133) runs in rounds: each round collects the next attempts of every population that is still
short of N feasible individuals and decodes them all in one multi-endpoint launch.

Degenerate populations: when none of a population's 20 * N random attempts decodes, the solo class leaves its device loop (one
direct-path individual, or no individual at all -> `([], inf, 0, 0.0, 0.0, inf)`).  GABatch does not re-implement that branch:
such a population is handed, whole, to an internal solo GASolver on the same engine during `begin()`, and its result is
reported in its place; the other populations run batched.

The batch owns its buffers and the library entries are stateless (scratch is the engine's, stream ordered), so a solo
GASolver, MPA, MAACO or another batch on the same Engine is not disturbed, and `Engine.update_grid` has nothing to
invalidate: a batch that is stepped after it simply decodes on the new map.  A batch is single-GPU (no `comm`).
"""
import numpy as np

from ._batch import cell_ids, check_endpoints, check_grid_and_seeds
from ._lib import PathfitError
from .engine import Engine, score_params
from .env import mark
from .paths import CellPath, cells_of
from .solvers import (INF, GASolver, ga_attempt_round, ga_pad_and_sort, ga_random_chromosomes_native, ga_result_tuple,
                      ga_row_individual, ga_take_feasible)


class GaPopulation:
    """Population k of a GABatch, with GASolver's read surface (ga_solver.py:30-35, :162-218)."""

    def __init__(self, batch, k):
        self._b, self.k = batch, k
        self.start_node, self.target_node = batch.starts[k], batch.targets[k]
        self.seed = batch.seeds[k]
        self.convergence_curve = []
        self.best_solution_overall = {"fitness": INF, "path": []}
        self.attempts = 0                   # initial attempts made (ga_solver.py:100-114)
        self._solo = None                   # a degenerate population: the solo GASolver that ran it (GABatch docstring)
        self._result = None

    @property
    def population(self):
        """The reference's list of dicts in the population's current (sorted) order; materialised on demand."""
        return self._solo.population if self._solo is not None else self._b._population_of(self.k)

    def result(self):
        """What GASolver.solve() returns."""
        return self._result if self._solo is not None else ga_result_tuple(self.best_solution_overall)


class GABatch:
    def __init__(self, grid, num_generations, population_size, num_waypoints_per_chromosome, mutation_rate, crossover_rate,
                 seeds=(), starts=None, targets=None, tournament_size=3, turn_penalty_factor=0.1, safety_penalty_factor=0.05,
                 min_safe_distance=1.5, allow_diagonal_moves=True, restrict_diagonal_near_obstacle_policy=True,
                 diagonal_obstacle_penalty_value=1000.0, engine=None, device=0, verbose=False):
        # every argument is checked before the device is touched
        self.grid, self.seeds = check_grid_and_seeds("GABatch", grid, seeds, "population", "population_size", population_size)
        if int(num_waypoints_per_chromosome) < 1:
            raise ValueError("GABatch: num_waypoints_per_chromosome must be >= 1 (a GA without waypoints is one A* call: AStarSolver)")
        if int(num_generations) < 0:
            raise ValueError("GABatch: num_generations must be >= 0")
        if not 1 <= int(tournament_size) <= 64:
            raise ValueError("GABatch: tournament_size must be in [1, 64]")
        self.rows, self.cols = self.grid.shape
        K = len(self.seeds)
        try:
            self.starts, self.targets = check_endpoints("GABatch", "GA", self.grid, starts, targets, K)
        except ValueError as ex:                                       # (a missing marker is reported in the solo class's words)
            raise ValueError(str(ex) if str(ex).startswith("GABatch:") else f"GABatch: {ex}") from None
        self.K = K
        self.num_generations, self.population_size = int(num_generations), int(population_size)
        self.num_waypoints = int(num_waypoints_per_chromosome)
        self.mutation_rate, self.crossover_rate, self.tournament_size = mutation_rate, crossover_rate, int(tournament_size)
        self.allow_diagonal_moves = allow_diagonal_moves
        self.restrict_diagonal_near_obstacle_policy = restrict_diagonal_near_obstacle_policy
        self._weights = dict(turn_penalty_factor=turn_penalty_factor, safety_penalty_factor=safety_penalty_factor,
                             min_safe_distance=min_safe_distance, diagonal_obstacle_penalty_value=diagonal_obstacle_penalty_value)
        self.verbose = verbose
        self.engine = engine if engine is not None else Engine(self.grid, device)
        self._s, self._t = cell_ids(self.engine, "GABatch", self.grid, self.starts, self.targets)
        self._sp = score_params(0, restrict_diagonal_near_obstacle_policy, turn_penalty_factor, safety_penalty_factor,
                                min_safe_distance, diagonal_obstacle_penalty_value)
        self.path_cap = min(self.rows * self.cols, 16 * (self.rows + self.cols) + 64)      # _WaypointSolver._path_cap
        self._pops = [GaPopulation(self, k) for k in range(K)]
        self.live = []                      # the populations that run batched, in batch order (begin() fills it)
        self._d = None                      # the device state (begin())
        self._closed = False
        self.init_launches = 0              # multi-endpoint launches begin() made

    # ------------------------------------------------------------------
    def population(self, k):
        return self._pops[k]

    def _check_open(self):
        if self._closed or not getattr(self.engine, "h", None):
            raise PathfitError("GABatch: the batch is closed")

    def close(self):
        d, self._d = self._d, None
        self._closed = True
        if d:
            for v in d.values():
                for b in (v if isinstance(v, list) else [v]):
                    if hasattr(b, "free"):
                        b.free()

    # ------------------------------------------------------------------ initialisation
    def _decode(self, wp, s_cells, t_cells):
        """_WaypointSolver._evaluate with per-agent endpoints: retry once with the full R * C capacity, then raise."""
        e = self.engine
        kw = dict(wp_cells=wp, sp=self._sp, allow_diag=self.allow_diagonal_moves, restrict_corner=self.restrict_diagonal_near_obstacle_policy)
        paths, st, stats = e.decode_multi_host(s_cells, t_cells, path_cap=self.path_cap, **kw)
        self.init_launches += 1
        if (st == 3).any():
            paths, st, stats = e.decode_multi_host(s_cells, t_cells, path_cap=self.rows * self.cols, **kw)
            self.init_launches += 1
            if (st == 3).any():
                raise RuntimeError("pathfit: open-list scratch overflow on %d agents" % int((st == 3).sum()))
        return [CellPath(p, self.cols) for p in paths], stats, np.array([len(p) > 0 for p in paths])

    def _solo_solver(self, k):
        return GASolver(mark(self.grid, self.starts[k], self.targets[k]), self.num_generations, self.population_size,
                        self.num_waypoints, self.mutation_rate, self.crossover_rate, tournament_size=self.tournament_size,
                        allow_diagonal_moves=self.allow_diagonal_moves,
                        restrict_diagonal_near_obstacle_policy=self.restrict_diagonal_near_obstacle_policy, engine=self.engine,
                        seed=self.seeds[k], verbose=self.verbose, **self._weights)

    def begin(self):
        """GASolver._initialize_population (ga_solver.py:95-133) and :167-171 for every population, then the move into HBM."""
        self._check_open()
        if self._d is not None:
            raise PathfitError("GABatch: begin() has already run")
        K, N, W, occ = self.K, self.population_size, self.num_waypoints, self.grid == 1
        pops = [[] for _ in range(K)]
        while True:
            short = [k for k in range(K) if len(pops[k]) < N and self._pops[k].attempts < 20 * N]
            if not short:
                break
            # one round: the next attempts of every population that is still short, decoded in ONE launch
            sizes = [ga_attempt_round(N, len(pops[k]), self._pops[k].attempts) for k in short]
            wp = np.concatenate([ga_random_chromosomes_native(self.seeds[k], self._pops[k].attempts, n, W, occ) for k, n in zip(short, sizes)])
            cps, stats, feas = self._decode(wp, np.repeat(self._s[short], sizes), np.repeat(self._t[short], sizes))
            o = 0
            for k, n in zip(short, sizes):
                ga_take_feasible(pops[k], N, wp[o:o + n], cps[o:o + n], stats[o:o + n], feas[o:o + n], self.cols)
                self._pops[k].attempts += n
                o += n
        self.live = [k for k in range(K) if pops[k]]
        for k in range(K):
            p = self._pops[k]
            if not pops[k]:                                          # degenerate: the solo class runs it whole
                p._solo = self._solo_solver(k)
                p._result = p._solo.solve()
                p.best_solution_overall, p.convergence_curve = p._solo.best_solution_overall, p._solo.convergence_curve
                continue
            ga_pad_and_sort(pops[k], N, self.seeds[k])               # :130-132
            p.best_solution_overall = pops[k][0].copy()              # :170
            p.convergence_curve.append(p.best_solution_overall["fitness"])
        self._to_device(pops)

    def _to_device(self, pops):
        """The live populations into HBM, back to back in batch order: row j N + i = individual i of live population j."""
        e, N, W, cap, live = self.engine, self.population_size, self.num_waypoints, self.path_cap, self.live
        Kb = len(live)
        d = {"cur": 0}
        self._d = d
        if not Kb:
            return
        ind = [x for k in live for x in pops[k]]
        chrom = np.stack([x["_cells"] for x in ind]).astype(np.int32)
        stats = np.array([[x["length"], x["turns"], x["safety_penalty"], x["diag_penalty"], x["fitness"]] for x in ind], np.float64)
        cells, lens = np.zeros((Kb * N, cap), np.int32), np.zeros(Kb * N, np.int32)
        for i, x in enumerate(ind):
            cc = cells_of(x["path"], self.cols)
            if len(cc) > cap:
                raise RuntimeError("pathfit: path capacity overflow in GA initialisation")
            cells[i, :len(cc)] = cc; lens[i] = len(cc)
        KN = Kb * N
        d["seeds"] = e.put(np.array([self.seeds[k] for k in live], np.uint64))
        d["start"], d["target"] = e.put(np.repeat(self._s[live], N)), e.put(np.repeat(self._t[live], N))      # per CHILD
        d["chrom"] = [e.put(chrom), e.buf((KN, W), np.int32)]
        d["stats"] = [e.put(stats), e.buf((KN, 5), np.float64)]
        d["cells"] = [e.put(cells), e.buf((KN, cap), np.int32)]
        d["len"] = [e.put(lens), e.buf(KN, np.int32)]
        d["fit"] = e.put(stats[:, 4].copy())
        d["iota"] = e.put(np.tile(np.arange(N, dtype=np.int32), Kb))
        d["order"], d["psid"] = e.put(np.tile(np.arange(N, dtype=np.int32), Kb)), e.buf(KN, np.int32)
        d["kid_chrom"], d["kid_cells"] = e.buf((KN, W), np.int32), e.buf((KN, cap), np.int32)
        d["kid_len"], d["kid_st"], d["kid_stats"] = e.buf(KN, np.int32), e.buf(KN, np.int32), e.buf((KN, 5), np.float64)
        self._rows = np.empty((Kb, 6), np.float64)

    # ------------------------------------------------------------------ device state, for readers and tests
    def device_state(self, k):
        """(order, chromosomes [N][W], stats [N][5], cells [N][cap], lengths [N]) of live population k: host copies."""
        self._check_open()
        d, N, W, cap, j = self._d, self.population_size, self.num_waypoints, self.path_cap, self.live.index(k)
        cur, r0 = d["cur"], j * N
        return (d["order"].read(r0, N), d["chrom"][cur].read(r0 * W, N * W).reshape(N, W), d["stats"][cur].read(r0 * 5, N * 5).reshape(N, 5),
                d["cells"][cur].read(r0 * cap, N * cap).reshape(N, cap), d["len"][cur].read(r0, N))

    def _population_of(self, k):
        order, chrom, stats, cells, lens = self.device_state(k)
        return [ga_row_individual(chrom[i].copy(), CellPath(cells[i, :lens[i]].copy(), self.cols), stats[i], self.cols) for i in order]

    # ------------------------------------------------------------------ one generation
    def step(self, gen):
        """ga_solver.py:178-213 for every live population (gen is 0-based, as the streams are keyed).  Per generation the host
        reads the decode's range flag (4 B), the counters and the K best rows (K x 48 B); a population's chromosome and path row
        are read only when its best improves."""
        self._check_open()
        if self._d is None:
            raise PathfitError("GABatch: begin() has not run")
        Kb = len(self.live)
        if not Kb:
            return
        e, d, N, W, cap = self.engine, self._d, self.population_size, self.num_waypoints, self.path_cap
        cur, KN = d["cur"], Kb * N
        e.ga_select_batch(d["seeds"], gen, Kb, N, self.tournament_size, d["fit"], d["order"], d["psid"])               # :181
        e.ga_breed_batch(d["seeds"], gen, Kb, N, W, self.crossover_rate, self.mutation_rate, d["chrom"][cur], d["psid"], d["kid_chrom"])   # :186-194
        e.decode_multi(KN, W, d["start"], d["target"], cap, d["kid_cells"], d["kid_len"], d["kid_st"], d["kid_chrom"], None, self._sp,
                       d["kid_stats"], self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle_policy)         # :198-200 the hot path
        if e.counters()["overflow_agents"]:
            raise RuntimeError("pathfit: scratch/path capacity overflow in GA decode")
        e.ga_assemble_batch(Kb, N, W, cap, d["kid_len"], d["kid_chrom"], d["kid_stats"], d["kid_cells"], d["psid"], d["chrom"][cur],
                            d["stats"][cur], d["cells"][cur], d["len"][cur], d["chrom"][1 - cur], d["stats"][1 - cur],
                            d["cells"][1 - cur], d["len"][1 - cur])                                                    # :201-205
        cur = d["cur"] = 1 - cur
        e.gather_col(KN, d["stats"][cur], 5, 4, d["fit"])
        d["order"].copy_from(0, d["iota"], 0, KN)
        e.sort_order_by_key_seg(Kb, N, d["fit"], 1, 0, d["order"])                                                     # :209 stable sort
        rows = e.best_rows_seg(Kb, N, d["stats"][cur], d["order"], self._rows)
        for j, k in enumerate(self.live):
            p, sid, s5 = self._pops[k], int(rows[j, 0]), rows[j, 1:].copy()
            if s5[4] < p.best_solution_overall["fitness"]:                                                             # :212-213
                r = j * N + sid
                ch = d["chrom"][cur].read(r * W, W)
                L = int(d["len"][cur].read(r, 1)[0])
                p.best_solution_overall = ga_row_individual(ch, CellPath(d["cells"][cur].read(r * cap, L), self.cols), s5, self.cols)
            p.convergence_curve.append(p.best_solution_overall["fitness"])
        if self.verbose and ((gen + 1) % 10 == 0 or gen == 0 or gen == self.num_generations - 1):
            best = min(self._pops[k].best_solution_overall["fitness"] for k in self.live)
            print(f"GABatch Gen {gen + 1}/{self.num_generations}: K={self.K}, BestFit={best:.2f}")

    def solve(self):
        """-> the K result tuples, each what GASolver.solve() returns."""
        self.begin()
        for gen in range(self.num_generations):
            self.step(gen)
        return [p.result() for p in self._pops]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
