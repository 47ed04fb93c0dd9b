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

from ._batch import WaypointBatch
from .engine import Engine
from .env import mark
from .paths import CellPath
from .solvers import (INF, GASolver, ga_pad_and_sort, ga_random_chromosomes_native, ga_result_tuple, ga_row_individual,
                      ga_take_feasible, pack_path_rows)


class GaPopulation:
    """Population k of a GABatch, with GASolver's read surface (ga_solver.py:30-35, :162-218)."""

    def __init__(self, batch, k):
        self._b, self.k = batch, k
        self.start_node, self.target_node = batch.starts[k], batch.targets[k]
        self.seed = batch.seeds[k]
        self.convergence_curve = []
        self.best_solution_overall = {"fitness": INF, "path": []}
        self.attempts = 0                   # initial attempts made (ga_solver.py:100-114)
        self._init = []                     # the individuals begin() has collected
        self._solo = None                   # a degenerate population: the solo GASolver that ran it (GABatch docstring)
        self._result = None

    @property
    def population(self):
        """The reference's list of dicts in the population's current (sorted) order; materialised on demand."""
        return self._solo.population if self._solo is not None else self._b._population_of(self.k)

    def result(self):
        """What GASolver.solve() returns."""
        return self._result if self._solo is not None else ga_result_tuple(self.best_solution_overall)


class GABatch(WaypointBatch):
    _solver, _unit, _wp, _mirror = "GA", "population", "wp_cells", ("best_solution_overall", "convergence_curve")

    def __init__(self, grid, num_generations, population_size, num_waypoints_per_chromosome, mutation_rate, crossover_rate,
                 seeds=(), starts=None, targets=None, tournament_size=3, turn_penalty_factor=0.1, safety_penalty_factor=0.05,
                 min_safe_distance=1.5, allow_diagonal_moves=True, restrict_diagonal_near_obstacle_policy=True,
                 diagonal_obstacle_penalty_value=1000.0, engine=None, device=0, verbose=False):
        # every argument is checked before the device is touched
        self._check_sizes(grid, seeds, "population_size", population_size, "num_waypoints_per_chromosome", num_waypoints_per_chromosome,
                          "num_generations", num_generations)
        if not 1 <= int(tournament_size) <= 64:
            raise ValueError("GABatch: tournament_size must be in [1, 64]")
        self.num_generations, self.population_size = int(num_generations), self._N
        self.mutation_rate, self.crossover_rate, self.tournament_size = mutation_rate, crossover_rate, int(tournament_size)
        self._occ = self.grid == 1
        self._open(starts, targets, allow_diagonal_moves, restrict_diagonal_near_obstacle_policy,
                   dict(turn_penalty_factor=turn_penalty_factor, safety_penalty_factor=safety_penalty_factor,
                        min_safe_distance=min_safe_distance, diagonal_obstacle_penalty_value=diagonal_obstacle_penalty_value),
                   engine, lambda: Engine(self.grid, device), GaPopulation, verbose)      # (Engine: this module's name for it)

    def population(self, k):
        return self._units[k]

    # ------------------------------------------------------------------ initialisation (WaypointBatch.begin)
    def _solo_solver(self, k):
        return GASolver(mark(self.grid, self.starts[k], self.targets[k]), self.num_generations, self.population_size,
                        self.num_waypoints, self.mutation_rate, self.crossover_rate, tournament_size=self.tournament_size,
                        allow_diagonal_moves=self.allow_diagonal_moves,
                        restrict_diagonal_near_obstacle_policy=self.restrict_diagonal_near_obstacle_policy, engine=self.engine,
                        seed=self.seeds[k], verbose=self.verbose, **self._weights)

    def _draw(self, p, n):
        return (ga_random_chromosomes_native(p.seed, p.attempts, n, self.num_waypoints, self._occ),)

    def _take(self, p, draw, cps, stats, feas):
        ga_take_feasible(p._init, self.population_size, draw[0], cps, stats, feas, self.cols)

    def _to_device(self):
        """ga_solver.py:130-132 and :167-171 for the live populations, then their move into HBM, back to back in batch order:
        row j N + i = individual i of live population j."""
        e, N, W, cap, live = self.engine, self.population_size, self.num_waypoints, self.path_cap, self.live
        Kb = len(live)
        d = {"cur": 0}
        self._d = d
        if not Kb:
            return
        ind = []
        for p in (self._units[k] for k in live):
            pop, p._init = p._init, None
            ga_pad_and_sort(pop, N, p.seed)                          # :130-132
            p.best_solution_overall = pop[0].copy()                  # :170
            p.convergence_curve.append(p.best_solution_overall["fitness"])
            ind += pop
        chrom = np.stack([x["_cells"] for x in ind]).astype(np.int32)
        stats = np.array([[x["length"], x["turns"], x["safety_penalty"], x["diag_penalty"], x["fitness"]] for x in ind], np.float64)
        cells, lens = pack_path_rows([x["path"] for x in ind], self.cols, cap, "GA")
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
        self._check_begun()
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
            p, sid, s5 = self._units[k], int(rows[j, 0]), rows[j, 1:].copy()
            if s5[4] < p.best_solution_overall["fitness"]:                                                             # :212-213
                r = j * N + sid
                ch = d["chrom"][cur].read(r * W, W)
                L = int(d["len"][cur].read(r, 1)[0])
                p.best_solution_overall = ga_row_individual(ch, CellPath(d["cells"][cur].read(r * cap, L), self.cols), s5, self.cols)
            p.convergence_curve.append(p.best_solution_overall["fitness"])
        if self.verbose and ((gen + 1) % 10 == 0 or gen == 0 or gen == self.num_generations - 1):
            best = min(self._units[k].best_solution_overall["fitness"] for k in self.live)
            print(f"GABatch Gen {gen + 1}/{self.num_generations}: K={self.K}, BestFit={best:.2f}")

    def solve(self):
        """-> the K result tuples, each what GASolver.solve() returns."""
        self.begin()
        for gen in range(self.num_generations):
            self.step(gen)
        return [p.result() for p in self._units]
