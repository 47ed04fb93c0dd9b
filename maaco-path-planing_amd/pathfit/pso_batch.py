"""K independent PSO swarms in one batched sweep (pf_decode_batch_multi, pf_pso_*_batch).

A swarm is one PSOSolver run with its own seed, start cell and target cell; the swarms of a batch share the grid,
`num_particles` (N), `num_waypoints_per_particle` (W), `num_iterations`, `w`, `c1`, `c2`, the move policy, the score parameters
and `asynchronous`.  Swarm k computes bit for bit what `PSOSolver(grid_k, ..., seed=seeds[k], asynchronous=...)` computes,
grid_k being the grid with its START / TARGET markers moved to (starts[k], targets[k]).

The asynchronous sweep (pso.py:222-229: a particle sees the gbest as the particles before it left it) is reproduced by
speculate-and-repair, as in the solo class: a ROUND evaluates, for every swarm, the particles from its first one that is not
final yet (`cur[k]`) to its last, all in one update launch, ONE decode launch -- every item carries its own start and target,
so the longest-first queue and the tail policy see the whole batch and one swarm's tail is filled with the others' chains --,
one scan launch and one commit launch.  In each swarm everything up to and including the first gbest improver is final; the
particles behind it are evaluated again in the next round with the moved gbest (their draws are keyed per particle, so they
draw the same numbers).  K solo swarms cost the SUM of their rounds in chain-bound launches per iteration, the batch the MAX.
The update writes into compact staging rows and the commit copies the final ones into the swarm, so nothing is rolled back.

Per round the host reads the K scan records (16 K bytes, one copy) and the decode's counter block and range flag, and uploads one
table of 4 (2 K + 1) bytes (the segment offsets and `cur`); no position, velocity, path or stats column crosses PCIe inside a
sweep, and a swarm's gbest path row is read only when somebody reads `gbest_particle_data`.

Initialisation (pso.py:97-161) runs in rounds: each round collects the next attempts of every swarm that is still short of N
feasible particles and decodes them all in one multi-endpoint launch.

Degenerate swarms: when none of a swarm's 20 * N random attempts decodes, the solo class takes the direct A* path as its one
particle (pso.py:126-143) or has no particle at all -> `([], inf, 0, 0.0, 0.0, inf)`.  PSOBatch does not re-implement that
branch: such a swarm is handed, whole, to an internal solo PSOSolver on the same engine during `begin()`, and its result is
reported in its place (`sweep()` reports its convergence curve); the other swarms run batched.

The batch owns its buffers and the library entries are stateless, so a solo solver or another batch on the same Engine is not
disturbed, and `Engine.update_grid` has nothing to invalidate.  A batch is single-GPU (no `comm`) and always speculates on
every particle that is not final (no `max_speculation`).
"""
import numpy as np

from ._batch import WaypointBatch
from .engine import Engine
from .env import mark
from .paths import CellPath
from .solvers import (INF, PSOSolver, pack_path_rows, pso_attempt_draws, pso_gbest_record, pso_pad, pso_particle_dicts, pso_result_tuple,
                      pso_take_feasible)

SCAN_REC = np.dtype([("idx", "<i4"), ("ovf", "<i4"), ("fit", "<f8")])       # PsoScanRec (csrc/pf_pso_batch.h)


class PsoSwarm:
    """Swarm k of a PSOBatch, with PSOSolver's read surface (pso.py:37-38, :163-240)."""

    def __init__(self, batch, k):
        self._b, self.k = batch, k
        self.start_node, self.target_node = batch.starts[k], batch.targets[k]
        self.seed = batch.seeds[k]
        self.convergence_curve = []
        self.rounds = []                    # per sweep: the rounds in which the swarm had particles to evaluate
        self.attempts = 0                   # initial attempts made (pso.py:99-103)
        self._init = ([], [], [], [])       # the particles begin() has collected: positions, velocities, paths, stats
        self._gbest = {"fitness": INF, "path": [], "position": []}
        self._gdev = None                   # the gbest has moved on the device: {"idx", "fitness", "host": the record was read}
        self._solo = None                   # a degenerate swarm: the solo PSOSolver that ran it (PSOBatch docstring)
        self._result = None

    @property
    def gbest_particle_data(self):
        """The reference's gbest dict; its path row and stats are read from HBM when somebody asks."""
        return self._solo.gbest_particle_data if self._solo is not None else self._b._gbest_of(self)

    @property
    def particles(self):
        """The reference's list of particle dicts; materialised on demand."""
        return self._solo.particles if self._solo is not None else self._b._particles_of(self.k)

    def result(self):
        """What PSOSolver.solve() returns."""
        return self._result if self._solo is not None else pso_result_tuple(self.gbest_particle_data)


class PSOBatch(WaypointBatch):
    _solver, _unit, _wp, _mirror = "PSO", "swarm", "wp_pos", ("convergence_curve",)

    def __init__(self, grid, num_iterations, num_particles, num_waypoints_per_particle, w, c1, c2, seeds=(), starts=None, targets=None,
                 turn_penalty_factor=0.1, safety_penalty_factor=0.05, min_safe_distance=1.5, allow_diagonal_moves=True,
                 restrict_diagonal_near_obstacle_policy=True, diagonal_obstacle_penalty_value=1000.0, asynchronous=True, engine=None,
                 device=0, verbose=False):
        # every argument is checked before the device is touched
        self._check_sizes(grid, seeds, "num_particles", num_particles, "num_waypoints_per_particle", num_waypoints_per_particle,
                          "num_iterations", num_iterations)
        self.num_iterations, self.num_particles = int(num_iterations), self._N
        self.w, self.c1, self.c2 = w, c1, c2
        self.max_vel = max(1.0, 0.15 * max(self.rows, self.cols))      # pso.py:34
        self.asynchronous = bool(asynchronous)
        self._it = 0                        # sweeps made
        self._open(starts, targets, allow_diagonal_moves, restrict_diagonal_near_obstacle_policy,
                   dict(turn_penalty_factor=turn_penalty_factor, safety_penalty_factor=safety_penalty_factor,
                        min_safe_distance=min_safe_distance, diagonal_obstacle_penalty_value=diagonal_obstacle_penalty_value),
                   engine, lambda: Engine(self.grid, device), PsoSwarm, verbose)          # (Engine: this module's name for it)

    def swarm(self, k):
        return self._units[k]

    # ------------------------------------------------------------------ initialisation (WaypointBatch.begin)
    def _solo_solver(self, k):
        return PSOSolver(mark(self.grid, self.starts[k], self.targets[k]), self.num_iterations, self.num_particles, self.num_waypoints,
                         self.w, self.c1, self.c2, allow_diagonal_moves=self.allow_diagonal_moves,
                         restrict_diagonal_near_obstacle_policy=self.restrict_diagonal_near_obstacle_policy, engine=self.engine,
                         seed=self.seeds[k], verbose=self.verbose, asynchronous=self.asynchronous, **self._weights)

    def _draw(self, p, n):
        return pso_attempt_draws(p.seed, p.attempts, n, self.num_waypoints, self.rows, self.cols, self.max_vel)

    def _take(self, p, draw, cps, stats, feas):
        pso_take_feasible(p._init, self.num_particles, draw[0], draw[1], cps, stats, feas)

    def _to_device(self):
        """pso.py:159-160 and the :121 gbest scan for the live swarms, and their move into HBM, back to back in batch order:
        row j N + a = particle a of live swarm j."""
        e, N, W, cap, live = self.engine, self.num_particles, self.num_waypoints, self.path_cap, self.live
        Kb = len(live)
        d = {}
        self._d = d
        if not Kb:
            return
        KN = Kb * N
        sw = ([], [], [], [])                                          # (positions, velocities, paths, stats) of all of them
        for p in (self._units[k] for k in live):
            pso_pad(p._init, N, p.seed)                                # :159-160
            for all_, own in zip(sw, p._init):
                all_ += own
            p._init = None
        pos, vel = np.array(sw[0], np.float64).reshape(KN, W, 2), np.array(sw[1], np.float64).reshape(KN, W, 2)
        stats = np.array(sw[3], np.float64).reshape(KN, 5)
        cells, lens = pack_path_rows(sw[2], self.cols, cap, "PSO")
        gb, gstats, gpath = np.zeros((Kb, W, 2)), np.zeros((Kb, 5)), np.zeros((Kb, cap + 1), np.int32)
        for j, p in enumerate(self._units[k] for k in live):
            g = j * N + int(np.argmin(stats[j * N:(j + 1) * N, 4]))    # first minimum == the sequential :121 scan
            gb[j], gstats[j], gpath[j, 0], gpath[j, 1:] = pos[g], stats[g], lens[g], cells[g]
            p._gbest = pso_gbest_record(pos[g], sw[2][g], stats[g])
            p.convergence_curve.append(p._gbest["fitness"])
        d["seeds"] = e.put(np.array([self.seeds[k] for k in live], np.uint64))
        d["start"], d["target"] = e.put(self._s[live]), e.put(self._t[live])                                  # per SWARM
        d["pos"], d["vel"], d["pb"], d["pbf"] = e.put(pos), e.put(vel), e.put(pos), e.put(stats[:, 4].copy())   # pso.py:111-117
        d["cells"], d["len"], d["stats"] = e.put(cells), e.put(lens), e.put(stats)
        d["pb_cells"], d["pb_len"] = e.put(cells), e.put(lens)
        d["gb"], d["gstats"], d["gpath"], d["gfit"] = e.put(gb), e.put(gstats), e.put(gpath), e.put(gstats[:, 4].copy())
        d["tab"], d["rec"] = e.buf(2 * Kb + 1, np.int32), e.buf((Kb, 2), np.float64)
        # staging: one row per item of a round
        d["s_pos"], d["s_vel"] = e.buf((KN, W, 2), np.float64), e.buf((KN, W, 2), np.float64)
        d["s_start"], d["s_target"], d["s_row"] = e.buf(KN, np.int32), e.buf(KN, np.int32), e.buf(KN, np.int32)
        d["s_cells"], d["s_len"], d["s_st"], d["s_stats"] = e.buf((KN, cap), np.int32), e.buf(KN, np.int32), e.buf(KN, np.int32), e.buf((KN, 5), np.float64)
        self._gfit = [float(v) for v in gstats[:, 4]]
        self._rec = np.empty(Kb, SCAN_REC)

    # ------------------------------------------------------------------ device state, for readers and tests
    def device_state(self, k):
        """(pos [N][W][2], vel, pbest, pbest_fit [N], cells [N][cap], len [N], stats [N][5], pb_cells [N][cap], pb_len [N]) of
        live swarm k: host copies."""
        self._check_begun()
        if k not in self.live:
            raise ValueError(f"PSOBatch: swarm {k} is degenerate and has no rows in the batch (read swarm({k}).particles)")
        d, N, W, cap, r0 = self._d, self.num_particles, self.num_waypoints, self.path_cap, self.live.index(k) * self.num_particles
        w2 = W * 2
        return (d["pos"].read(r0 * w2, N * w2).reshape(N, W, 2), d["vel"].read(r0 * w2, N * w2).reshape(N, W, 2),
                d["pb"].read(r0 * w2, N * w2).reshape(N, W, 2), d["pbf"].read(r0, N), d["cells"].read(r0 * cap, N * cap).reshape(N, cap),
                d["len"].read(r0, N), d["stats"].read(r0 * 5, N * 5).reshape(N, 5), d["pb_cells"].read(r0 * cap, N * cap).reshape(N, cap),
                d["pb_len"].read(r0, N))

    def _particles_of(self, k):
        pos, vel, pb, pbf, cells, lens, stats, pbc, pbl = self.device_state(k)
        n = len(lens)
        return pso_particle_dicts(pos, vel, pb, pbf, [CellPath(pbc[i, :pbl[i]].copy(), self.cols) for i in range(n)],
                                  [CellPath(cells[i, :lens[i]].copy(), self.cols) for i in range(n)], stats)

    def _gbest_of(self, p):
        g = p._gdev
        if g is not None and not g["host"]:
            self._check_begun()
            d, W, cap, j = self._d, self.num_waypoints, self.path_cap, self.live.index(p.k)
            pos = d["gb"].read(j * W * 2, W * 2).reshape(-1, 2)
            L = int(d["gpath"].read(j * (cap + 1), 1)[0])               # the row k_pso_commit_batch left in HBM: length, cells
            p._gbest = pso_gbest_record(pos, CellPath(d["gpath"].read(j * (cap + 1) + 1, L), self.cols), d["gstats"].read(j * 5, 5))
            g["host"] = True
        return p._gbest

    # ------------------------------------------------------------------ one iteration
    def sweep(self):
        """One iteration of pso.py:178-231 for every live swarm -> the K gbest fitnesses.  A round is four launches whatever K is
        (update, decode, scan, commit), one read of the K scan records and one upload of the round's table."""
        self._check_begun()
        e, d, N, W, cap, live = self.engine, self._d, self.num_particles, self.num_waypoints, self.path_cap, self.live
        Kb, sync = len(live), 0 if self.asynchronous else 1
        cur, rounds, rec = np.zeros(Kb, np.int64), [0] * Kb, self._rec if Kb else None
        while Kb and (cur < N).any():
            cnt = N - cur                                              # swarm j evaluates its particles [cur[j], N)
            off = np.concatenate([[0], np.cumsum(cnt)])
            n = int(off[-1])
            d["tab"].upload(np.concatenate([off, cur]).astype(np.int32))
            e.pso_update_batch(n, Kb, N, W, self.w, self.c1, self.c2, self.max_vel, self._it, d["seeds"], d["tab"], d["start"], d["target"],
                               d["pos"], d["vel"], d["pb"], d["gb"], d["s_pos"], d["s_vel"], d["s_start"], d["s_target"], d["s_row"])   # :186-202
            e.decode_multi(n, W, d["s_start"], d["s_target"], cap, d["s_cells"], d["s_len"], d["s_st"], None, d["s_pos"], self._sp,
                           d["s_stats"], self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle_policy)                      # :209-214 the hot path
            e.pso_scan_batch(Kb, N, sync, d["tab"], d["s_stats"], d["s_len"], d["s_st"], d["pbf"], d["gfit"], d["rec"], rec)
            if rec["ovf"].any():
                raise RuntimeError("pathfit: scratch/path capacity overflow in PSO decode")
            e.pso_commit_batch(n, Kb, N, W, cap, sync, d["tab"], d["rec"], d["s_row"], d["s_pos"], d["s_vel"], d["s_stats"], d["s_len"],
                               d["s_cells"], d["pos"], d["vel"], d["stats"], d["len"], d["cells"], d["pb"], d["pbf"], d["pb_cells"],
                               d["pb_len"], d["gb"], d["gstats"], d["gpath"], d["gfit"])                                              # :216-229
            for j in range(Kb):
                if not cnt[j]:
                    continue
                rounds[j] += 1
                idx = int(rec["idx"][j])
                if idx >= 0:                                           # pso.py:222-229: the swarm's gbest moves to particle cur + idx
                    self._gfit[j] = float(rec["fit"][j])
                    self._units[live[j]]._gdev = {"idx": int(cur[j]) + idx, "fitness": self._gfit[j], "host": False}
                cur[j] = cur[j] + idx + 1 if (idx >= 0 and self.asynchronous) else N
        it = self._it = self._it + 1
        out = []
        for k, p in enumerate(self._units):
            if p._solo is not None:                                    # ran whole in begin(): its curve is reported
                c = p.convergence_curve
                out.append(c[min(it, len(c) - 1)] if c else INF)
                continue
            j = live.index(k)
            p.rounds.append(rounds[j])
            p.convergence_curve.append(self._gfit[j])
            out.append(self._gfit[j])
        if self.verbose and (it % 10 == 0 or it == 1 or it == self.num_iterations):
            print(f"PSOBatch Iter {it}/{self.num_iterations}: K={self.K}, GBestFit={min(out):.2f}")
        return out

    def solve(self):
        """-> the K result tuples, each what PSOSolver.solve() returns."""
        self.begin()
        for _ in range(self.num_iterations):
            self.sweep()
        return [p.result() for p in self._units]
