"""K independent MPA schools swept together (pf_mpa_batch_*).

A school is one MPA population with its own seed, start cell and target cell; the schools of a batch share the grid,
`num_predators`, `num_iterations`, the hyper-parameters and the score parameters.  One iteration of all of them is one
segmented sort, one elite pick (a block per school), ONE longest-first work queue over the 2 * K * num_predators phase and FADs
items -- so one school's tail is filled with the others' searches -- and one gather of the K best rows.  School k computes bit
for bit what a solo `MPA(grid_k, ..., seed=seeds[k])` computes, grid_k being the grid with its START / TARGET markers moved to
(starts[k], targets[k]).  The batch owns its tables, so it never disturbs a solo MPA on the same Engine.  A batch is
single-GPU and always fused (no `agent0` / `n_local` / `fused`).

The host keeps, per school, what `MPA` keeps: CF (MPA.py:336) and the 4-level best-so-far tie-break (:415-437) on the
gathered best rows; a school's best path is read only when that school's best improves.
"""
import ctypes as C

import numpy as np

from ._batch import EngineOwned, cell_ids, check_endpoints, check_grid_and_seeds
from ._lib import Counters, MpaParams
from .engine import Engine, score_params
from .mpa import BestSoFar, cf_and_phase, levy_sigma
from .paths import CellPath


class MpaSchool(BestSoFar):
    """School k of an MPABatch, with MPA's read surface (MPA.py:30-36, :320-448)."""

    def __init__(self, batch, k):
        self._b, self.k = batch, k
        self.start_node, self.target_node = batch.starts[k], batch.targets[k]
        self.seed = batch.seeds[k]
        self._init_best()

    @property
    def order(self):
        """sorted position -> storage slot within the school (host copy on demand)."""
        N = self._b.num_predators
        return self._b.d_order.read(self.k * N, N)

    @property
    def population(self):
        """The reference's list of dicts, in the school's current (sorted) order; materialised on demand."""
        b, N = self._b, self._b.num_predators
        cap, r0 = b.path_cap, self.k * N
        cells = b.d_cells.read(r0 * cap, N * cap).reshape(N, cap)
        lens, stats = b.d_len.read(r0, N), b.d_stats.read(r0 * 5, N * 5).reshape(N, 5)
        out = []
        for slot in self.order:
            s = stats[slot]
            out.append({"path": CellPath(cells[slot, :lens[slot]].copy(), b.cols), "length": float(s[0]),
                        "turns": int(s[1]), "safety_penalty": float(s[2]), "diag_penalty": float(s[3]),
                        "fitness": float(s[4])})
        return out

    def _fetch(self, slot):
        return lambda: CellPath(self._b._path_of_slot(self.k, slot), self._b.cols).tolist()


class MPABatch(EngineOwned):
    _destroy = "pf_mpa_batch_destroy"

    def __init__(self, grid, num_predators, num_iterations, seeds=(), starts=None, targets=None, FADs_rate=0.2, P_const=0.5,
                 levy_beta=1.5, turn_penalty_factor=0.1, safety_penalty_factor=0.05, min_safe_distance=1.5,
                 allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, diagonal_obstacle_penalty=1000.0,
                 engine=None, device=0, verbose=False, path_cap=None):
        # every argument is checked before the device is touched
        self.grid, self.seeds = check_grid_and_seeds("MPABatch", grid, seeds, "school", "num_predators", num_predators)
        self.rows, self.cols = self.grid.shape
        K = len(self.seeds)
        if path_cap is not None and int(path_cap) < 2:
            raise ValueError("MPABatch: path_cap must be >= 2")
        self.starts, self.targets = check_endpoints("MPABatch", "MPA", self.grid, starts, targets, K)
        self.K = K
        self.num_predators, self.num_iterations = int(num_predators), int(num_iterations)
        self.FADs_rate, self.P_const, self.levy_beta = FADs_rate, P_const, levy_beta
        self.allow_diagonal_moves = allow_diagonal_moves
        self.restrict_diagonal_near_obstacle = restrict_diagonal_near_obstacle
        self.verbose = verbose
        self.engine = engine if engine is not None else Engine(self.grid, device)
        e = self.engine
        self._s, self._t = cell_ids(e, "MPABatch", self.grid, self.starts, self.targets)
        sd = np.array(self.seeds, np.uint64)
        self._sp = score_params(1, restrict_diagonal_near_obstacle, turn_penalty_factor, safety_penalty_factor,
                                min_safe_distance, diagonal_obstacle_penalty)
        params = MpaParams(float(P_const), float(levy_beta), levy_sigma(levy_beta), float(FADs_rate), self.num_predators,
                           int(self._s[0]), int(self._t[0]), int(bool(allow_diagonal_moves)),
                           int(bool(restrict_diagonal_near_obstacle)))
        b = C.c_void_p()
        self._b = None
        self._ck(e.L.pf_mpa_batch_create(e.h, C.byref(params), C.byref(self._sp), K, self._s.ctypes.data, self._t.ctypes.data,
                                         sd.ctypes.data, C.byref(b)))
        self._b = b
        self._fixed_cap = path_cap is not None       # an explicit path_cap is never grown: what does not fit is an error
        self.path_cap = int(path_cap) if self._fixed_cap else min(self.rows * self.cols, 8 * (self.rows + self.cols) + 64)
        self.path_cap = min(self.path_cap, self.rows * self.cols)
        self._schools = [MpaSchool(self, k) for k in range(K)]
        self._rows = np.empty((K, 6), np.float64)
        self._init_population()

    # ------------------------------------------------------------------
    def school(self, k):
        return self._schools[k]

    def create_ms(self):
        """Host wall time of pf_mpa_batch_create in ms: (initial searches + scores, bound tables, whole call)."""
        out = np.zeros(3, np.float64)
        self.engine.L.pf_mpa_batch_create_ms(self._handle(), out.ctypes.data)
        return tuple(float(v) for v in out)

    def counters(self):
        """(counters of the last sweep, items overflowed so far, proposals the host's libm resolved so far)."""
        c, ovf, dbt = Counters(), C.c_int64(), C.c_int64()
        self.engine.L.pf_mpa_batch_counters(self._handle(), C.byref(c), C.byref(ovf), C.byref(dbt))
        return {n: getattr(c, n) for n, _ in c._fields_}, ovf.value, dbt.value

    def _init_population(self):
        """MPA._initialize_population_with_safety (MPA.py:231-245) per school: N copies of its A*(start, target) path (the batch
        memoised it), or of the fallback [start, target] when the target is unreachable (:235-236)."""
        e, K, N, RC = self.engine, self.K, self.num_predators, self.rows * self.cols
        paths, buf, L = [], np.empty(RC, np.int32), C.c_int32()
        for k in range(K):
            self._ck(e.L.pf_mpa_batch_init_path(self._handle(), k, buf.ctypes.data, RC, C.byref(L), None))
            p = buf[:L.value].copy()
            if len(p) == 0:
                p = np.array([self._s[k], self._t[k]], np.int32)
            paths.append(p)
        longest = max(len(p) for p in paths)
        if self._fixed_cap and longest > self.path_cap:
            raise RuntimeError("pathfit: scratch/path capacity overflow: an initial path of %d cells (path_cap=%d)" % (longest, self.path_cap))
        while longest > self.path_cap:
            self.path_cap = min(RC, self.path_cap * 4)
        stats = e.score_host(paths, self._sp)
        cap = self.path_cap
        cells = np.zeros((K * N, cap), np.int32)
        for k, p in enumerate(paths):
            cells[k * N:(k + 1) * N, :len(p)] = p
        self.d_cells = e.put(cells)
        self.d_len = e.put(np.repeat(np.array([len(p) for p in paths], np.int32), N))
        self.d_stats = e.put(np.repeat(stats, N, axis=0))
        self.d_c1_cells, self.d_c1_len, self.d_c1_stats = e.buf((K * N, cap), np.int32), e.buf(K * N, np.int32), e.buf((K * N, 5), np.float64)
        self.d_c2_cells, self.d_c2_len, self.d_c2_stats = e.buf((K * N, cap), np.int32), e.buf(K * N, np.int32), e.buf((K * N, 5), np.float64)
        self.d_status = e.buf(K * N, np.int32)
        self.d_order = e.put(np.tile(np.arange(N, dtype=np.int32), K))   # per school: sorted position -> local slot
        self._sorted = False

    def _path_of_slot(self, k, slot):
        out, L = np.empty(self.path_cap, np.int32), C.c_int32()
        self._ck(self.engine.L.pf_mpa_batch_read_path(self._handle(), int(k), int(slot), self.path_cap, self.d_cells.ptr, self.d_len.ptr,
                                                      out.ctypes.data, out.size, C.byref(L)))
        return out[:L.value].copy()

    def _sort(self):
        """list.sort(key=fitness) of every school (MPA.py:321,:333,:412); skipped while no sweep has touched the populations since
        the last one (MPA._sort)."""
        if self._sorted:
            return
        self._ck(self.engine.L.pf_mpa_batch_sort(self._handle(), self.d_stats.ptr, self.d_order.ptr))
        self._sorted = True

    def _best_rows(self):
        self._ck(self.engine.L.pf_mpa_batch_best_rows(self._handle(), self.d_stats.ptr, self.d_order.ptr, self._rows.ctypes.data))
        return self._rows

    def step(self, it):
        """One iteration of MPA.py:332-440 for every school (it is 1-based).  -> the K best rows' stats [K][5]."""
        e, cap = self.engine, self.path_cap
        h = self._handle()
        self._sort()                                                     # :333
        self._ck(e.L.pf_mpa_batch_pick_elite(h, cap, self.d_cells.ptr, self.d_len.ptr, self.d_stats.ptr, self.d_order.ptr))   # :334
        CF, phase = cf_and_phase(it, self.num_iterations)                # :336
        self._sorted = False                                             # the sweep rewrites the populations
        self._ck(e.L.pf_mpa_batch_iterate(h, phase, CF, int(it), cap, self.d_cells.ptr, self.d_len.ptr, self.d_stats.ptr,
                                          self.d_order.ptr, self.d_c1_cells.ptr, self.d_c1_len.ptr, self.d_c1_stats.ptr,
                                          self.d_c2_cells.ptr, self.d_c2_len.ptr, self.d_c2_stats.ptr, self.d_status.ptr))   # :339-410
        n = self.counters()[0]["overflow_agents"]          # counted on the device: no status column leaves HBM
        if n:
            raise RuntimeError("pathfit: scratch/path capacity overflow on %d predators (path_cap=%d)" % (n, self.path_cap))
        self._sort()                                                     # :412
        rows = self._best_rows()
        for k, sc in enumerate(self._schools):
            sc._take(rows[k, 1:], sc._fetch(int(rows[k, 0])))            # :415-440
        return rows[:, 1:].copy()

    def begin(self):
        """MPA.py:321-330: the initial sort, best row and first point of the curve of every school."""
        self._sort()                                                     # :321
        rows = self._best_rows()
        for k, sc in enumerate(self._schools):
            sc._take_first(rows[k, 1:], sc._fetch(int(rows[k, 0])))      # :322-330

    def solve_path_planning(self):
        self.begin()
        for it in range(1, self.num_iterations + 1):
            s = self.step(it)
            if self.verbose and (it % 10 == 0 or it == 1 or it == self.num_iterations):
                best = min(sc.best_fitness_overall for sc in self._schools)
                print(f"MPABatch Iter {it}/{self.num_iterations}: K={self.K}, best iteration Fit={s[:, 4].min():.2f}, "
                      f"best overall Fit={best:.2f}")
        return [sc.result() for sc in self._schools]
