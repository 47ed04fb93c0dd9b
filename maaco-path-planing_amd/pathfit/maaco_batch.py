"""K independent MAACO colonies walked, scored and updated together (pf_maaco_batch_*).

The colonies share one grid, one set of hyper-parameters, `num_ants` and `num_iterations`; each has its own seed and its own
start / target.  One iteration of all of them is one walk over the K * num_ants ants, one best-of-iteration / take-over launch
and one pheromone pass, with one host wait.  Colony k computes bit for bit what a solo
`MAACO(grid_k, ..., seed=seeds[k])` computes, grid_k being the grid with its START / TARGET markers moved to
(starts[k], targets[k]).  The batch owns its state, so it never disturbs a solo MAACO on the same Engine.
"""
import ctypes as C

import numpy as np

from ._batch import EngineOwned, cell_ids, check_endpoints, check_grid_and_seeds
from ._lib import MaacoParams
from .engine import Engine, maaco_out13
from .maaco import grow_path_cap, take_iteration
from .paths import CellPath

INF = float("inf")


class MaacoColony:
    """Colony k of a MAACOBatch, with MAACO's public attributes (MAACO.py:47-48, :373)."""

    def __init__(self, batch, k):
        self._b, self.k = batch, k
        self.start_node, self.target_node = batch.starts[k], batch.targets[k]
        self.seed = batch.seeds[k]
        self._best_path, self._best_on_device = [], False
        self.best_path_length_overall = INF
        self.best_path_turns_overall = INF
        self.convergence_curve_data = []

    @property
    def best_path_overall(self):
        if self._best_on_device:
            self._best_path = CellPath(self._b._best_path_cells(self.k), self._b.cols).tolist()
            self._best_on_device = False
        return self._best_path

    @best_path_overall.setter
    def best_path_overall(self, v):
        self._best_path, self._best_on_device = v, False

    @property
    def pheromone_matrix(self):
        b = self._b
        t = np.empty((b.rows, b.cols), np.float64)
        b._ck(b.engine.L.pf_maaco_batch_get_pheromone(b._handle(), self.k, t.ctypes.data))
        return t

    @pheromone_matrix.setter
    def pheromone_matrix(self, tau):
        b = self._b
        t = np.ascontiguousarray(tau, np.float64)
        if t.size != b.rows * b.cols:
            raise ValueError("pheromone_matrix: wrong size")
        b._ck(b.engine.L.pf_maaco_batch_set_pheromone(b._handle(), self.k, t.ctypes.data))

    def result(self):
        return self.best_path_overall, self.best_path_length_overall, self.best_path_turns_overall


class MAACOBatch(EngineOwned):
    _destroy = "pf_maaco_batch_destroy"

    def __init__(self, grid, num_ants, num_iterations, alpha, beta, rho, Q, a_turn_coef, wh_max, wh_min,
                 k_h_adaptive, q0_initial, C0_initial_pheromone=0.1, seeds=(), starts=None, targets=None, engine=None,
                 device=0, verbose=False):
        # every argument is checked before the device is touched
        self.grid, self.seeds = check_grid_and_seeds("MAACOBatch", grid, seeds, "colony", "num_ants", num_ants)
        self.rows, self.cols = self.grid.shape
        K = len(self.seeds)
        self.starts, self.targets = check_endpoints("MAACOBatch", "MAACO", self.grid, starts, targets, K)
        self.K = K
        self.num_ants, self.num_iterations = int(num_ants), int(num_iterations)
        self.alpha, self.beta, self.rho, self.Q = alpha, beta, rho, Q
        self.a_turn_coef, self.wh_max, self.wh_min = a_turn_coef, wh_max, wh_min
        self.k_h_adaptive, self.q0_initial = k_h_adaptive, q0_initial
        self.C0_base = C0_initial_pheromone
        self.verbose = verbose
        self.engine = engine if engine is not None else Engine(self.grid, device)
        e = self.engine
        s, t = cell_ids(e, "MAACOBatch", self.grid, self.starts, self.targets)
        sd = np.array(self.seeds, np.uint64)
        params = MaacoParams(float(alpha), float(beta), float(rho), float(Q), float(a_turn_coef), float(wh_max), float(wh_min),
                             float(k_h_adaptive), float(q0_initial), float(C0_initial_pheromone), self.num_iterations,
                             int(s[0]), int(t[0]))
        b = C.c_void_p()
        self._b = None
        self._ck(e.L.pf_maaco_batch_create(e.h, C.byref(params), K, self.num_ants, s.ctypes.data, t.ctypes.data, sd.ctypes.data,
                                           C.byref(b)))
        self._b = b
        self.path_cap = min(self.rows * self.cols, 6 * (self.rows + self.cols) + 64)
        self._bufs = None
        self._out = np.empty((K, 13), np.float64)
        self._colonies = [MaacoColony(self, k) for k in range(K)]

    def colony(self, k):
        return self._colonies[k]

    def _alloc(self):
        e, m = self.engine, self.K * self.num_ants
        if self._bufs is None or self._bufs[0] != self.path_cap:
            self._bufs = (self.path_cap, e.buf((m, self.path_cap), np.int32), e.buf(m, np.int32), e.buf(m, np.float64),
                          e.buf(m, np.int32), e.buf(m, np.int32))
        return self._bufs[1:]

    def walk_bufs(self):
        """(cells [K n][cap], len, plen, turns, status) device buffers of the last iteration: colony k's ants are rows [k n, (k+1) n)."""
        return self._bufs[1:]

    def _best_path_cells(self, k):
        out = np.empty(self._bufs[0] if self._bufs else self.path_cap, np.int32)
        L = C.c_int32()
        self._ck(self.engine.L.pf_maaco_batch_best_path(self._handle(), int(k), out.ctypes.data, out.size, C.byref(L)))
        return out[:L.value]

    def iterate_dev(self, iter_num):
        """One iteration of every colony (MAACO.iterate_dev for each), with the same redo when a path row overflows (in any
        colony: then no colony's pheromone moved).  -> the K iteration-best lengths."""
        cols = self._colonies
        bl = np.array([c.best_path_length_overall for c in cols], np.float64)
        bt = np.array([float(c.best_path_turns_overall) for c in cols], np.float64)
        while True:
            dc, dl, dp, dt, ds = self._alloc()
            self._ck(self.engine.L.pf_maaco_batch_iterate(self._handle(), int(iter_num), self.num_ants, self.path_cap, dc.ptr, dl.ptr,
                                                          dp.ptr, dt.ptr, ds.ptr, bl.ctypes.data, bt.ctypes.data,
                                                          self._out.ctypes.data))
            if not grow_path_cap(self, self._out[0, 12]):                            # (else redo: tau was left untouched)
                return [take_iteration(c, maaco_out13(self._out[k])) for k, c in enumerate(cols)]

    def solve_path_planning(self):
        for iter_num in range(1, self.num_iterations + 1):
            ib = self.iterate_dev(iter_num)
            if self.verbose and (iter_num % 10 == 0 or iter_num == 1 or iter_num == self.num_iterations):
                best = min(c.best_path_length_overall for c in self._colonies)
                print(f"MAACOBatch Iter {iter_num}/{self.num_iterations}: K={self.K}, best iteration L={min(ib):.2f}, "
                      f"best overall L={best:.2f}")
        return [c.result() for c in self._colonies]
