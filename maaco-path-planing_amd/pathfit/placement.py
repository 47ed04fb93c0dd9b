"""Placement: which `count` of the candidate cells to open -- chargers, depots, exits, parking cells -- so that the demand cells are
served best: the p-median ("sum": the smallest total path length from every demand to its nearest open site) or the p-center
("max": the smallest largest such length, the total behind it).  The fields come from the site cells chunk by chunk
(pf_dist_field_batch, or pf_cost_field under a cost map), each chunk is gathered at the demand cells into its row block of the
site-by-demand matrix in HBM (pf_assign_matrix), and the sites are searched on the device by pf_place_improve: best-improvement
additions and swaps from the row of the kept sites (so the device does the greedy construction), then rounds of perturbed
restarts of the incumbent, all starts of a round improved in one call over the one shared matrix.  The key begins with the number
of demands no open site reaches, so maps with sealed rooms get a site per room first.  The rule is identical run to run for a
given seed; `placement_cost` holds any other set against it.  `field` hands the open cells to NearestSourceField, `paths` traces
every served demand's route through the parent maps of the same fields."""
import collections

import numpy as np

from ._lib import PathfitError
from ._planner import BIG, OPEN_MAX, SITES_MAX, Planner, _int_in, as_matrices, improve_call, move_limit, no_bad_entry, one_if_shared  # noqa: F401
from ._planner import restarts, slot_count, slot_rows, start_rows
from ._planner import slot_perturbations as perturbations, slot_perturbed as perturbed  # noqa: F401  (they are imported from here)
from .engine import Engine

DEMANDS_MAX = 4096                                                   # PF_PLACE_DEMANDS_MAX
OBJECTIVES = {"sum": 0, "max": 1}

Improved = collections.namedtuple("Improved", "row owner value status info")
Cost = collections.namedtuple("Cost", "total radius unserved")


def _mode(who, objective):
    if not isinstance(objective, str) or objective not in OBJECTIVES:
        raise ValueError(f"{who}: objective must be 'sum' or 'max', got {objective!r}")
    return OBJECTIVES[objective]


def _shape_check(who, m, n, p):
    return slot_count(who, m, n, p, "demands", DEMANDS_MAX, "served")


def key_of(mode, unserved, total, radius):
    """The rule's key: (unserved, sum) for "sum", (unserved, max, sum) for "max"."""
    return (int(unserved), float(total)) if mode == 0 else (int(unserved), float(radius), float(total))


def set_cost(matrix, sites):
    """Cost(total, radius, unserved) of opening the rows `sites` of the matrix: per demand the smallest entry, the finite ones
    summed left to right (np.cumsum: np.sum is pairwise and is not the rule)."""
    a = np.asarray(matrix, np.float64)
    near = a[list(sites)].min(0) if len(sites) else np.full(a.shape[1], np.inf)
    fin = near != np.inf
    t = np.where(fin, near, 0.0)
    return Cost(float(np.cumsum(t)[-1]), float(t.max()), int((~fin).sum()))


def _improve(e, mode, m, n, fixed, dm, shared, rows, limit):
    """One pf_place_improve call over the start rows [B, p] -> (Improved, kernel ms)."""
    B, p = np.shape(rows)
    return improve_call(e, Improved, rows, (((B, n), np.int32), ((B, 4), np.float64), (B, np.int32), ((B, 4), np.int64)),
                        lambda ds, do, dv, dst, di: e.place_improve(mode, m, n, p, fixed, B, shared, dm, limit, ds, do, dv, dst, di))


def search(e, mode, m, n, p, keep, dm, starts, rounds, seed, limit):
    """The search over the matrix dm holds -> dict(row, owner, total, radius, unserved, history, moves, kernel_ms).  Round 0 improves
    [keep..., -1, ...]; each later round improves `starts` perturbations of the incumbent in one call and keeps the strictly smallest
    key at the smallest start index (restarts).  With every slot kept there are no later rounds."""
    f = len(keep)
    got, ms = _improve(e, mode, m, n, f, dm, True, [[int(v) for v in keep] + [-1] * (p - f)], limit)
    got, x, history, moves, t = restarts(got, rounds if p > f else 0, seed, lambda rng, row: perturbations(rng, row, f, m, starts),
                                         lambda rows: _improve(e, mode, m, n, f, dm, True, rows, limit),
                                         lambda g, b: key_of(mode, g.info[b, 2], g.value[b, 0], g.value[b, 1]))
    return dict(row=got.row[x], owner=got.owner[x], total=float(got.value[x, 0]), radius=float(got.value[x, 1]), unserved=int(got.info[x, 2]), history=history,
                moves=moves, kernel_ms=ms + t)


class Placement(Planner):
    """sites, demands: (r, c) pairs, at most 1024 candidate sites and 4096 demands (a demand listed twice counts twice).  count: the
    slots p, at most min(len(sites), 64); it includes `keep`, indices into `sites` that are open whatever happens.  objective:
    "sum" or "max".  cost: None (path lengths, pf_dist_field_batch) or an [R, C] cost map as CostField's (pf_cost_field).  starts,
    rounds, seed: `rounds` rounds of `starts` perturbed restarts drawn from np.random.default_rng(seed).  max_moves: the moves one
    start may take (None: 16 per slot).

    row: int32 [count], the slots (a candidate index or -1: a slot may stay empty where no addition changes the key).  sites: the
    open candidates' indices in slot order, the empty slots left out; cells: their (r, c).  total: the left-to-right sum of every
    served demand's distance to its nearest open site; radius: the largest; unserved: the demands no open site reaches; feasible:
    unserved == 0.  owner: int32 per demand, the position within `sites` of its nearest open site (the earliest slot on a tie), -1
    where unserved; loads: the demands per open site.  history: the key after round 0, 1, ... ((unserved, total) for "sum",
    (unserved, radius, total) for "max"); moves: the moves of all starts; matrix: float64 [candidates, demands]."""
    _closed, _built = "the placement is closed", "a placement"

    def __init__(self, grid, sites, demands, count, objective="sum", keep=(), cost=None, starts=8, rounds=3, seed=0, max_moves=None,
                 allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        who = type(self).__name__
        self._set_grid(grid)
        self.mode = _mode(who, objective)
        self.objective = objective
        self.site_ids, self.demand_ids = self._cell_ids("sites", sites), self._cell_ids("demands", demands)
        self.m, self.n = len(self.site_ids), len(self.demand_ids)
        self.count = _shape_check(who, self.m, self.n, count)
        self.candidates = [(int(v) // self.cols, int(v) % self.cols) for v in self.site_ids]
        self.demands = [(int(v) // self.cols, int(v) % self.cols) for v in self.demand_ids]
        self._set_keep(keep)
        self._set_cost_and_moves(cost, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        self._set_search(starts, rounds, seed, max_moves, self.count)
        e = self._open(engine, Engine, self.site_ids)                # every argument is checked: the device
        self.mbuf = e.buf((self.m, self.n), np.float64)
        self._compute()

    def _compute(self):
        e = self.engine
        ms = self._gather(lambda c, r0: e.assign_matrix(c, self.demand_ids, self.buf, self.mbuf, r0, self.n, False))
        self.matrix = self.mbuf.download().reshape(self.m, self.n)
        got = search(e, self.mode, self.m, self.n, self.count, self.keep, self.mbuf, self.starts, self.rounds, self.seed, self.max_moves)
        self.row = np.asarray(got["row"], np.int32)
        self.sites = [int(v) for v in self.row if v >= 0]
        self.cells = [self.candidates[v] for v in self.sites]
        self.total, self.radius, self.unserved = got["total"], got["radius"], got["unserved"]
        self.feasible = self.unserved == 0
        at = {v: x for x, v in enumerate(self.sites)}
        self.owner = np.array([at[int(v)] if v >= 0 else -1 for v in got["owner"]], np.int32)
        self.loads = [int((self.owner == x).sum()) for x in range(len(self.sites))]
        self.history, self.moves = got["history"], got["moves"]
        self.solve_kernel_ms = got["kernel_ms"]
        self.kernel_ms = ms + self.solve_kernel_ms

    def placement_cost(self, sites):
        """Cost(total, radius, unserved) of opening any other set of candidates (indices into the constructor's sites, no index
        twice) under `matrix` and the rule's left-to-right sum: what another heuristic's choice is compared with;
        placement_cost(self.sites) == (total, radius, unserved).  Host side."""
        who = type(self).__name__
        try:
            seq = [self._index(f"sites[{x}]", v, self.m) for x, v in enumerate(sites)]
        except TypeError:
            raise ValueError(f"{who}: sites must be a sequence of indices into the candidate sites, got {sites!r}") from None
        if len(set(seq)) != len(seq):
            raise ValueError(f"{who}: sites names a site twice")
        return set_cost(self.matrix, seq)

    def field(self):
        """A NearestSourceField over the open cells on the same engine: the distance of every cell to its nearest open site, and
        the owner map.  The caller closes it."""
        from .nearest_field import NearestSourceField
        self._check_open()
        if not self.cells:
            raise PathfitError(f"{type(self).__name__}: no site is open")
        return NearestSourceField(self.grid, [list(self.cells)], self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle, engine=self.engine)

    def paths(self):
        """One entry per demand: the CellPath from its open site's cell to the demand, None for an unserved demand (Planner._trace)."""
        self._check_open()
        served = [j for j in range(self.n) if self.owner[j] >= 0]
        out = [None] * self.n
        for j, path in zip(served, self._trace([(self.sites[int(self.owner[j])], int(self.demand_ids[j])) for j in served], "routes")):
            out[j] = path
        return out

    @classmethod
    def solve_matrices(cls, engine, mats, rows, objective="sum", fixed=0, shared=False, max_moves=None):
        """For callers with their own matrices and starts: mats float64 [B, m, n] -- or, with `shared`, one [m, n] for all starts --
        with mats[b, i, j] what demand j pays at site i (+inf or in [+0.0, 2^1000]; real-valued demand weights go here: scale the
        columns); rows int [B, p], the start rows (a site or -1 per slot, no site twice, the slots below `fixed` not empty: they
        are kept) -> Improved(row int32 [B, p], owner int32 [B, n] (a site or -1), value float64 [B, 4] = (sum after, max after, sum
        before, max before), status int32 [B]: 0 no better candidate is left, 2 stopped by max_moves (None: 16 p), info int64
        [B, 4] = (moves, sweeps, unserved after, unserved before))."""
        who = cls.__name__
        mode = _mode(who, objective)
        a = as_matrices(who, "mats", mats, "m", "n")
        m, n = int(a.shape[1]), int(a.shape[2])
        one_if_shared(who, shared, a, "[m, n] matrix")
        o = start_rows(who, "rows", rows, a, shared, "p")
        p = _shape_check(who, m, n, int(o.shape[1]))
        fixed = _int_in(who, "fixed", fixed, 0, p)
        limit = move_limit(who, max_moves, p)
        with np.errstate(invalid="ignore"):                           # (NaN fails the comparisons; -0.0 by its sign bit)
            no_bad_entry(who, "mats", a, np.signbit(a) | ~((a <= BIG) | (a == np.inf)), "neither +inf nor a number in [+0.0, 2^1000]")
        slot_rows(who, o, m, fixed)
        dm = engine.put(a.reshape(-1), np.float64)
        try:
            return _improve(engine, mode, m, n, fixed, dm, bool(shared), o, limit)[0]
        finally:
            dm.free()
