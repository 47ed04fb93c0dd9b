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

from ._field import Field
from ._lib import PathfitError
from .assignment import chunk_rows
from .cost_field import checked_cost
from .engine import Engine
from .paths import CellPath
from .tour_search import BIG, MOVES_MAX, STARTS_MAX, _int_in

SITES_MAX, DEMANDS_MAX, OPEN_MAX = 1024, 4096, 64                    # PF_PLACE_SITES_MAX, PF_PLACE_DEMANDS_MAX, PF_PLACE_OPEN_MAX
OBJECTIVES = {"sum": 0, "max": 1}

Improved = collections.namedtuple("Improved", "row owner value status info")
Cost = collections.namedtuple("Cost", "total radius unserved")


def _mode(who, objective):
    if not isinstance(objective, str) or objective not in OBJECTIVES:
        raise ValueError(f"{who}: objective must be 'sum' or 'max', got {objective!r}")
    return OBJECTIVES[objective]


def _shape_check(who, m, n, p):
    if m < 1:
        raise ValueError(f"{who}: sites is empty")
    if n < 1:
        raise ValueError(f"{who}: demands is empty")
    if m > SITES_MAX:
        raise ValueError(f"{who}: {m} sites; at most {SITES_MAX} are searched")
    if n > DEMANDS_MAX:
        raise ValueError(f"{who}: {n} demands; at most {DEMANDS_MAX} are served")
    if not isinstance(p, (int, np.integer)) or isinstance(p, bool) or not 1 <= int(p) <= min(m, OPEN_MAX):
        raise ValueError(f"{who}: count must be an integer in [1, {min(m, OPEN_MAX)}] (at most the sites, at most {OPEN_MAX}), got {p!r}")
    return int(p)


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


def perturbed(row, fixed, draws):
    """A perturbed start: per draw (s, i) slot fixed + s takes site i if i is not in the row, else the draw is dropped."""
    out = [int(v) for v in row]
    for s, i in draws:
        if int(i) not in out:
            out[fixed + int(s)] = int(i)
    return out


def perturbations(rng, row, fixed, m, starts):
    """`starts` perturbed starts of a row: one rng.integers(0, [p - f, m], (starts, Q, 2)) draw with Q = max(1, (p - f) // 4)."""
    p = len(row)
    draws = rng.integers(0, [p - fixed, m], (starts, max(1, (p - fixed) // 4), 2))
    return [perturbed(row, fixed, draws[s]) for s in range(starts)]


def _improve(e, mode, m, n, fixed, dm, shared, rows, limit):
    """One pf_place_improve call over the start rows [B, p] -> (Improved, kernel ms)."""
    rows = np.ascontiguousarray(rows, np.int32)
    B, p = rows.shape
    ds = e.put(rows.reshape(-1), np.int32)
    do, dv, dst, di = e.buf((B, n), np.int32), e.buf((B, 4), np.float64), e.buf(B, np.int32), e.buf((B, 4), np.int64)
    try:
        e.place_improve(mode, m, n, p, fixed, B, shared, dm, limit, ds, do, dv, dst, di)
        ms = e.last_kernel_ms()
        return Improved(ds.download().reshape(B, p).astype(np.int32), do.download().reshape(B, n).astype(np.int32), dv.download().reshape(B, 4),
                        dst.download().reshape(B), di.download().reshape(B, 4)), ms
    finally:
        for b in (ds, do, dv, dst, di):
            b.free()


def search(e, mode, m, n, p, keep, dm, starts, rounds, seed, limit):
    """The search over the matrix dm holds -> dict(row, owner, total, radius, unserved, history, moves, kernel_ms).  Round 0 improves
    [keep..., -1, ...]; each later round improves `starts` perturbations of the incumbent in one call and keeps the strictly smallest
    key at the smallest start index.  With every slot kept there are no later rounds."""
    f = len(keep)
    got, ms = _improve(e, mode, m, n, f, dm, True, [[int(v) for v in keep] + [-1] * (p - f)], limit)

    def key(g, x):
        return key_of(mode, g.info[x, 2], g.value[x, 0], g.value[x, 1])
    best, row, owner, value, uns = key(got, 0), got.row[0], got.owner[0], got.value[0], int(got.info[0, 2])
    history, moves = [best], int(got.info[0, 0])
    rng = np.random.default_rng(seed)
    for _ in range(rounds if p > f else 0):
        got, t = _improve(e, mode, m, n, f, dm, True, perturbations(rng, row, f, m, starts), limit)
        ms += t
        moves += int(got.info[:, 0].sum())
        keys = [key(got, x) for x in range(len(got.row))]
        x = keys.index(min(keys))                                     # (the first smallest)
        if keys[x] < best:
            best, row, owner, value, uns = keys[x], got.row[x], got.owner[x], got.value[x], int(got.info[x, 2])
        history.append(best)
    return dict(row=row, owner=owner, total=float(value[0]), radius=float(value[1]), unserved=uns, history=history, moves=moves, kernel_ms=ms)


class Placement(Field):
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
    _bufs = ("buf", "pbuf", "mbuf", "cost_device")
    CHUNK_BYTES = 256 << 20

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
        try:
            keep = list(keep)
        except TypeError:
            raise ValueError(f"{who}: keep must be a list of indices into sites, got {keep!r}") from None
        self.keep = [self._index(f"keep[{x}]", v, self.m) for x, v in enumerate(keep)]
        if len(set(self.keep)) != len(self.keep):
            raise ValueError(f"{who}: keep names a site twice")
        if len(self.keep) > self.count:
            raise ValueError(f"{who}: keep holds {len(self.keep)} sites, more than count = {self.count}")
        self.cost = None if cost is None else checked_cost(who, self.grid, cost)
        self.starts = _int_in(who, "starts", starts, 1, STARTS_MAX)
        self.rounds = _int_in(who, "rounds", rounds, 0, 1 << 20)
        self.seed = _int_in(who, "seed", seed, 0, (1 << 63) - 1)
        limit = _int_in(who, "max_moves", max_moves, 0, MOVES_MAX, none_ok=True)
        self.max_moves = 16 * self.count if limit is None else limit
        self.allow_diagonal_moves = bool(allow_diagonal_moves)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self.chunk = chunk_rows(self.m, self.rows * self.cols, self.CHUNK_BYTES)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        e = self.engine
        self.cost_device = None if self.cost is None else e.put(self.cost.reshape(-1), np.float64)
        self.buf = e.buf((self.chunk, self.rows, self.cols), np.float64)
        self.mbuf = e.buf((self.m, self.n), np.float64)
        self.pbuf = None
        self._compute()

    def _check_open(self):
        if self.buf is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the placement is closed")

    def _fields(self, r0):
        """The fields of the sites r0 .. r0 + c - 1 into buf (c = the chunk's rows) -> c."""
        e, c = self.engine, min(self.chunk, self.m - r0)
        ids = self.site_ids[r0:r0 + c]
        if self.cost_device is None:
            e.dist_field_batch(ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        else:
            e.cost_field(self.cost_device, np.arange(c + 1, dtype=np.int32), ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        self._held = r0
        return c

    def _compute(self):
        e = self.engine
        ms = 0.0
        for r0 in range(0, self.m, self.chunk):
            c = self._fields(r0)
            ms += e.last_kernel_ms()
            e.assign_matrix(c, self.demand_ids, self.buf, self.mbuf, r0, self.n, False)
            ms += e.last_kernel_ms()
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
        """One entry per demand: the CellPath from its open site's cell to the demand, None for an unserved demand.  Each is
        DistanceField.paths' route cell for cell: a parent-map call over a chunk of the sites' fields and one trace call with a
        field index per query.  A chunk of fields that was released for a later one is computed again."""
        self._check_open()
        e, full = self.engine, self.rows * self.cols
        ad, rs = self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle
        site_of = [self.sites[int(o)] if o >= 0 else -1 for o in self.owner]
        out = [None] * self.n
        for r0 in sorted(range(0, self.m, self.chunk), key=lambda r: r != self._held):      # the chunk held first: it is not computed again
            mine = [j for j in range(self.n) if r0 <= site_of[j] < r0 + self.chunk]
            if not mine:
                continue
            c = min(self.chunk, self.m - r0)
            if self._held != r0:
                self._fields(r0)
                if self.pbuf is not None:
                    self.pbuf.free()
                    self.pbuf = None
            if self.pbuf is None:
                pbuf = e.buf((self.chunk, self.rows, self.cols), np.uint8)
                try:
                    if self.cost_device is None:
                        e.dist_field_parents(c, self.buf, pbuf, ad, rs)
                    else:
                        e.cost_field_parents(self.cost_device, c, self.buf, pbuf, ad, rs)
                except Exception:
                    pbuf.free()
                    raise
                self.pbuf = pbuf
            q = len(mine)
            dk = e.put(np.array([site_of[j] - r0 for j in mine], np.int32))
            dt = e.put(self.demand_ids[np.array(mine)].astype(np.int32))
            dl, dst = e.buf(q, np.int32), e.buf(q, np.int32)
            dcl, cap = None, e.default_path_cap()
            try:
                while True:
                    dcl = e.buf((q, cap), np.int32)
                    e.dist_field_paths(c, self.pbuf, dt, q, cap, dcl, dl, dst, dk, self.buf, False, None)
                    st = dst.download()
                    if cap >= full or not (st == 3).any():
                        break
                    dcl.free()
                    dcl, cap = None, full
                if (st == 3).any():
                    raise PathfitError(f"{type(self).__name__}: {int((st == 3).sum())} routes hold more than {cap} cells")
                lens, cells = dl.download(), dcl.download().reshape(q, cap)
                for x, j in enumerate(mine):
                    out[j] = CellPath(cells[x, :lens[x]].copy(), self.cols)
            finally:
                for b in (dk, dt, dl, dst, dcl):
                    if b is not None:
                        b.free()
        return out

    def refresh(self, cost=None):
        """Search the sites again on the map the engine holds now (after engine.update_grid) and, when given, under a new cost map
        (for a placement built with one)."""
        who = type(self).__name__
        self._check_open()
        if cost is not None and self.cost is None:
            raise ValueError(f"{who}: refresh(cost) needs a placement built with a cost map")
        held = getattr(self.engine, "grid_u8", None)
        grid = np.array(held, dtype=int) if held is not None else self.grid
        if self.cost is not None:
            new = checked_cost(who, grid, self.cost if cost is None else cost)
            if cost is not None:
                self.cost = new
                self.cost_device.upload(new.reshape(-1))
        self.grid = grid
        if self.pbuf is not None:
            self.pbuf.free()
            self.pbuf = None
        self._compute()
        return self

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
        try:
            a = np.ascontiguousarray(mats, np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: mats must be a [B, m, n] array of numbers") from None
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or min(a.shape) < 1:
            raise ValueError(f"{who}: mats has shape {a.shape}, not [B, m, n] with B, m, n >= 1")
        m, n = int(a.shape[1]), int(a.shape[2])
        if shared and a.shape[0] != 1:
            raise ValueError(f"{who}: shared=True takes one [m, n] matrix, got {a.shape[0]}")
        try:
            o = np.array(rows)
            o = o[None] if o.ndim == 1 else o
            ok = o.ndim == 2 and o.shape[0] >= 1 and o.shape[1] >= 1 and o.dtype.kind in "iu"
        except (TypeError, ValueError):
            ok = False
        if not ok or (not shared and o.shape[0] != a.shape[0]):
            raise ValueError(f"{who}: rows must be an integer array [B, p] with a row per matrix (any B >= 1 with shared=True)")
        p = _shape_check(who, m, n, int(o.shape[1]))
        fixed = _int_in(who, "fixed", fixed, 0, p)
        limit = _int_in(who, "max_moves", max_moves, 0, MOVES_MAX, none_ok=True)
        limit = 16 * p if limit is None else limit
        with np.errstate(invalid="ignore"):
            bad = np.argwhere(np.signbit(a) | ~((a <= BIG) | (a == np.inf)))      # (NaN fails the comparisons; -0.0 by its sign bit)
        if len(bad):
            b, i, j = (int(v) for v in bad[0])
            raise ValueError(f"{who}: mats[{b}, {i}, {j}] = {float(a[b, i, j])!r} is neither +inf nor a number in [+0.0, 2^1000]")
        for b, row in enumerate(o):
            seen = set()
            for s, v in enumerate(row):
                v = int(v)
                if not -1 <= v < m or v in seen or (v < 0 and s < fixed):
                    raise ValueError(f"{who}: rows[{b}, {s}] = {v}: a start holds sites of [0, {m}) or -1, no site twice, and no empty slot below fixed")
                if v >= 0:
                    seen.add(v)
        dm = engine.put(a.reshape(-1), np.float64)
        try:
            return _improve(engine, mode, m, n, fixed, dm, bool(shared), o, limit)[0]
        finally:
            dm.free()
