"""Coverage: which `count` of the candidate cells to open -- cameras, guards, chargers -- so that the most target cells are seen
(by="sight": a target counts where an open site has a free line of sight to it, Visibility's rule, within `max_range`) or reached
(by="reach": where it lies within `radius` of an open site by path length, or by weighted length under a cost map).  The masks come
from the site cells chunk by chunk (pf_visibility_field, or pf_dist_field_batch / pf_cost_field), each chunk is packed at the target
cells into its row block of the site-by-target bit masks in HBM, 64 targets a word (pf_cover_pack), and the sites are searched on
the device by pf_cover_improve: best-improvement additions, swaps and drops under the key (targets not covered, open sites) from
the row of the kept sites (so the device does the greedy construction and removes redundant sites), then rounds of perturbed
restarts of the incumbent, all starts of a round improved in one call over the one shared mask set.  Everything is an integer: the
result is identical run to run for a given seed; `coverage_of` holds any other set against it.  With count=None the rule answers
how few sites cover everything that can be covered."""
import collections
import math

import numpy as np

from ._lib import PathfitError
from ._planner import OPEN_MAX, SITES_MAX, Planner, _int_in, chunk_rows, improve_call, move_limit, one_if_shared, restarts  # noqa: F401
from ._planner import slot_count, slot_rows, start_rows
from ._planner import slot_perturbations as perturbations
from .engine import Engine
from .visibility import range_to_sq

ELEMS_MAX = 1 << 20                                                  # PF_COVER_ELEMS_MAX
KINDS = {"sight": 0, "reach": 1}

Improved = collections.namedtuple("Improved", "row covered value status info")


def words_of(n):
    return (int(n) + 63) // 64


def pack_bits(bits):
    """bool [..., n] -> uint64 [..., ceil(n / 64)]: element j is bit j & 63 of word j >> 6, the tail bits 0."""
    b = np.asarray(bits, bool)
    n = b.shape[-1]
    pad = np.zeros(b.shape[:-1] + (words_of(n) * 64,), bool)
    pad[..., :n] = b
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).reshape(-1).view("<u8").reshape(b.shape[:-1] + (words_of(n),))


def unpack_bits(words, n):
    """uint64 [..., W] -> bool [..., n]."""
    w = np.ascontiguousarray(words, "<u8")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (8 * w.shape[-1],)), axis=-1, bitorder="little")[..., :n].astype(bool)   # (a row count of 0 is legal)


def key_of(n, covered, open_sites):
    """The rule's key: (targets not covered, open sites)."""
    return int(n) - int(covered), int(open_sites)


def _shape_check(who, m, n, p):
    return slot_count(who, m, n, p, "targets", ELEMS_MAX, "covered")


def _improve(e, m, n, fixed, dm, shared, rows, limit):
    """One pf_cover_improve call over the start rows [B, p] -> (Improved, kernel ms)."""
    B, p = np.shape(rows)
    return improve_call(e, Improved, rows, (((B, words_of(n)), np.uint64), ((B, 4), np.int64), (B, np.int32), ((B, 4), np.int64)),
                        lambda ds, dc, dv, dst, di: e.cover_improve(m, n, p, fixed, B, shared, dm, limit, ds, dc, dv, dst, di))


def search(e, m, n, p, keep, dm, starts, rounds, seed, limit):
    """The search over the masks dm holds -> dict(row, covered, count, open, unique, history, moves, drops, kernel_ms).  Round 0
    improves [keep..., -1, ...]; each later round improves `starts` perturbations of the incumbent (Placement's stream) in one call
    and keeps the strictly smallest key at the smallest start index (restarts).  With every slot kept there are no later rounds."""
    f = len(keep)
    tried = []                                                        # every call's Improved: the drops are summed over all starts

    def improve(rows):
        tried.append(_improve(e, m, n, f, dm, True, rows, limit))
        return tried[-1]
    got, ms = improve([[int(v) for v in keep] + [-1] * (p - f)])
    got, x, history, moves, t = restarts(got, rounds if p > f else 0, seed, lambda rng, row: perturbations(rng, row, f, m, starts), improve,
                                         lambda g, b: key_of(n, g.value[b, 0], g.value[b, 1]))
    return dict(row=got.row[x], covered=got.covered[x], count=int(got.value[x, 0]), open=int(got.value[x, 1]), unique=int(got.info[x, 2]), history=history,
                moves=moves, drops=sum(int(g.info[:, 3].sum()) for g, _ in tried), kernel_ms=ms + t)


class Coverage(Planner):
    """sites: (r, c) pairs, at most 1024 candidate cells.  count: the slots p, at most min(len(sites), 64) (None: that); it includes
    `keep`, indices into `sites` that are open whatever happens.  targets: (r, c) pairs, at most 2^20 (None: every free cell in
    cell-id order; a target listed twice counts twice).  by: "sight" -- Visibility's rule from the site cells, max_range as
    Visibility's (None: no limit), restrict_diagonal_near_obstacle its strict rule -- or "reach" -- path length <= radius
    (pf_dist_field_batch; restrict_diagonal_near_obstacle the corner rule of the moves), or weighted length <= radius under `cost`,
    an [R, C] cost map as CostField's (pf_cost_field); radius is required, finite and >= 0.  starts, rounds, seed: `rounds` rounds of
    `starts` perturbed restarts drawn from np.random.default_rng(seed).  max_moves: the moves one start may take (None: 16 per slot).

    row: int32 [count], the slots (a candidate index or -1: a slot stays empty where no addition covers anything new).  sites: the
    open candidates' indices in slot order; cells: their (r, c).  covered: the targets some open site covers; coverage: covered / n;
    complete: covered == n.  mask: bool [n]; map(): bool [R, C].  seen_by: int32 [n], how many open sites cover each target;
    unique: per open site, the targets only it covers.  history: the key (not covered, open) after round 0, 1, ...; moves, drops:
    over all starts.  The packed masks stay in HBM (mask_device uint64 [m, ceil(n / 64)]); `masks` downloads them when asked."""
    _bufs = ("buf", "mask_device", "target_device", "cost_device")
    _closed, _built = "the coverage is closed", "a coverage"

    def __init__(self, grid, sites, count=None, targets=None, by="sight", max_range=None, radius=None, restrict_diagonal_near_obstacle=True, cost=None, keep=(),
                 starts=8, rounds=3, seed=0, max_moves=None, engine=None):
        who = type(self).__name__
        self._set_grid(grid)
        if not isinstance(by, str) or by not in KINDS:
            raise ValueError(f"{who}: by must be 'sight' or 'reach', got {by!r}")
        self.by, self.kind = by, KINDS[by]
        self.site_ids = self._cell_ids("sites", sites)
        if targets is None:
            self.target_ids = np.flatnonzero(self.grid.reshape(-1) != 1).astype(np.int32)
        else:
            self.target_ids = self._cell_ids("targets", targets)
        self.m, self.n = len(self.site_ids), len(self.target_ids)
        self.count = _shape_check(who, self.m, self.n, min(self.m, OPEN_MAX) if count is None and self.m >= 1 else count)
        self.candidates = [(int(v) // self.cols, int(v) % self.cols) for v in self.site_ids]
        self.targets = [(int(v) // self.cols, int(v) % self.cols) for v in self.target_ids]
        self._set_keep(keep)
        self.max_range, self.radius, self.cost = max_range, None, None
        if self.kind == 0:
            if radius is not None or cost is not None:
                raise ValueError(f"{who}: radius and cost belong to by='reach'")
            if self.rows * self.rows + self.cols * self.cols >= 2 ** 31 - 1:
                raise ValueError(f"{who}: R^2 + C^2 must stay below 2^31 - 1")
            try:
                self.range_sq = range_to_sq(max_range)
            except ValueError as err:
                raise ValueError(f"{who}: " + str(err).split(": ", 1)[1]) from None
        else:
            if max_range is not None:
                raise ValueError(f"{who}: max_range belongs to by='sight'")
            try:
                r = float(radius) if isinstance(radius, (int, float, np.integer, np.floating)) and not isinstance(radius, bool) else math.nan
            except (TypeError, ValueError):
                r = math.nan
            if not 0.0 <= r < math.inf:
                raise ValueError(f"{who}: radius must be a finite number >= 0, got {radius!r}")
            self.radius = r
        self._set_cost_and_moves(cost, True, restrict_diagonal_near_obstacle)
        self._set_search(starts, rounds, seed, max_moves, self.count)
        self.words = words_of(self.n)
        # a chunk holds at most CHUNK_BYTES of source rows: bytes for sight (an eighth of a double), doubles for reach
        chunk = chunk_rows(self.m, self.rows * self.cols, self.CHUNK_BYTES * (8 if self.kind == 0 else 1))
        e = self._open(engine, Engine, self.site_ids, chunk, np.uint8 if self.kind == 0 else np.float64)   # every argument is checked: the device
        self.target_device = e.put(self.target_ids, np.int32)
        self.mask_device = e.buf((self.m, self.words), np.uint64)
        try:
            self._compute()
        except BaseException:
            self.close()                                             # a failed constructor holds no HBM
            raise

    def _fields(self, r0):
        """The visibility rows (by="sight") or the fields of the sites r0 .. r0 + c - 1 into buf (c = the chunk's rows) -> c."""
        if self.kind != 0:
            return super()._fields(r0)
        c = min(self.chunk, self.m - r0)
        self.engine.visibility_field(self.site_ids[r0:r0 + c], self.buf, self.restrict_diagonal_near_obstacle, self.range_sq)
        self._held = r0
        return c

    def _compute(self):
        e = self.engine
        ms = self._gather(lambda c, r0: e.cover_pack(self.kind, c, self.n, self.buf, self.rows * self.cols, self.target_device,
                                                     0.0 if self.radius is None else self.radius, r0, self.mask_device))
        self._masks = None
        got = search(e, self.m, self.n, self.count, self.keep, self.mask_device, self.starts, self.rounds, self.seed, self.max_moves)
        self.row = np.asarray(got["row"], np.int32)
        self.sites = [int(v) for v in self.row if v >= 0]
        self.cells = [self.candidates[v] for v in self.sites]
        self.covered = got["count"]
        self.coverage = self.covered / self.n
        self.complete = self.covered == self.n
        self.mask = unpack_bits(got["covered"], self.n)
        self.history, self.moves, self.drops = got["history"], got["moves"], got["drops"]
        # the open rows only: seen_by and unique
        open_masks = np.array([self.mask_device.read(v * self.words, self.words) for v in self.sites], np.uint64).reshape(len(self.sites), self.words)   # ([0, W] with no open site)
        bits = unpack_bits(open_masks, self.n)
        self.seen_by = bits.sum(0).astype(np.int32)
        self.unique = [[int(j) for j in np.flatnonzero(bits[x] & (self.seen_by == 1))] for x in range(len(self.sites))]
        self.solve_kernel_ms = got["kernel_ms"]
        self.kernel_ms = ms + self.solve_kernel_ms

    @property
    def masks(self):
        """uint64 [candidates, ceil(n / 64)]: the packed masks, downloaded on the first use."""
        if self._masks is None:
            self._check_open()
            self._masks = self.mask_device.download().reshape(self.m, self.words)
        return self._masks

    def map(self):
        """bool [R, C]: True at the covered target cells."""
        out = np.zeros(self.rows * self.cols, bool)
        out[self.target_ids[self.mask]] = True
        return out.reshape(self.rows, self.cols)

    def coverage_of(self, sites):
        """How many targets any other set of candidates covers (indices into the constructor's sites, no index twice), on the host
        over `masks`: what another heuristic's choice is compared with; coverage_of(self.sites) == covered."""
        who = type(self).__name__
        try:
            seq = [self._index(f"sites[{x}]", v, self.m) for x, v in enumerate(sites)]
        except TypeError:
            raise ValueError(f"{who}: sites must be a sequence of indices into the candidate sites, got {sites!r}") from None
        if len(set(seq)) != len(seq):
            raise ValueError(f"{who}: sites names a site twice")
        if not seq:
            return 0
        return int(unpack_bits(np.bitwise_or.reduce(self.masks[seq], axis=0), self.n).sum())

    def exposure(self):
        """int32 [R, C]: Visibility.exposure of the open cells under this object's rule and range (by="sight"): how many open sites
        see each cell of the map, targets or not."""
        from .visibility import Visibility
        if self.kind != 0:
            raise ValueError(f"{type(self).__name__}: exposure() belongs to by='sight'")
        self._check_open()
        if not self.cells:
            return np.zeros((self.rows, self.cols), np.int32)
        v = Visibility(self.grid, self.restrict_diagonal_near_obstacle, engine=self.engine)
        try:
            return v.exposure(self.cells, self.max_range)
        finally:
            v.close()

    def field(self):
        """A NearestSourceField over the open cells on the same engine (by="reach" without a cost map): the path length of every
        cell to its nearest open site, and the owner map.  The caller closes it."""
        from .nearest_field import NearestSourceField
        who = type(self).__name__
        if self.kind != 1 or self.cost is not None:
            raise ValueError(f"{who}: field() belongs to by='reach' without a cost map")
        self._check_open()
        if not self.cells:
            raise PathfitError(f"{who}: no site is open")
        return NearestSourceField(self.grid, [list(self.cells)], True, self.restrict_diagonal_near_obstacle, engine=self.engine)

    @classmethod
    def solve_masks(cls, engine, masks, rows, n, fixed=0, shared=False, max_moves=None):
        """For callers with their own masks and starts: masks uint64 [B, m, W] -- or, with `shared`, one [m, W] for all starts -- with
        W = ceil(n / 64), element j bit j & 63 of word j >> 6 and no bit at j >= n (pack_bits builds them from bool [.., n]); rows int
        [B, p], the start rows (a site or -1 per slot, no site twice, the slots below `fixed` not empty: they are kept) ->
        Improved(row int32 [B, p], covered uint64 [B, W], value int64 [B, 4] = (covered after, open after, covered before, open
        before), status int32 [B]: 0 no better candidate is left, 2 stopped by max_moves (None: 16 p), info int64 [B, 4] = (moves,
        sweeps, elements covered exactly once, drops))."""
        who = cls.__name__
        a = np.asarray(masks)
        if a.dtype != np.uint64 or a.ndim not in (2, 3) or min(a.shape) < 1:
            raise ValueError(f"{who}: masks must be a uint64 array [B, m, W] with B, m, W >= 1")
        a = np.ascontiguousarray(a[None] if a.ndim == 2 else a)
        n = _int_in(who, "n", n, 1, ELEMS_MAX)
        m = int(a.shape[1])
        if a.shape[2] != words_of(n):
            raise ValueError(f"{who}: masks holds {a.shape[2]} words a row, n = {n} needs {words_of(n)}")
        one_if_shared(who, shared, a, "[m, W] mask set")
        o = start_rows(who, "rows", rows, a, shared, "p", per="mask set")
        p = _shape_check(who, m, n, int(o.shape[1]))
        fixed = _int_in(who, "fixed", fixed, 0, p)
        limit = move_limit(who, max_moves, p)
        if n % 64:
            bad = np.argwhere(a[:, :, -1] >> np.uint64(n % 64) != 0)
            if len(bad):
                raise ValueError(f"{who}: masks[{int(bad[0][0])}, {int(bad[0][1])}] holds a bit at an element >= n = {n}")
        slot_rows(who, o, m, fixed)
        dm = engine.put(a.reshape(-1), np.uint64)
        try:
            return _improve(engine, m, n, fixed, dm, bool(shared), o, limit)[0]
        finally:
            dm.free()
