"""What the six planners share (Tour, Assignment, TourSearch, FleetTours, Placement, Coverage): Planner, the class
between Field and each of them, and the checks and the restart driver their searches and their solve_matrices / solve_masks use.

Planner owns the host side around the kernels: the device state (the cost map, the chunk of fields `buf`, the parent maps `pbuf`,
the chunk held), the fields of a chunk (`_fields`), the loop that computes every chunk and hands it to the planner's gather
(`_gather`), the route tracer (`_trace`), `refresh` and `_check_open`.  A planner keeps what is its own: its argument rules, its
matrix or masks, its search call, its key, its perturbation and what it reports."""
import numpy as np

from ._field import Field
from ._lib import PathfitError
from .cost_field import checked_cost
from .paths import CellPath

MOVES_MAX = 1 << 20
STARTS_MAX = 1 << 16
BIG = 2.0 ** 1000
SITES_MAX, OPEN_MAX = 1024, 64                                       # PF_PLACE_SITES_MAX, PF_PLACE_OPEN_MAX and PF_COVER_'s: the sites, the slots of a row


def chunk_rows(n_rows, cells, budget):
    """How many field rows of `cells` doubles are computed at once: as many as fit `budget` bytes, at least one, at most n_rows."""
    return int(max(1, min(int(n_rows), int(budget) // (8 * int(cells)))))


# ---- the checks of the constructors and of solve_matrices / solve_masks
def _int_in(who, name, v, lo, hi, none_ok=False):
    if v is None and none_ok:
        return None
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= int(v) <= hi:
        raise ValueError(f"{who}: {name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def move_limit(who, max_moves, items):
    """max_moves as an int in [0, 2^20]; None: 16 per item."""
    limit = _int_in(who, "max_moves", max_moves, 0, MOVES_MAX, none_ok=True)
    return 16 * items if limit is None else limit


def as_matrices(who, name, mats, x, y):
    """`mats` as float64 [B, x, y], one [x, y] as B = 1.  x == y: the matrices are square and B >= 1; else B, x, y >= 1."""
    try:
        a = np.ascontiguousarray(mats, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a [B, {x}, {y}] array of numbers") from None
    if a.ndim == 2:
        a = a[None]
    if x == y and (a.ndim != 3 or a.shape[1] != a.shape[2] or a.shape[0] < 1):
        raise ValueError(f"{who}: {name} has shape {a.shape}, not [B, {x}, {y}] with B >= 1")
    if x != y and (a.ndim != 3 or min(a.shape) < 1):
        raise ValueError(f"{who}: {name} has shape {a.shape}, not [B, {x}, {y}] with B, {x}, {y} >= 1")
    return a


def one_if_shared(who, shared, a, what):
    """The `shared` rule: one matrix (one mask set) for all starts."""
    if shared and a.shape[0] != 1:
        raise ValueError(f"{who}: shared=True takes one {what}, got {a.shape[0]}")


def no_bad_entry(who, name, a, bad, want):
    """The first entry of a [B, x, y] where the bool array `bad` is set, in index order, is reported."""
    at = np.argwhere(bad)
    if len(at):
        b, i, j = (int(v) for v in at[0])
        raise ValueError(f"{who}: {name}[{b}, {i}, {j}] = {float(a[b, i, j])!r} is {want}")


def start_rows(who, name, rows, a, shared, letter, width=None, per="matrix"):
    """The start rows as an integer array [B, width] (None: any width >= 1) with a row per matrix of `a`, any B >= 1 when shared."""
    try:
        o = np.array(rows)
        o = o[None] if o.ndim == 1 else o
        ok = o.ndim == 2 and o.shape[0] >= 1 and o.dtype.kind in "iu" and (o.shape[1] >= 1 if width is None else o.shape[1] == width)
    except (TypeError, ValueError):
        ok = False
    if not ok or (not shared and o.shape[0] != a.shape[0]):
        raise ValueError(f"{who}: {name} must be an integer array [B, {letter}] with a row per {per} (any B >= 1 with shared=True)")
    return o


def slot_count(who, m, n, p, noun, most, verb):
    """The shape rule of Placement and Coverage: m sites, n demands or targets (`noun`, at most `most` are `verb`), p slots -> p."""
    if m < 1:
        raise ValueError(f"{who}: sites is empty")
    if n < 1:
        raise ValueError(f"{who}: {noun} is empty")
    if m > SITES_MAX:
        raise ValueError(f"{who}: {m} sites; at most {SITES_MAX} are searched")
    if n > most:
        raise ValueError(f"{who}: {n} {noun}; at most {most} are {verb}")
    if not isinstance(p, (int, np.integer)) or isinstance(p, bool) or not 1 <= int(p) <= min(m, OPEN_MAX):
        raise ValueError(f"{who}: count must be an integer in [1, {min(m, OPEN_MAX)}] (at most the sites, at most {OPEN_MAX}), got {p!r}")
    return int(p)


def slot_rows(who, rows, m, fixed):
    """The slot-row rule of Placement and Coverage: a site or -1 per slot, no site twice, no empty slot below `fixed`."""
    for b, row in enumerate(rows):
        seen = set()
        for s, v in enumerate(row):
            v = int(v)
            if not -1 <= v < m or v in seen or (v < 0 and s < fixed):
                raise ValueError(f"{who}: rows[{b}, {s}] = {v}: a start holds sites of [0, {m}) or -1, no site twice, and no empty slot below fixed")
            if v >= 0:
                seen.add(v)


def slot_perturbed(row, fixed, draws):
    """A perturbed start: per draw (s, i) slot fixed + s takes site i if i is not in the row, else the draw is dropped."""
    out = [int(v) for v in row]
    for s, i in draws:
        if int(i) not in out:
            out[fixed + int(s)] = int(i)
    return out


def slot_perturbations(rng, row, fixed, m, starts):
    """`starts` perturbed starts of a row: one rng.integers(0, [p - f, m], (starts, Q, 2)) draw with Q = max(1, (p - f) // 4)."""
    p = len(row)
    draws = rng.integers(0, [p - fixed, m], (starts, max(1, (p - fixed) // 4), 2))
    return [slot_perturbed(row, fixed, draws[s]) for s in range(starts)]


# ---- one search call, and the rounds of restarts around it
def improve_call(e, result, rows, outs, call):
    """One search call over the start rows int32 [B, w]: the rows go up, the outputs `outs` ((shape, dtype) each) are allocated,
    call(d_rows, *d_outs) runs, everything comes down -> (result(rows, *outputs), kernel ms)."""
    rows = np.ascontiguousarray(rows, np.int32)
    bufs = [e.put(rows.reshape(-1), np.int32)] + [e.buf(shape, dt) for shape, dt in outs]
    try:
        call(*bufs)
        ms = e.last_kernel_ms()
        return result(bufs[0].download().reshape(rows.shape).astype(np.int32), *(b.download().reshape(s) for b, (s, _) in zip(bufs[1:], outs))), ms
    finally:
        for b in bufs:
            b.free()


def restarts(first, rounds, seed, perturb, improve, key):
    """The rounds behind round 0, whose one start `first` holds (an Improved: the rows come first, info[:, 0] are the moves): per
    round perturb(rng, the incumbent's row) -> the start rows, improve(rows) -> (Improved, ms) in one call, and the first smallest
    key(improved, x) replaces the incumbent iff it is strictly smaller.  One np.random.default_rng(seed) per search ->
    (the Improved that holds the incumbent, its index there, the incumbent's key after round 0, 1, ..., the moves, the rounds' ms)."""
    got, at, best = first, 0, key(first, 0)
    history, moves, ms = [best], int(first.info[0, 0]), 0.0
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        new, t = improve(perturb(rng, got[0][at]))
        ms += t
        moves += int(new.info[:, 0].sum())
        keys = [key(new, x) for x in range(len(new.status))]
        x = keys.index(min(keys))                                     # (the first smallest)
        if keys[x] < best:
            best, got, at = keys[x], new, x
        history.append(best)
    return got, at, history, moves, ms


class Planner(Field):
    """A class sets _closed and _built, the two phrases of its messages, and calls in its constructor, in this order:
    _set_cost_and_moves, _set_search (the four searches), then -- every argument checked -- _open, which touches the device."""
    _bufs = ("buf", "pbuf", "mbuf", "cost_device")
    CHUNK_BYTES = 256 << 20
    _closed = "the planner is closed"
    _built = "a planner"
    pbuf = None
    allow_diagonal_moves = True

    def _set_cost_and_moves(self, cost, allow_diagonal_moves, restrict_diagonal_near_obstacle):
        self.cost = None if cost is None else checked_cost(type(self).__name__, self.grid, cost)
        self.allow_diagonal_moves = bool(allow_diagonal_moves)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)

    def _set_search(self, starts, rounds, seed, max_moves, items):
        who = type(self).__name__
        self.starts = _int_in(who, "starts", starts, 1, STARTS_MAX)
        self.rounds = _int_in(who, "rounds", rounds, 0, 1 << 20)
        self.seed = _int_in(who, "seed", seed, 0, (1 << 63) - 1)
        self.max_moves = move_limit(who, max_moves, items)

    def _open(self, engine, new_engine, sources, chunk=None, dtype=np.float64):
        """The last check, then the device: the engine, the cost map and the buffer of `chunk` rows for the fields of `sources`
        (None: as many rows as fit CHUNK_BYTES)."""
        self._src = sources
        self.chunk = chunk_rows(len(sources), self.rows * self.cols, self.CHUNK_BYTES) if chunk is None else chunk
        self._set_engine(engine, new_engine)
        e = self.engine
        self.cost_device = None if self.cost is None else e.put(self.cost.reshape(-1), np.float64)
        self.buf = e.buf((self.chunk, self.rows, self.cols), dtype)
        return e

    def _check_open(self):
        if self.buf is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: {self._closed}")

    def _fields(self, r0):
        """The fields of the sources r0 .. r0 + k - 1 into buf (k = the chunk's rows) -> k."""
        e, k = self.engine, min(self.chunk, len(self._src) - r0)
        ids = self._src[r0:r0 + k]
        if self.cost_device is None:
            e.dist_field_batch(ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        else:
            e.cost_field(self.cost_device, np.arange(k + 1, dtype=np.int32), ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle)
        self._held = r0
        return k

    def _gather(self, take):
        """Every chunk's fields, each handed to take(k, r0), the planner's gather of the chunk's k rows from row r0 on -> kernel ms."""
        e, ms = self.engine, 0.0
        for r0 in range(0, len(self._src), self.chunk):
            k = self._fields(r0)
            ms += e.last_kernel_ms()
            take(k, r0)
            ms += e.last_kernel_ms()
        return ms

    def _drop_parents(self):
        if self.pbuf is not None:
            self.pbuf.free()
            self.pbuf = None

    def _trace(self, queries, noun):
        """queries: (source row, target cell id) pairs -> their CellPaths in query order, each DistanceField.paths' route from the
        source to the target cell for cell.  The queries are grouped by the chunk of fields their source lies in, the chunk held
        first (it is not computed again): a parent-map call per chunk and one trace call with a field index per query.  A chunk
        of fields that was released for a later one is computed again."""
        e, full, n = self.engine, self.rows * self.cols, len(self._src)
        ad, rs = self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle
        out = [None] * len(queries)
        for r0 in sorted(range(0, n, self.chunk), key=lambda r: r != self._held):
            mine = [x for x, (s, _) in enumerate(queries) if r0 <= s < r0 + self.chunk]
            if not mine:
                continue
            k = min(self.chunk, n - r0)
            if self._held != r0:
                self._fields(r0)
                self._drop_parents()
            if self.pbuf is None:
                pbuf = e.buf((self.chunk, self.rows, self.cols), np.uint8)
                try:
                    if self.cost_device is None:
                        e.dist_field_parents(k, self.buf, pbuf, ad, rs)
                    else:
                        e.cost_field_parents(self.cost_device, k, self.buf, pbuf, ad, rs)
                except Exception:
                    pbuf.free()
                    raise
                self.pbuf = pbuf
            q = len(mine)
            dk = e.put(np.array([queries[x][0] - r0 for x in mine], np.int32))
            dt = e.put(np.array([queries[x][1] for x in mine], np.int32))
            dl, dst = e.buf(q, np.int32), e.buf(q, np.int32)
            dcl, cap = None, e.default_path_cap()
            try:
                while True:
                    dcl = e.buf((q, cap), np.int32)
                    e.dist_field_paths(k, self.pbuf, dt, q, cap, dcl, dl, dst, dk, self.buf, False, None)
                    st = dst.download()
                    if cap >= full or not (st == 3).any():
                        break
                    dcl.free()
                    dcl, cap = None, full
                if (st == 3).any():
                    raise PathfitError(f"{type(self).__name__}: {int((st == 3).sum())} {noun} hold more than {cap} cells")
                lens, cells = dl.download(), dcl.download().reshape(q, cap)
                for y, x in enumerate(mine):
                    out[x] = CellPath(cells[y, :lens[y]].copy(), self.cols)
            finally:
                for b in (dk, dt, dl, dst, dcl):
                    if b is not None:
                        b.free()
        return out

    def refresh(self, cost=None):
        """Compute the result again on the map the engine holds now (after engine.update_grid) and, when given, under a new cost map
        (for an object built with one)."""
        who = type(self).__name__
        self._check_open()
        if cost is not None and self.cost is None:
            raise ValueError(f"{who}: refresh(cost) needs {self._built} built with a cost map")
        held = getattr(self.engine, "grid_u8", None)
        grid = np.array(held, dtype=int) if held is not None else self.grid
        if self.cost is not None:
            new = checked_cost(who, grid, self.cost if cost is None else cost)
            if cost is not None:
                self.cost = new
                self.cost_device.upload(new.reshape(-1))
        self.grid = grid
        self._drop_parents()
        self._compute()
        return self

    def _set_keep(self, keep):
        """`keep` of Placement and Coverage: indices into the m sites, none twice, at most `count`."""
        who = type(self).__name__
        try:
            keep = list(keep)
        except TypeError:
            raise ValueError(f"{who}: keep must be a list of indices into sites, got {keep!r}") from None
        self.keep = [self._index(f"keep[{x}]", v, self.m) for x, v in enumerate(keep)]
        if len(set(self.keep)) != len(self.keep):
            raise ValueError(f"{who}: keep names a site twice")
        if len(self.keep) > self.count:
            raise ValueError(f"{who}: keep holds {len(self.keep)} sites, more than count = {self.count}")
