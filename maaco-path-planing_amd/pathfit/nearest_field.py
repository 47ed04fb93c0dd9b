"""NearestSourceField: the nearest-exit / nearest-charger / task-allocation map.  ONE field per source SET (pf_dist_field_merged):
the exact length from every cell to the nearest source of the set, the source that owns each cell (pf_dist_field_owners), the size
of each source's territory and the route from the owning source to each of many targets -- in 8 R C bytes of labels and 4 R C
bytes of owners per set whatever the number of sources, where a DistanceField needs a row and a parent map per source."""
import numpy as np

from ._batch import _cells
from .dist_field import DistanceField
from .engine import Engine


def _is_pair(p):
    try:
        a, b = p
    except (TypeError, ValueError):
        return False
    return np.ndim(a) == 0 and np.ndim(b) == 0


class NearestSourceField(DistanceField):
    """fields[b, r, c] = the length of the shortest path into (r, c) from the nearest source of source_sets[b] under the move policy
    (inf: an obstacle, or out of reach of the whole set): bit for bit the elementwise minimum of DistanceField's rows for the set.
    source_sets: a list of B lists of (r, c) pairs; one flat list of pairs means B = 1.  A cell listed twice counts once, under its
    lowest index.

    owners[b, r, c] = the index within source_sets[b] of the source that owns the cell, -1 where no route ends.  Ties: the owner is
    the root of the tree a dijkstra.py-shaped search seeded with the whole set leaves -- the parent of a cell is the neighbour u with
    the smallest (D[u], u) that offers the cell's label, at every step.  It is NOT the lowest source index among the sources at the
    same distance; DistanceField.paths(k=None) keeps its own lowest-k rule.  The two agree on every length, not on every cell."""
    _bufs = ("obuf", "cbuf", "ibuf") + DistanceField._bufs
    _info_bounds_chains = True              # info[b, 0] (the levels) bounds the cells of a parent chain: the owner kernel's rounds

    def __init__(self, grid, source_sets, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        self._set_grid(grid)
        self._set_source_sets(source_sets, allow_diagonal_moves, restrict_diagonal_near_obstacle)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        self._start()

    def _set_source_sets(self, source_sets, allow_diagonal_moves, restrict_diagonal_near_obstacle):
        """The sets and the policy, checked on the host."""
        who = type(self).__name__
        try:
            sets = list(source_sets)
        except TypeError:
            raise ValueError(f"{who}: source_sets must be a list of lists of (r, c) pairs, got {source_sets!r}") from None
        if not sets:
            raise ValueError(f"{who}: source_sets is empty")
        if _is_pair(sets[0]):
            sets = [sets]
        self.source_sets = []
        for b, pts in enumerate(sets):
            try:
                pts = list(pts)
            except TypeError:
                raise ValueError(f"{who}: source_sets[{b}] must be a list of (r, c) pairs, got {pts!r}") from None
            if not pts:
                raise ValueError(f"{who}: source_sets[{b}] is empty")
            self.source_sets.append(_cells(who, f"source_sets[{b}]", pts, len(pts), self.grid))
        self.B = self.K = len(self.source_sets)                       # (K: the inherited calls see B fields)
        self.allow_diagonal_moves = bool(allow_diagonal_moves)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self.set_off = np.concatenate([[0], np.cumsum([len(s) for s in self.source_sets])]).astype(np.int32)
        self.ids = np.array([r * self.cols + c for s in self.source_sets for r, c in s], np.int32)

    def _start(self):
        """The buffers and the field rows, once the engine is set."""
        self._fields = self._parents = self._owners = self._counts = self._info = None
        self.pbuf = self.obuf = self.cbuf = self.ibuf = None
        self.chosen = np.zeros(0, np.int32)
        self.buf = self.engine.buf((self.B, self.rows, self.cols), np.float64)
        self.ibuf = self.engine.buf((self.B, 4), np.int64)
        self._compute_fields()
        self.kernel_ms = self.engine.last_kernel_ms()

    def _compute_fields(self):
        """The field rows into `buf`, their info block into `ibuf` (CostField computes them under its cost map)."""
        self.engine.dist_field_merged(self.set_off, self.ids, self.buf, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle, self.ibuf)

    def _k_checked(self, b):
        return self._index("b", b, self.B)

    @property
    def info(self):
        """int64 [B, 4]: levels that held a live cell, cells reached, relaxations offered, list appends of each set's field."""
        if self._info is None:
            self._check_open()
            self._info = self.ibuf.download()
        return self._info

    def _owner_buf(self):
        """The owner maps in HBM (int32 [B, R, C]) and the territory sizes, computed on first use."""
        pbuf = self._parent_buf()
        if self.obuf is None:
            e = self.engine
            obuf, cbuf = e.buf((self.B, self.rows, self.cols), np.int32), e.buf(len(self.ids), np.int64)
            try:
                e.dist_field_owners(self.set_off, self.ids, pbuf, obuf, self.ibuf if self._info_bounds_chains else None, cbuf)
            except Exception:
                obuf.free()
                cbuf.free()
                raise
            self.obuf, self.cbuf = obuf, cbuf
            self.owners_kernel_ms = e.last_kernel_ms()
        return self.obuf

    @property
    def owners(self):
        """int32 [B, R, C], computed and downloaded on first use: the index within its set of the source that owns the cell (the
        root of the cell's chain through `parents`), -1 where no route ends."""
        if self._owners is None:
            self._owners = self._owner_buf().download()
        return self._owners

    def territory_sizes(self, b):
        """int64 per source of set b: the cells it owns, itself included (0 for a second listing of a cell)."""
        b = self._k_checked(b)
        if self._counts is None:
            self._owner_buf()
            self._counts = self.cbuf.download()
        return self._counts[self.set_off[b]:self.set_off[b + 1]].copy()

    def nearest(self, b, cell):
        """(the index within set b of the source that owns `cell`, the path length from it), or (None, inf) where no route ends."""
        b = self._k_checked(b)
        at = b * self.rows * self.cols + int(self._target_ids([cell])[0])
        if self._owners is not None:
            own = int(self._owners.reshape(-1)[at])
        else:
            own = int(self._owner_buf().read(at, 1)[0])
        if own < 0:
            return None, float("inf")
        return own, float(self._fields.reshape(-1)[at] if self._fields is not None else self.buf.read(at, 1)[0])

    def paths(self, targets, b=0, reverse=False, path_cap=None):
        """The route from the source of set b that owns each of `targets` ((r, c) pairs) to that target -> a list of CellPath, empty
        where no route ends: the path a dijkstra.py-shaped search seeded with the whole set leaves, cell for cell; `chosen` holds
        the owners (-1: no route).  reverse and path_cap as DistanceField.paths."""
        ids = self._target_ids(targets)
        b = self._k_checked(b)
        if path_cap is not None and int(path_cap) < 1:
            raise ValueError(f"{type(self).__name__}: path_cap must be >= 1")
        out = self._paths_of(ids, np.full(len(ids), b, np.int32), reverse, path_cap)
        self.chosen = self.owners[b].reshape(-1)[ids] if len(ids) else np.zeros(0, np.int32)
        return out
