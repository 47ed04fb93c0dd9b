"""AnyAngle: exact any-angle shortest paths between cell centres (pf_sight_pack, pf_sight_field, pf_sight_paths) -- the yardstick for
Euclidean length that PathSmoother's forward pass is measured against.  A route is a polyline whose vertices are cell centres and
whose segments all pass PathSmoother.visible; its length is the left-to-right float64 sum of the segments' Euclidean lengths.  The
class builds the sight graph over a node list on the device (a bit per ordered pair of nodes) and labels it from source sets: with
nodes="free" every free cell is a node and the labels are the optimum over all such polylines, bit for bit a heap Dijkstra's.
nodes="corners" keeps only the cells at convex obstacle corners (plus `also`): a roadmap for maps with more than 16 384 free cells.
Under this sight rule the optimum bends at cells that touch no corner, so "corners" results are UPPER BOUNDS: never below what
"free" gives for the same pair, and above it on most maps with obstacles.  The occupancy is the engine's at call
time: `refresh` follows Engine.update_grid."""
import math
from fractions import Fraction

import numpy as np

from ._field import Field
from ._lib import PathfitError
from .engine import Engine
from .paths import CellPath

NODES_MAX = 16384
RANGE_SQ_MAX = 2 ** 31 - 2


def free_cells(grid):
    """int32 ids of the free cells, ascending."""
    return np.flatnonzero(np.asarray(grid).reshape(-1) != 1).astype(np.int32)


def corner_cells(grid):
    """int32 ids, ascending: the free cells with a diagonal obstacle neighbour whose two shared orthogonal neighbours are free
    (cells outside the grid count as free): where a taut route can bend round an obstacle's convex corner."""
    ob = np.asarray(grid) == 1
    R, C = ob.shape
    p = np.zeros((R + 2, C + 2), bool)
    p[1:-1, 1:-1] = ob
    keep = np.zeros((R, C), bool)
    for dr in (-1, 1):
        for dc in (-1, 1):
            keep |= p[1 + dr:R + 1 + dr, 1 + dc:C + 1 + dc] & ~p[1 + dr:R + 1 + dr, 1:C + 1] & ~p[1:R + 1, 1 + dc:C + 1 + dc]
    return np.flatnonzero((keep & ~ob).reshape(-1)).astype(np.int32)


class AnyAngle(Field):
    """nodes: "free", "corners" or a list of (r, c); `also` adds cells (starts, goals); the union is sorted by cell id and must hold
    1 .. 16 384 cells.  restrict_diagonal_near_obstacle: PathSmoother's strict rule (a segment that touches an obstacle's corner is
    blocked); max_range: sight edges no longer than this many cells (None: no limit).  A node on an obstacle is kept and isolated.

    node_cells int32 [M]; graph_info int64 [4] = (set off-diagonal bits, the largest degree, the node index that holds it, nodes on
    obstacles); info int64 [B, 4] of the last field = (finite labels, usable sources, the node index with the largest finite label or
    -1, 0); work = (the most rounds of a set, rounds, candidate sums, labels lowered); kernel_ms the last call's kernel time."""
    _bufs = ("adj_device", "dist_device", "parent_device")

    def __init__(self, grid, nodes="free", also=(), restrict_diagonal_near_obstacle=True, max_range=None, engine=None):
        self._set_grid(grid)
        if self.rows * self.rows + self.cols * self.cols >= 2 ** 31 - 1:
            raise ValueError("AnyAngle: R^2 + C^2 must stay below 2^31 - 1")
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self.max_range_sq = self._range_sq(max_range)
        if isinstance(nodes, str):
            if nodes not in ("free", "corners"):
                raise ValueError(f"AnyAngle: nodes must be \"free\", \"corners\" or a list of (r, c) pairs, got {nodes!r}")
            base = free_cells(self.grid) if nodes == "free" else corner_cells(self.grid)
        else:
            base = self._cell_ids("nodes", nodes)
        if isinstance(also, (str, bytes)):
            raise ValueError(f"AnyAngle: also must be a list of (r, c) pairs, got {also!r}")
        self.node_cells = np.unique(np.concatenate([base.astype(np.int64), self._cell_ids("also", also).astype(np.int64)])).astype(np.int32)
        self.M = int(self.node_cells.size)
        if not 1 <= self.M <= NODES_MAX:
            raise ValueError(f"AnyAngle: the node list holds {self.M} cells, 1 .. {NODES_MAX} are supported" +
                             (" (nodes=\"corners\" is the roadmap for larger maps)" if self.M > NODES_MAX and nodes == "free" else ""))
        self.ld = (self.M + 63) // 64
        self._index_of = np.full(self.rows * self.cols, -1, np.int32)
        self._index_of[self.node_cells] = np.arange(self.M, dtype=np.int32)
        self.adj_device = self.dist_device = self.parent_device = None
        self.graph_info = self.info = self.dist = None
        self.set_off = self.src = None
        self.B, self.work, self.kernel_ms = 0, (0, 0, 0, 0), 0.0
        self.lengths, self.turns, self.status = np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int32)
        self._closed = False
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        self._pack()

    # ------------------------------------------------------------------ arguments
    @staticmethod
    def _range_sq(max_range):
        if max_range is None:
            return -1
        try:
            m = float(max_range)
        except (TypeError, ValueError):
            m = math.nan
        if isinstance(max_range, bool) or not (0.0 <= m < math.inf):
            raise ValueError(f"AnyAngle: max_range must be None or a finite number >= 0, got {max_range!r}")
        f = Fraction(max_range) if isinstance(max_range, (int, Fraction)) else Fraction(m)
        return min(int(f * f // 1), RANGE_SQ_MAX)

    def _check_open(self):
        if getattr(self, "_closed", True) or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the field is closed")

    def _node(self, what, p):
        """(r, c) -> its node index; a cell that is no node is an error."""
        i = int(self._index_of[self._cell(what, p)])
        if i < 0:
            raise ValueError(f"AnyAngle: {what} = {tuple(int(v) for v in p)} is not among the nodes (add it with also=)")
        return i

    def _source_sets(self, sources):
        """A list of sets, each one (r, c) pair or a list of them -> (set_off int32 [B + 1], src int32 node indices)."""
        if isinstance(sources, (str, bytes)):
            raise ValueError(f"AnyAngle: sources must be a list of (r, c) pairs or of lists of them, got {sources!r}")
        try:
            sources = list(sources)
        except TypeError:
            raise ValueError(f"AnyAngle: sources must be a list of (r, c) pairs or of lists of them, got {sources!r}") from None
        if len(sources) == 0:
            raise ValueError("AnyAngle: sources is empty")
        off, src = [0], []
        for b, s in enumerate(sources):
            one = False
            try:
                one = len(s) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in s)
            except TypeError:
                raise ValueError(f"AnyAngle: sources[{b}] must be an (r, c) pair or a list of them, got {s!r}") from None
            if one:
                src.append(self._node(f"sources[{b}]", s))
            else:
                if isinstance(s, (str, bytes)):
                    raise ValueError(f"AnyAngle: sources[{b}] must be an (r, c) pair or a list of them, got {s!r}")
                src += [self._node(f"sources[{b}][{j}]", p) for j, p in enumerate(s)]
            off.append(len(src))
        return np.array(off, np.int32), np.array(src, np.int32).reshape(-1)

    # ------------------------------------------------------------------ the graph
    def _pack(self):
        e = self.engine
        if self.adj_device is None:
            self.adj_device = e.buf((self.M, self.ld), np.uint64)
        di = e.buf(4, np.int64)
        try:
            e.sight_pack(self.node_cells, self.adj_device, self.ld, self.restrict_diagonal_near_obstacle, self.max_range_sq, di)
            self.kernel_ms = self.pack_kernel_ms = e.last_kernel_ms()
            self.graph_info = di.download()
        finally:
            di.free()

    def adjacency(self):
        """bool [M, M]: [i, j] is True where node i sees node j; the diagonal says the node's cell is free."""
        self._check_open()
        words = self.adj_device.download().reshape(self.M, self.ld)
        return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :self.M] != 0

    def degree(self):
        """int64 [M]: how many other nodes each node sees."""
        a = self.adjacency()
        return a.sum(axis=1).astype(np.int64) - np.diag(a)

    # ------------------------------------------------------------------ the labels
    def field(self, sources):
        """sources: a list of B source sets, each an (r, c) pair or a list of them (node cells) -> dist float64 [B, M] over the
        nodes (`node_cells`): the length of the shortest any-angle route from the set's nearest usable source, 0 at a source, inf
        where none arrives (a node on an obstacle, a sealed room, a set of obstacle cells only).  The labels and their parents stay
        in HBM for paths / map / gap."""
        off, src = self._source_sets(sources)
        self._check_open()
        return self._field(off, src)

    def _field(self, off, src):
        e, B = self.engine, len(off) - 1
        if B != self.B or self.dist_device is None:
            for name in ("dist_device", "parent_device"):
                buf = getattr(self, name)
                setattr(self, name, None)
                if buf is not None:
                    buf.free()
            self.dist_device, self.parent_device = e.buf((B, self.M), np.float64), e.buf((B, self.M), np.int32)
        self.B, self.set_off, self.src = B, off, src
        di = e.buf((B, 4), np.int64)
        try:
            e.sight_field(self.node_cells, self.adj_device, self.ld, off, src, self.dist_device, self.parent_device, di)
            self.kernel_ms = self.field_kernel_ms = e.last_kernel_ms()
            self.work = e.sight_field_work()
            self.info = di.download().reshape(B, 4)
        finally:
            di.free()
        self.dist = self.dist_device.download().reshape(B, self.M)
        return self.dist

    def _need_field(self, what):
        if self.dist is None:
            raise ValueError(f"AnyAngle: {what} needs a field() call before it")

    def map(self, b=0):
        """float64 [R, C]: set b's labels laid out on the grid, inf off the nodes."""
        self._need_field("map")
        b = self._index("b", b, self.B)
        out = np.full(self.rows * self.cols, np.inf)
        out[self.node_cells] = self.dist[b]
        return out.reshape(self.rows, self.cols)

    def _sets_of(self, k, n):
        if k is None:
            return np.zeros(n, np.int32)
        if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
            return np.full(n, self._index("k", k, self.B), np.int32)
        try:
            k = list(k)
        except TypeError:
            raise ValueError(f"AnyAngle: k must be None, a set index or one per target, got {k!r}") from None
        if len(k) != n:
            raise ValueError(f"AnyAngle: k holds {len(k)} set indices for {n} targets")
        return np.array([self._index(f"k[{i}]", v, self.B) for i, v in enumerate(k)], np.int32).reshape(n)

    def _targets(self, targets):
        if isinstance(targets, (str, bytes)):
            raise ValueError(f"AnyAngle: targets must be a list of (r, c) pairs, got {targets!r}")
        try:
            targets = list(targets)
        except TypeError:
            raise ValueError(f"AnyAngle: targets must be a list of (r, c) pairs, got {targets!r}") from None
        return np.array([self._node(f"targets[{i}]", p) for i, p in enumerate(targets)], np.int32).reshape(len(targets))

    def paths(self, targets, k=None, reverse=False):
        """targets: (r, c) node cells; k: the set each is routed from (None: set 0; an index; or one per target) -> a list of CellPath
        of WAYPOINTS, source -> target (target -> source when reverse): consecutive waypoints see each other and the polyline is
        the optimum.  `lengths` (equal to the label, bit for bit), `turns` and `status` (0 ok, 2 out of reach: an empty CellPath)
        describe the call."""
        self._need_field("paths")
        tg = self._targets(targets)
        ks = self._sets_of(k, len(tg))
        n = len(tg)
        if n == 0:
            self.lengths, self.turns, self.status = np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int32)
            return []
        self._check_open()
        e, cap = self.engine, self.M
        bufs = [e.put(ks), e.put(tg), e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf((n, 2), np.float64), e.buf(n, np.int32)]
        try:
            e.sight_paths(self.node_cells, self.B, self.dist_device, self.parent_device, n, bufs[1], cap, bufs[2], bufs[3], bufs[5], bufs[0], bufs[4], reverse)
            self.kernel_ms = e.last_kernel_ms()
            way, wl, stats, self.status = bufs[2].download().reshape(n, cap), bufs[3].download(), bufs[4].download().reshape(n, 2), bufs[5].download()
        finally:
            for b in bufs:
                b.free()
        if ((self.status != 0) & (self.status != 2)).any():
            raise PathfitError(f"AnyAngle: internal: a route ended with status {int(self.status[(self.status != 0) & (self.status != 2)][0])}")
        self.lengths, self.turns = stats[:, 0].copy(), stats[:, 1].astype(np.int64)
        self.lengths[self.status == 2] = np.inf
        return [CellPath(way[i, :wl[i]].copy(), self.cols) for i in range(n)]

    def route(self, a, b):
        """The shortest any-angle route a -> b (both node cells) -> its CellPath of waypoints, empty when b is out of reach;
        `lengths[0]` is its length."""
        ia, ib = self._node("a", a), self._node("b", b)
        self._check_open()
        self._field(np.array([0, 1], np.int32), np.array([ia], np.int32))
        return self.paths([tuple(int(v) for v in divmod(int(self.node_cells[ib]), self.cols))])[0]

    def gap(self, lengths, targets, k=0):
        """How far other routes to `targets` are from the optimum: lengths / dist - 1 (float64 [n]) for their Euclidean lengths, for
        example PathSmoother.lengths of routes from set k's source; 0 is optimal, inf / inf and 0 / 0 give nan."""
        self._need_field("gap")
        tg = self._targets(targets)
        ks = self._sets_of(k, len(tg))
        try:
            ln = np.array(lengths, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"AnyAngle: lengths must be numbers, got {lengths!r}") from None
        if len(ln) != len(tg):
            raise ValueError(f"AnyAngle: {len(ln)} lengths for {len(tg)} targets")
        with np.errstate(divide="ignore", invalid="ignore"):
            return ln / self.dist[ks, tg] - 1.0

    def refresh(self):
        """After engine.update_grid: pack the graph again on the map the engine holds now and recompute the last field (same
        source sets); the node list stays as it was built."""
        self._check_open()
        held = getattr(self.engine, "grid_u8", None)
        if held is not None:
            self.grid = np.array(held, dtype=int)
        self._pack()
        if self.set_off is not None:
            self._field(self.set_off, self.src)
        return self

    def close(self):
        self._closed = True
        super().close()
