"""The CPU model of the sight graph (include/pathfit.h: pf_sight_pack, pf_sight_field, pf_sight_paths), written from
the rule alone: the adjacency is tests/smooth_model.py's visible between the nodes' cells, the labels are a heap Dijkstra's over node
indices with the left-to-right fp64 sums, the parents and the routes follow the header's rules.  tests/test_sight_checkers.py pins
the heap against a random-order label-correcting sweep and against brute force over all simple walks."""
import functools
import heapq
import math

import numpy as np

import golden_io as gio
import smooth_model as sm
import visibility_checkers as vc

INF = float("inf")
NODES_MAX = 16384
MAPS = sm.MAPS20
# the issue's table: the maps' own start -> target under the strict rule (Dijkstra's route, PathSmoother's, the best, corners only)
TABLE = {
    "fig7": (31.556349186104, 29.659944540734, 28.885039798219, 29.469620086417),
    "img1": (32.142135623731, 30.275337360629, 29.403101907134, 29.994446574619),
    "img3": (42.242640687119, 41.886349517373, 38.042412109045, 39.841452831853),
}


def occ_of(g):
    return (np.asarray(g) == 1).astype(np.uint8)


# ---------------------------------------------------------------------------- the nodes
def free_nodes(g):
    return np.flatnonzero(np.asarray(g).reshape(-1) != 1).astype(np.int32)


def corner_nodes(g):
    """Free cells with a diagonal obstacle neighbour whose two shared orthogonal neighbours are free (the cell stands at a convex
    corner of the obstacle); cells outside the grid count as free."""
    occ = occ_of(g)
    R, C = occ.shape
    p = np.zeros((R + 2, C + 2), bool)
    p[1:-1, 1:-1] = occ == 1
    keep = np.zeros((R, C), bool)
    for dr in (-1, 1):
        for dc in (-1, 1):
            diag = p[1 + dr:R + 1 + dr, 1 + dc:C + 1 + dc]
            side_r = p[1 + dr:R + 1 + dr, 1:C + 1]
            side_c = p[1:R + 1, 1 + dc:C + 1 + dc]
            keep |= diag & ~side_r & ~side_c
    return np.flatnonzero((keep & (occ != 1)).reshape(-1)).astype(np.int32)


def node_ids(g, rule="free", also=()):
    """The node cells of a rule ("free", "corners" or a list of (r, c)) joined with the cells `also`, sorted by cell id."""
    C = np.asarray(g).shape[1]
    base = free_nodes(g) if rule == "free" else corner_nodes(g) if rule == "corners" else np.array([r * C + c for r, c in rule], np.int64)
    extra = np.array([r * C + c for r, c in also], np.int64)
    return np.unique(np.concatenate([np.asarray(base, np.int64), extra])).astype(np.int32)


# ---------------------------------------------------------------------------- the graph
def adjacency(occ, nodes, strict, max_range_sq=-1):
    """bool [M, M]: [i, j] iff visible(nodes[i], nodes[j], strict) within the range; the diagonal is "the cell is free".  Small
    maps ask smooth_model.all_pairs (the rule for every pair at once), large ones visibility_checkers.seen_map per node; both are
    pinned to smooth_model.visible by their own tests and, for these nodes, by tests/test_sight_checkers.py."""
    R, C = occ.shape
    nodes = np.asarray(nodes, np.int64)
    rr, cc = nodes // C, nodes % C
    if R * C <= 1024:
        adj = _all_pairs(occ.tobytes(), R, C, bool(strict))[np.ix_(nodes, nodes)].copy()
    else:
        adj = np.zeros((len(nodes), len(nodes)), bool)
        for i, a in enumerate(nodes):
            adj[i] = vc.seen_map(occ, (int(rr[i]), int(cc[i])), strict).reshape(-1)[nodes]
    if max_range_sq >= 0:
        adj &= ((rr[:, None] - rr[None, :]) ** 2 + (cc[:, None] - cc[None, :]) ** 2) <= max_range_sq
    return adj


@functools.lru_cache(maxsize=None)
def _all_pairs(occ_bytes, R, C, strict):
    return sm.all_pairs(np.frombuffer(occ_bytes, np.uint8).reshape(R, C), strict)[0]


def adjacency_by_definition(occ, nodes, strict, max_range_sq=-1):
    """The same from one smooth_model.visible per pair (slow: small node lists only)."""
    C = occ.shape[1]
    p = [(int(v) // C, int(v) % C) for v in nodes]
    adj = np.zeros((len(p), len(p)), bool)
    for i, a in enumerate(p):
        for j, b in enumerate(p):
            near = max_range_sq < 0 or (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 <= max_range_sq
            adj[i, j] = near and sm.visible(occ, a, b, strict)
    return adj


def pack_bits(adj, ld=None):
    """bool [M, M] -> uint64 [M, ld]: bit j & 63 of word j >> 6 of row i."""
    M = len(adj)
    W = (M + 63) // 64
    ld = W if ld is None else ld
    b = np.zeros((M, ld * 64), np.uint8)
    b[:, :adj.shape[1]] = adj
    return np.packbits(b, axis=1, bitorder="little").view("<u8").reshape(M, ld)


def unpack_bits(words, M):
    """uint64 [M, ld] -> bool [M, M] and the tail bits of the first ceil(M / 64) words as a bool array."""
    W = (M + 63) // 64
    bits = np.unpackbits(np.ascontiguousarray(words[:, :W]).view(np.uint8), axis=1, bitorder="little")
    return bits[:, :M] != 0, bits[:, M:] != 0


def pack_info(adj):
    """pf_sight_pack's info words."""
    off = adj & ~np.eye(len(adj), dtype=bool)
    deg = off.sum(axis=1)
    return [int(off.sum()), int(deg.max()), int(np.flatnonzero(deg == deg.max())[0]), int((~np.diag(adj)).sum())]


def weights(nodes, C):
    """float64 [M, M]: sqrt((double)(dr^2 + dc^2)), correctly rounded (numpy's sqrt is IEEE's)."""
    nodes = np.asarray(nodes, np.int64)
    rr, cc = nodes // C, nodes % C
    return np.sqrt(((rr[:, None] - rr[None, :]) ** 2 + (cc[:, None] - cc[None, :]) ** 2).astype(np.float64))


class RowWeights:
    """weights() without the matrix, for node lists of thousands: w[a, b] forms the entries asked for (indices broadcast as numpy's)."""

    def __init__(self, nodes, C):
        nodes = np.asarray(nodes, np.int64)
        self.rr, self.cc = nodes // C, nodes % C

    def __getitem__(self, ab):
        a, b = ab
        return np.sqrt(((self.rr[a] - self.rr[b]) ** 2 + (self.cc[a] - self.cc[b]) ** 2).astype(np.float64))


# ---------------------------------------------------------------------------- the labels
def usable(adj, sources):
    return sorted({int(s) for s in sources if adj[int(s), int(s)]})


def dijkstra(adj, w, sources):
    """Heap Dijkstra over node indices: float64 [M], +inf where no walk arrives.  An edge into v is read from row v.  The
    neighbours of a popped node are relaxed in one numpy step: the same fp64 additions, element by element."""
    M = len(adj)
    d = np.full(M, INF)
    heap = []
    for s in usable(adj, sources):
        d[s] = 0.0
        heap.append((0.0, s))
    heapq.heapify(heap)
    done = np.zeros(M, bool)
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du > d[u]:
            continue
        done[u] = True
        vs = np.flatnonzero(adj[:, u] & ~done)                        # the v whose row holds u
        cand = np.float64(du) + w[u, vs]
        low = cand < d[vs]
        d[vs[low]] = cand[low]
        for c, v in zip(cand[low].tolist(), vs[low].tolist()):
            heapq.heappush(heap, (c, v))
    return d


def dijkstra_complete(nodes, C, sources):
    """The same on the complete graph over `nodes` (an open map: every pair sees each other), the weights formed row by row so
    that 16 384 nodes need no matrix."""
    nodes = np.asarray(nodes, np.int64)
    rr, cc = nodes // C, nodes % C
    M = len(nodes)
    d = np.full(M, INF)
    heap = [(0.0, int(s)) for s in sorted(set(int(s) for s in sources))]
    for _, s in heap:
        d[s] = 0.0
    done = np.zeros(M, bool)
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du > d[u]:
            continue
        done[u] = True
        cand = np.float64(du) + np.sqrt(((rr - rr[u]) ** 2 + (cc - cc[u]) ** 2).astype(np.float64))
        low = (cand < d) & ~done
        d[low] = cand[low]
        for c, v in zip(cand[low].tolist(), np.flatnonzero(low).tolist()):
            heapq.heappush(heap, (c, v))
    return d


def sweep(adj, w, sources, seed):
    """Label correcting in a random node order, sweep after sweep, to the fixed point of d[v] = min_u fl(d[u] + w(u, v))."""
    M = len(adj)
    rnd = np.random.default_rng(seed)
    d = np.full(M, INF)
    d[usable(adj, sources)] = 0.0
    changed = True
    while changed:
        changed = False
        for v in rnd.permutation(M):
            us = np.flatnonzero(adj[v])
            if len(us):
                cand = (d[us] + w[us, v]).min()
                if cand < d[v]:
                    d[v] = cand
                    changed = True
    return d


def brute(adj, w, sources):
    """The definition: the least left-to-right sum over ALL simple walks from a usable source, one by one, nothing pruned (tiny
    graphs only).  A walk that repeats a node is never shorter: dropping the loop leaves a prefix sum that is no larger, and
    addition is monotone.  Python floats are IEEE doubles: the same additions as numpy's."""
    M = len(adj)
    d = [INF] * M
    nbr = [[int(u) for u in np.flatnonzero(adj[:, v]) if u != v] for v in range(M)]
    wl = [[float(x) for x in row] for row in w]

    def go(v, total, seen):
        if total < d[v]:
            d[v] = total
        for u in nbr[v]:
            if not (seen >> u) & 1:
                go(u, total + wl[v][u], seen | (1 << u))
    for s in usable(adj, sources):
        go(s, 0.0, 1 << s)
    return np.array(d, np.float64)


def sum_right_to_left(walk_w):
    total = np.float64(0.0)
    for x in reversed(walk_w):
        total = x + total
    return float(total)


def parents(adj, w, d, largest=False):
    """int32 [M]: -1 at label 0 and at +inf; else the smallest u with bit (v, u) set, d[u] < d[v] and fl(d[u] + w(u, v)) == d[v]
    (`largest`: the wrong rule that takes the largest such u, for the test that must reject it)."""
    M = len(adj)
    par = np.full(M, -1, np.int32)
    for v in range(M):
        if d[v] == 0.0 or d[v] == INF:
            continue
        us = np.flatnonzero(adj[v])
        ok = us[(d[us] < d[v]) & (d[us] + w[us, v] == d[v])]
        assert len(ok), ("a finite label without a parent", v)
        par[v] = ok[-1] if largest else ok[0]
    return par


def field_info(d):
    """pf_sight_field's info words for one row."""
    fin = np.flatnonzero(d < INF)
    if len(fin) == 0:
        return [0, 0, -1, 0]
    top = d[fin].max()
    return [len(fin), int((d == 0.0).sum()), int(fin[d[fin] == top][0]), 0]


def field(adj, w, set_off, src):
    """-> (dist float64 [B, M], parent int32 [B, M], info int64 [B, 4])"""
    B, M = len(set_off) - 1, len(adj)
    dist, par, info = np.full((B, M), INF), np.full((B, M), -1, np.int32), np.zeros((B, 4), np.int64)
    for b in range(B):
        dist[b] = dijkstra(adj, w, src[set_off[b]:set_off[b + 1]])
        par[b] = parents(adj, w, dist[b])
        info[b] = field_info(dist[b])
    return dist, par, info


# ---------------------------------------------------------------------------- the routes
def route(nodes, C, d, par, target, reverse=False, way_cap=None):
    """What pf_sight_paths leaves for one query -> (status, waypoint cells int32, length, turns)."""
    M = len(d)
    none = np.zeros(0, np.int32)
    if not 0 <= target < M:
        return 1, none, 0.0, 0
    if not d[target] < INF:
        return 2, none, 0.0, 0
    chain, v = [int(target)], int(target)
    while par[v] != -1:
        p = int(par[v])
        if not 0 <= p < M or len(chain) >= M:
            return 4, none, 0.0, 0
        chain.append(p)
        v = p
    if d[v] != 0.0:
        return 4, none, 0.0, 0
    if way_cap is not None and len(chain) > way_cap:
        return 3, none, 0.0, 0
    cells = np.asarray(nodes, np.int32)[chain[::-1]]
    length, turns = sm.stats(cells, C)
    return 0, (cells[::-1] if reverse else cells).copy(), length, turns


# ---------------------------------------------------------------------------- the issue's table
def grid_dijkstra(g, s, t):
    """The 8-connected shortest route s -> t under the strict corner rule, by a heap Dijkstra that breaks ties by cell id -> cells."""
    occ = occ_of(g)
    R, C = occ.shape
    d, par, heap = {s: 0.0}, {s: -1}, [(0.0, s)]
    done = set()
    while heap:
        du, u = heapq.heappop(heap)
        if u in done:
            continue
        done.add(u)
        if u == t:
            break
        r, c = divmod(u, C)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                rr, cc = r + dr, c + dc
                if (dr or dc) and 0 <= rr < R and 0 <= cc < C and occ[rr, cc] != 1:
                    if dr and dc and (occ[r, cc] == 1 or occ[rr, c] == 1):
                        continue
                    v, cand = rr * C + cc, du + (math.sqrt(2.0) if dr and dc else 1.0)
                    if v not in d or cand < d[v]:
                        d[v], par[v] = cand, u
                        heapq.heappush(heap, (cand, v))
    out, v = [], t
    while v != -1:
        out.append(v)
        v = par[v]
    return np.array(out[::-1], np.int32)


@functools.lru_cache(maxsize=None)
def graph_of(name, rule="free", strict=True):
    """(grid, nodes, adjacency, weights, start index, target index) of a golden map, the map's own start and target among the nodes."""
    g, s, t = gio.grid(name)
    C = g.shape[1]
    nodes = node_ids(g, rule, [divmod(s, C), divmod(t, C)])
    adj = adjacency(occ_of(g), nodes, strict)
    return g, nodes, adj, weights(nodes, C), int(np.searchsorted(nodes, s)), int(np.searchsorted(nodes, t))


@functools.lru_cache(maxsize=None)
def table_row(name):
    """(Dijkstra's route length, after forward string pulling, the best polyline through cell centres, corner cells only) for the
    map's own start -> target under the strict rule."""
    g, s, t = gio.grid(name)
    C = g.shape[1]
    occ = occ_of(g)
    cells = grid_dijkstra(g, s, t)
    way = cells[sm.smooth(occ, cells, True)]
    out = [sm.stats(cells, C)[0], sm.stats(way, C)[0]]
    for rule in ("free", "corners"):
        _, _, adj, w, si, ti = graph_of(name, rule)
        out.append(float(dijkstra(adj, w, [si])[ti]))
    return tuple(out)
