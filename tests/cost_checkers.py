"""CPU checkers for the cost fields (pf_cost_field / pf_cost_field_parents / pf_cost_paths, pathfit.CostField): the move weight, a
heap Dijkstra over source sets with the (g, cell id) pop order and strict-improvement came_from, the FIELD-ONLY parent rule in numpy,
a random-order sweep solver run to a fixed point, and the left-to-right cost of a path.  tests/test_cost_checkers.py pins them
against each other (and against field_checkers.reference_dijkstra at cost == 1) on any host; the GPU tests compare the device
against them.  Everything is plain IEEE double arithmetic: Python floats and numpy float64, one rounded operation at a time.

The rule: a legal move u -> v by move k weighs w = m (k < 4) or SQRT2 * m (k >= 4), m = 0.5 * (c[u] + c[v]); a label is
D[u] + w rounded once; parent(v) = the u with the smallest (D[u], u) among the cells with a legal move u -> v and D[u] + w == D[v]."""
import heapq

import numpy as np

import field_checkers as fc

INF = float("inf")
SQRT2 = fc.SQRT2
COST_MAX = float(2 ** 20)
SOURCE, NONE = fc.SOURCE, fc.NONE
POLICIES = fc.POLICIES
KINDS = ("ones", "int14", "u1", "u50", "u1e6")


def weight(c, u, v, k):
    """The weight of move k between flat cells u and v of the flat cost array c."""
    m = 0.5 * (float(c[u]) + float(c[v]))
    return m if k < 4 else SQRT2 * m


def cost_of_kind(kind, shape, seed):
    """The seeded cost maps of the tests: 1 everywhere; integers 1..4 (many ties); 1 + U * s for s = 1, 50, 10^6 (non-dyadic)."""
    rnd = np.random.default_rng(seed)
    if kind == "ones":
        return np.ones(shape, np.float64)
    if kind == "int14":
        return rnd.integers(1, 5, shape).astype(np.float64)
    s = {"u1": 1.0, "u50": 50.0, "u1e6": 1e6}[kind]
    return np.minimum(1.0 + rnd.random(shape) * s, COST_MAX)


def csr(sets):
    off = np.zeros(len(sets) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in sets])
    return off, np.array([v for s in sets for v in s], np.int32)


def dijkstra(grid, mm, cost, sources):
    """A heap Dijkstra seeded with every free cell of `sources` at 0: keys (g, cell id), a closed set, came_from overwritten on a
    strict improvement only -> (labels float64 [R, C], parent codes uint8 [R, C])."""
    R, C = mm.shape
    occ = np.asarray(grid).reshape(-1)
    c = np.asarray(cost, np.float64).reshape(-1).tolist()
    m = mm.reshape(-1).tolist()
    step = [fc.DR[k] * C + fc.DC[k] for k in range(8)]
    dist, code = [INF] * (R * C), [NONE] * (R * C)
    heap = []
    for s in sources:
        s = int(s)
        if occ[s] != 1 and dist[s] != 0.0:
            dist[s], code[s] = 0.0, SOURCE
            heap.append((0.0, s))
    heapq.heapify(heap)
    closed = set()
    while heap:
        g, u = heapq.heappop(heap)
        if u in closed:
            continue
        closed.add(u)
        mu, cu = m[u], c[u]
        for k in range(8):
            if (mu >> k) & 1:
                v = u + step[k]
                if v in closed:
                    continue
                h = 0.5 * (cu + c[v])
                t = g + (h if k < 4 else SQRT2 * h)
                if t < dist[v]:                                       # strict
                    dist[v], code[v] = t, k
                    heapq.heappush(heap, (t, v))
    return np.array(dist).reshape(R, C), np.array(code, np.uint8).reshape(R, C)


def fields(grid, cost, sets, ad, rs):
    """-> (D float64 [B, R, C], parents uint8 [B, R, C], info int64 [B, 4]) of the B source sets (flat ids) by the heap."""
    grid = np.asarray(grid)
    mm = fc.move_masks(grid, ad, rs)
    D, P, info = [], [], []
    for s in sets:
        d, p = dijkstra(grid, mm, cost, s)
        D.append(d)
        P.append(p)
        info.append(info_of(grid, d, s))
    return np.array(D), np.array(P), np.array(info, np.int64).reshape(len(sets), 4)


def info_of(grid, d, sources):
    """{sources that counted, cells with a finite label, the cell with the largest finite label (smallest id on a tie; -1), 0}."""
    occ = np.asarray(grid).reshape(-1)
    flat = d.reshape(-1)
    fin = np.isfinite(flat)
    n = int(fin.sum())
    far = int(np.argmax(np.where(fin, flat, -1.0))) if n else -1
    return [len({int(s) for s in sources if occ[int(s)] != 1}), n, far, 0]


def weights_into(cost, k):
    """w[r, c] = the weight of move k INTO (r, c) from (r, c) - step(k) (cost 1 beyond the grid: such a move is never legal)."""
    c = np.asarray(cost, np.float64)
    m = 0.5 * (fc.shifted(c, -fc.DR[k], -fc.DC[k], 1.0) + c)
    return m if k < 4 else SQRT2 * m


def rule_parents(field, mm, cost):
    """The field-only rule under the cost map (field_checkers.rule_parents with the move's weight formed from the two costs)."""
    R, C = field.shape
    ids = np.arange(R * C, dtype=np.int64).reshape(R, C)
    best_d = np.full((R, C), INF)
    best_u = np.full((R, C), -1, np.int64)
    code = np.full((R, C), NONE, np.uint8)
    finite = np.isfinite(field)
    for k in range(8):
        du = fc.shifted(field, -fc.DR[k], -fc.DC[k], INF)
        u = ids - (fc.DR[k] * C + fc.DC[k])
        with np.errstate(invalid="ignore"):
            ok = ((mm >> fc.OPP[k]) & 1 == 1) & finite & (du + weights_into(cost, k) == field)
        take = ok & ((du < best_d) | ((du == best_d) & ((best_u < 0) | (u < best_u))))
        best_d = np.where(take, du, best_d)
        best_u = np.where(take, u, best_u)
        code = np.where(take, np.uint8(k), code)
    code[field == 0.0] = SOURCE
    return code


def sweeps(grid, mm, cost, sources, seed, variant=None):
    """Relaxation sweeps over the cells in a fresh random order each, in place, until one whole sweep lowers nothing -> labels
    float64 [R, C].  Any order reaches the same least fixed point, bit for bit.  variant: a deliberately WRONG way of forming a
    label that the checker's own test must reject -- "split_diag": a diagonal summed as (D + m) + (SQRT2 - 1) * m, two roundings
    where the rule has one; "presum": a straight move taken two cells at a time, D[u2] + (w1 + w2), the weights summed first."""
    R, C = mm.shape
    occ = np.asarray(grid).reshape(-1)
    c = np.asarray(cost, np.float64).reshape(-1).tolist()
    m = mm.reshape(-1).tolist()
    step = [fc.DR[k] * C + fc.DC[k] for k in range(8)]
    D = [INF] * (R * C)
    for s in sources:
        if occ[int(s)] != 1:
            D[int(s)] = 0.0
    rnd = np.random.default_rng(seed)
    cells = [v for v in range(R * C) if occ[v] != 1]
    while True:
        changed = False
        for i in rnd.permutation(len(cells)):
            v = cells[i]
            best = D[v]
            for k in range(8):
                if not (m[v] >> fc.OPP[k]) & 1:
                    continue
                u = v - step[k]
                h = 0.5 * (c[u] + c[v])
                if variant == "split_diag" and k >= 4:
                    t = (D[u] + h) + (SQRT2 - 1.0) * h
                else:
                    t = D[u] + (h if k < 4 else SQRT2 * h)
                if t < best:
                    best = t
                if variant == "presum" and k < 4 and (m[u] >> fc.OPP[k]) & 1:
                    u2 = u - step[k]
                    t = D[u2] + (0.5 * (c[u2] + c[u]) + h)
                    if t < best:
                        best = t
            if best < D[v]:
                D[v] = best
                changed = True
        if not changed:
            return np.array(D).reshape(R, C)


def path_cost(cost, cells, C):
    """The left-to-right float64 sum of the weights along the flat cells (0.0 for one cell); every step must be a king move."""
    c = np.asarray(cost, np.float64).reshape(-1)
    total = 0.0
    for a, b in zip(cells[:-1], cells[1:]):
        dr, dc = int(b) // C - int(a) // C, int(b) % C - int(a) % C
        assert max(abs(dr), abs(dc)) == 1, (a, b)
        total = total + weight(c, int(a), int(b), 4 if dr and dc else 0)
    return total


def owners(code, sources):
    """owner[r, c] = the index within `sources` (the lowest for a cell listed twice) of the root of the cell's chain, -1 without one."""
    R, C = code.shape
    flat = code.reshape(-1)
    rank = {}
    for i, s in enumerate(sources):
        rank.setdefault(int(s), i)
    own = np.full(R * C, -1, np.int32)
    order = [v for v in range(R * C) if flat[v] != NONE]
    for v in order:
        chain, x = [], v
        while own[x] < 0 and flat[x] != SOURCE:
            chain.append(x)
            k = int(flat[x])
            x -= fc.DR[k] * C + fc.DC[k]
        o = own[x] if own[x] >= 0 else rank[x]
        own[x] = o
        for y in chain:
            own[y] = o
    return own.reshape(R, C)
