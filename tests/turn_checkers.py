"""CPU checkers for the turn fields (pf_turn_field / pf_turn_field_paths / pf_turn_paths, pathfit.TurnField): a heap Dijkstra over
(cell, heading) states in the rule's literal form, the same search in the kernel's form (one straight offer per state, eight turned
offers per cell), random-order sweeps run to a fixed point, the field-only route rule, the left-to-right cost of a path with its turn
count, and the minimum over all simple paths of a small grid.  tests/test_turn_checkers.py pins them against each other (and against
cost_checkers.dijkstra at turn weight 0) on any host; the GPU tests compare the device against them.  Plain IEEE double arithmetic:
Python floats, one rounded operation at a time.

The rule: a legal move u -> v by move k weighs w as cost_checkers.weight; T[d][s] = 0 for all eight d on a free source;
T[d][v] = min over d' of T[d'][u] + e, u = v - step(d), e = w for d' == d and (w + wt) -- rounded first -- otherwise; best = min over d."""
import heapq

import numpy as np

import cost_checkers as ck
import field_checkers as fc

INF = float("inf")
SQRT2 = fc.SQRT2
POLICIES = fc.POLICIES
KINDS = ("ones", "int14", "u50", "u1e6")
WEIGHTS = (0.0, 0.1, 0.3, 3.0, float(2 ** 20))
TW, TH = 32, 16                                                      # the kernel's tile (PF_TF_TW x PF_TF_TH)


def _tables(grid, mm, cost):
    R, C = mm.shape
    occ = np.asarray(grid).reshape(-1)
    c = [1.0] * (R * C) if cost is None else np.asarray(cost, np.float64).reshape(-1).tolist()
    return R, C, occ, c, mm.reshape(-1).tolist(), [fc.DR[k] * C + fc.DC[k] for k in range(8)]


def _seeded(occ, sources, RC):
    T = [[INF] * RC for _ in range(8)]
    seeds = []
    for s in sources:
        s = int(s)
        if occ[s] != 1 and T[0][s] != 0.0:
            for d in range(8):
                T[d][s] = 0.0
            seeds.append(s)
    return T, seeds


def dijkstra(grid, mm, cost, sources, wt):
    """The rule as it is written: heap entries (g, cell, heading), every popped state offers fl(g + e) to the eight states its
    moves lead to -> T float64 [8, R, C]."""
    R, C, occ, c, m, step = _tables(grid, mm, cost)
    T, seeds = _seeded(occ, sources, R * C)
    heap = [(0.0, s, d) for s in seeds for d in range(8)]
    heapq.heapify(heap)
    done = set()
    while heap:
        g, u, d0 = heapq.heappop(heap)
        if (u, d0) in done:
            continue
        done.add((u, d0))
        for d in range(8):
            if (m[u] >> d) & 1:
                v = u + step[d]
                h = 0.5 * (c[u] + c[v])
                w = h if d < 4 else SQRT2 * h
                t = g + (w if d == d0 else w + wt)
                if t < T[d][v]:
                    T[d][v] = t
                    heapq.heappush(heap, (t, v, d))
    return np.array(T).reshape(8, R, C)


def dijkstra_fast(grid, mm, cost, sources, wt):
    """The kernel's form, T[d][v] = min(T[d][u] + w, M[u] + (w + wt)): a popped state makes its one straight offer, and the first
    state popped of a cell (its M) the eight turned ones.  The same least fixed point, in a quarter of the offers."""
    R, C, occ, c, m, step = _tables(grid, mm, cost)
    T, seeds = _seeded(occ, sources, R * C)
    heap = [(0.0, s, d) for s in seeds for d in range(8)]
    heapq.heapify(heap)
    done, seen = set(), set()
    push, pop = heapq.heappush, heapq.heappop
    while heap:
        g, u, d0 = pop(heap)
        if (u, d0) in done:
            continue
        done.add((u, d0))
        mu, cu = m[u], c[u]
        if (mu >> d0) & 1:
            v = u + step[d0]
            h = 0.5 * (cu + c[v])
            t = g + (h if d0 < 4 else SQRT2 * h)
            if t < T[d0][v]:
                T[d0][v] = t
                push(heap, (t, v, d0))
        if u not in seen:
            seen.add(u)
            for d in range(8):
                if (mu >> d) & 1:
                    v = u + step[d]
                    h = 0.5 * (cu + c[v])
                    t = g + ((h if d < 4 else SQRT2 * h) + wt)
                    if t < T[d][v]:
                        T[d][v] = t
                        push(heap, (t, v, d))
    return np.array(T).reshape(8, R, C)


def info_of(grid, best, sources):
    return ck.info_of(grid, best, sources)


def fields(grid, cost, sets, wt, ad, rs, solver=dijkstra_fast):
    """-> (T float64 [B, 8, R, C], best float64 [B, R, C], info int64 [B, 4]) of the B source sets (flat ids)."""
    grid = np.asarray(grid)
    mm = fc.move_masks(grid, ad, rs)
    T = np.array([solver(grid, mm, cost, s, wt) for s in sets])
    best = T.min(axis=1)
    info = np.array([info_of(grid, best[b], s) for b, s in enumerate(sets)], np.int64).reshape(len(sets), 4)
    return T, best, info


def sweeps(grid, mm, cost, sources, wt, seed, variant=None):
    """Relaxation sweeps over the states in a fresh random order each, in place, until one whole sweep lowers nothing -> T float64
    [8, R, C].  Any order reaches the same least fixed point, bit for bit.  variant: a deliberately WRONG solver that the checker's
    own test must reject -- "two_roundings": a turning step summed as (M + w) + wt, two roundings where the rule has one;
    "first_turn": the first move out of a source is charged as a turn."""
    R, C, occ, c, m, step = _tables(grid, mm, cost)
    T, seeds = _seeded(occ, sources, R * C)
    seeds = set(seeds)
    rnd = np.random.default_rng(seed)
    states = [(v, d) for v in range(R * C) if occ[v] != 1 for d in range(8) if (m[v] >> fc.OPP[d]) & 1]
    while True:
        changed = False
        for i in rnd.permutation(len(states)):
            v, d = states[i]
            u = v - step[d]
            h = 0.5 * (c[u] + c[v])
            w = h if d < 4 else SQRT2 * h
            least = min(T[k][u] for k in range(8))
            turned = (least + w) + wt if variant == "two_roundings" else least + (w + wt)
            straight = INF if variant == "first_turn" and u in seeds else T[d][u] + w
            t = straight if straight < turned else turned
            if t < T[d][v]:
                T[d][v] = t
                changed = True
        if not changed:
            return np.array(T).reshape(8, R, C)


def route(T, cost, t, wt, heading=None):
    """The route rule on the states T [8, R, C] of one set: the cells source -> target as a list ([] where the target has no finite
    state).  heading: chase the walk into the state (t, heading) instead of the best one (such a walk may pass a cell twice)."""
    _, R, C = T.shape
    Tf = T.reshape(8, -1)
    c = np.ones(R * C) if cost is None else np.asarray(cost, np.float64).reshape(-1)
    if not 0 <= t < R * C:
        return []
    d = min(range(8), key=lambda k: (Tf[k, t], k)) if heading is None else heading
    if not np.isfinite(Tf[d, t]):
        return []
    v, cells = int(t), [int(t)]
    if heading is None and Tf[:, t].min() == 0.0:
        return cells
    while True:
        u = v - (fc.DR[d] * C + fc.DC[d])
        w = ck.weight(c, u, v, d)
        cells.append(u)
        if Tf[:, u].min() == 0.0:
            return cells[::-1]
        offers = [(Tf[k, u], k) for k in range(8) if Tf[k, u] + (w if k == d else w + wt) == Tf[d, v]]
        assert offers and len(cells) <= 8 * R * C, (v, d)
        v, d = u, min(offers)[1]


def path_cost(cost, cells, C, wt):
    """(the rule's left-to-right float64 cost, the turns) of the flat cells; every step must be a king move."""
    n = max(int(v) for v in cells) + 1
    c = np.ones(n) if cost is None else np.asarray(cost, np.float64).reshape(-1)
    total, turns, prev = 0.0, 0, None
    for a, b in zip(cells[:-1], cells[1:]):
        step = (int(b) // C - int(a) // C, int(b) % C - int(a) % C)
        assert max(abs(step[0]), abs(step[1])) == 1, (a, b)
        w = ck.weight(c, int(a), int(b), 4 if step[0] and step[1] else 0)
        if prev is not None and prev != step:
            total, turns = total + (w + wt), turns + 1
        else:
            total = total + w
        prev = step
    return total, turns


def count_turns(cells, C):
    """helper.py's count_turns on flat cells."""
    steps = [(int(b) // C - int(a) // C, int(b) % C - int(a) % C) for a, b in zip(cells[:-1], cells[1:])]
    return sum(1 for x, y in zip(steps[:-1], steps[1:]) if x != y)


def simple_path_minimum(grid, mm, cost, src, wt):
    """best[v] = the smallest rule cost over ALL simple paths from src to v (a depth-first enumeration: tiny grids only)."""
    R, C = mm.shape
    m = mm.reshape(-1).tolist()
    best = [INF] * (R * C)
    if np.asarray(grid).reshape(-1)[src] == 1:
        return np.array(best).reshape(R, C)

    def walk(path):
        total = path_cost(cost, path, C, wt)[0]
        if total < best[path[-1]]:
            best[path[-1]] = total
        for k in range(8):
            if (m[path[-1]] >> k) & 1:
                x = path[-1] + fc.DR[k] * C + fc.DC[k]
                if x not in path:
                    walk(path + [x])
    walk([int(src)])
    return np.array(best).reshape(R, C)


# ---- the maps of the tests
def pocket_map():
    """A corridor of three cells with the source at one end: the state (middle cell, entered from the far end) is reached only by
    walking past the middle cell into the dead end and back -> (grid, source, the state's cell, the state's heading)."""
    return np.zeros((1, 3), np.uint8), 0, 1, 1


def zigzag_map():
    """The seeded 18 x 23 map: Dijkstra's route from the first free cell to the last turns 16 times -> (grid, source, target)."""
    g = fc.seeded_map(18, 23, 0.25, 7)
    free = np.flatnonzero(g.reshape(-1) != 1)
    return g, int(free[0]), int(free[-1])


def detour_map(stacked):
    """Two tiles of the kernel, side by side (TH x 2 TW) or stacked (2 TH x TW), cost_checkers-style: the near tile costs 50 a cell,
    the far tile 1; a band of cost 2^10 crosses the near tile between the source and the rest of it; a road of cost 1 runs along the
    first row (column) through the band to the far tile.  The cells of the near tile beyond the band are cheapest by the road INTO
    the far tile and back -> (cost, source, probe cell, in_far_tile)."""
    if not stacked:
        cost = np.full((TH, 2 * TW), 50.0)
        cost[:, TW:] = 1.0
        cost[:, TW // 3:2 * TW // 3] = 2.0 ** 10
        cost[0, 3:] = 1.0
        return cost, (TH // 2) * 2 * TW + 2, (TH - 1) * 2 * TW + TW - 2, lambda v: v % (2 * TW) >= TW
    cost = np.full((2 * TH, TW), 50.0)
    cost[TH:, :] = 1.0
    cost[TH // 4:TH // 4 + 3, :] = 2.0 ** 10
    cost[1:, 0] = 1.0
    return cost, 0 * TW + 8, (TH - 1) * TW + TW - 2, lambda v: v // TW >= TH


def needs_the_far_tile(cost, s, probe, in_far_tile, wt, ad, rs):
    """True when best[probe] with the far tile walled off is strictly larger than with it: every optimal walk into the probe leaves
    the near tile and comes back, so a schedule that starts with the source's tile alone needs at least three launches."""
    g = np.zeros(cost.shape, np.uint8)
    open_best = fields(g, cost, [[s]], wt, ad, rs)[1][0].reshape(-1)[probe]
    walled = g.copy()
    walled.reshape(-1)[[v for v in range(g.size) if in_far_tile(v)]] = 1
    near_best = fields(walled, cost, [[s]], wt, ad, rs)[1][0].reshape(-1)[probe]
    return not in_far_tile(s) and not in_far_tile(probe) and np.isfinite(near_best) and open_best < near_best
