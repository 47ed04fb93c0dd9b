"""The CPU model of the cost-field repair (pf_cost_field_repair, pathfit.CostField.repair) on cost_checkers / field_checkers: the
changed list of two (grid, cost) pairs; the raise phase -- sweeps in a seeded random order, in place, until one whole sweep raises
nothing --; the re-seed; the lower phase as a tile queue whose first queue follows the rule; the words raised; and the facts about a
case that the GPU tests lean on (which tiles hold a raised word, how many raise launches any timing needs).
tests/test_repair_checkers.py pins the model against cost_checkers.dijkstra on the new map, bit for bit, and makes it reject three
wrong repairs.  Everything is plain IEEE double arithmetic, one rounded operation at a time.

The rule.  D is a least fixed point for an old map and cost map.  Under the NEW occupancy, mask and costs a cell v is supported when
it is a free source of the set with label 0, or free with a finite label and some u has a legal move u -> v with
D[u] + w_new(u, v) == D[v] for u's current label.  A finite label on an obstacle and every unsupported finite label become inf,
until nothing changes; every free source takes 0; the lowering starts from the tiles that had a word raised, that meet the 3 x 3
block about a changed cell, or that hold a re-seeded source."""
import numpy as np

import cost_checkers as ck
import field_checkers as fc

INF = ck.INF
TILE = (16, 64)                                                      # rows x columns of the device's tile
VARIANTS = ("no_raise", "legal_from_changed", "lower_touched_only")  # the wrong repairs the checker's test must reject


def changed_cells(grid0, cost0, grid1, cost1):
    """Flat ids, ascending: the free / obstacle state differs, or the cell is free in both maps and its cost differs."""
    g0, g1 = np.asarray(grid0).reshape(-1), np.asarray(grid1).reshape(-1)
    c0, c1 = np.asarray(cost0, np.float64).reshape(-1), np.asarray(cost1, np.float64).reshape(-1)
    out = []
    for v in range(g0.size):
        f0, f1 = g0[v] != 1, g1[v] != 1
        if f0 != f1 or (f0 and f1 and c0[v] != c1[v]):
            out.append(v)
    return out


def block_tiles(x, R, C, tile=TILE):
    """The tiles (ty, tx) that meet the 3 x 3 block about flat cell x."""
    r, c = divmod(int(x), C)
    return {(rr // tile[0], cc // tile[1]) for rr in range(max(r - 1, 0), min(r + 1, R - 1) + 1) for cc in range(max(c - 1, 0), min(c + 1, C - 1) + 1)}


def tiles_of(cells, C, tile=TILE):
    return {((int(v) // C) // tile[0], (int(v) % C) // tile[1]) for v in cells}


def _weights(c, u, v, k):
    h = 0.5 * (c[u] + c[v])
    return h if k < 4 else ck.SQRT2 * h


def raise_phase(D, occ, m, c, C, srcs, seed, changed=(), variant=None):
    """In place on the flat list D -> the cells raised, in the order they went.  variant "legal_from_changed": only the changed
    cells, the cells with a legal move from one, and the cells with a legal move from a raised cell are ever looked at."""
    step = [fc.DR[k] * C + fc.DC[k] for k in range(8)]
    rnd = np.random.default_rng(seed)
    look = None
    if variant == "legal_from_changed":
        look = set(int(x) for x in changed)
        look |= {x + step[k] for x in list(look) for k in range(8) if (m[x] >> k) & 1}
    raised = []
    if variant == "no_raise":
        return raised
    while True:
        cells = sorted(look) if look is not None else list(range(len(D)))
        moved = False
        for i in rnd.permutation(len(cells)):
            v = cells[i]
            d = D[v]
            if d == INF:
                continue
            held = False
            if occ[v] != 1:
                held = d == 0.0 and v in srcs
                for k in range(8):
                    if held:
                        break
                    if (m[v] >> fc.OPP[k]) & 1:
                        u = v - step[k]
                        held = D[u] + _weights(c, u, v, k) == d
            if not held:
                D[v] = INF
                raised.append(v)
                moved = True
                if look is not None:
                    look |= {v + step[k] for k in range(8) if (m[v] >> k) & 1}
        if not moved:
            return raised


def lower_phase(D, occ, m, c, R, C, first, seed, tile=TILE):
    """The tile queue, in place on the flat list D: every queued tile is swept in a random order to its own fixed point; a tile that
    holds a cell within one step of a lowered cell goes on the next queue -> (rounds, tile visits, cells lowered at least once)."""
    step = [fc.DR[k] * C + fc.DC[k] for k in range(8)]
    rnd = np.random.default_rng(seed)
    queue, rounds, visits, fell_all = set(first), 0, 0, set()
    while queue:
        rounds += 1
        nxt = set()
        order = sorted(queue)
        for i in rnd.permutation(len(order)):
            ty, tx = order[i]
            visits += 1
            cells = [r * C + k for r in range(ty * tile[0], min((ty + 1) * tile[0], R)) for k in range(tx * tile[1], min((tx + 1) * tile[1], C))
                     if occ[r * C + k] != 1]
            fell = set()
            while True:
                moved = False
                for j in rnd.permutation(len(cells)):
                    v = cells[j]
                    best = D[v]
                    for k in range(8):
                        if (m[v] >> fc.OPP[k]) & 1:
                            u = v - step[k]
                            t = D[u] + _weights(c, u, v, k)
                            if t < best:
                                best = t
                    if best < D[v]:
                        D[v] = best
                        fell.add(v)
                        moved = True
                if not moved:
                    break
            for v in fell:
                nxt |= block_tiles(v, R, C, tile) - {(ty, tx)}
            fell_all |= fell
        queue = nxt
    return rounds, visits, fell_all


class Repair:
    """One repair by the model: .D float64 [R, C], .raised (cells, in order), .n_raised, .first (the lower phase's first queue),
    .lowered (cells), .reseeded (the sources that took 0)."""


def repair(D_old, grid, cost, sources, changed, ad, rs, seed=0, variant=None, tile=TILE):
    """D_old [R, C]: a least fixed point for `sources` on an old map; grid, cost: the NEW map; changed: flat ids -> a Repair."""
    grid = np.asarray(grid)
    R, C = grid.shape
    occ = grid.reshape(-1).tolist()
    m = fc.move_masks(grid, ad, rs).reshape(-1).tolist()
    c = np.asarray(cost, np.float64).reshape(-1).tolist()
    D = np.asarray(D_old, np.float64).reshape(-1).tolist()
    srcs = {int(s) for s in sources}
    out = Repair()
    out.raised = raise_phase(D, occ, m, c, C, srcs, seed, changed, variant)
    out.n_raised = len(out.raised)
    out.reseeded = [s for s in sorted(srcs) if occ[s] != 1 and D[s] != 0.0]
    for s in out.reseeded:
        D[s] = 0.0
    first = tiles_of(out.raised, C, tile)
    if variant != "lower_touched_only":
        first |= tiles_of(out.reseeded, C, tile)
        for x in changed:
            first |= block_tiles(x, R, C, tile)
    out.first = first
    out.rounds, out.visits, out.lowered = lower_phase(D, occ, m, c, R, C, first, seed + 1, tile)
    out.D = np.array(D).reshape(R, C)
    return out


def raised_by_label_order(D_old, grid, cost, sources, ad, rs):
    """The cells the raise phase raises, without sweeps: a supporter's label is strictly smaller, so one pass over the finite labels
    in ascending order decides every cell after its possible supporters -> sorted flat ids.  (The sweeps' count, pinned by
    tests/test_repair_checkers.py; quick enough for the GPU tests' large maps.)"""
    grid = np.asarray(grid)
    C = grid.shape[1]
    occ = grid.reshape(-1).tolist()
    m = fc.move_masks(grid, ad, rs).reshape(-1).tolist()
    c = np.asarray(cost, np.float64).reshape(-1).tolist()
    flat = np.asarray(D_old, np.float64).reshape(-1)
    D = flat.tolist()
    srcs = {int(s) for s in sources}
    step = [fc.DR[k] * C + fc.DC[k] for k in range(8)]
    keep = bytearray(len(D))
    gone = []
    for v in np.argsort(flat, kind="stable").tolist():
        d = D[v]
        if d == INF:
            break
        held = False
        if occ[v] != 1:
            held = d == 0.0 and v in srcs
            for k in range(8):
                if held:
                    break
                if (m[v] >> fc.OPP[k]) & 1:
                    u = v - step[k]
                    held = keep[u] == 1 and D[u] + _weights(c, u, v, k) == d
        if held:
            keep[v] = 1
        else:
            gone.append(v)
    return sorted(gone)


def min_raise_launches(raised, changed, R, C, tile=TILE):
    """A lower bound on the raise launches under ANY timing: the first queue holds the tiles of the changed cells' blocks, a launch
    queues only neighbours of the tiles it visits, and a word is raised only in a visit of its own tile -- so a raised word in a
    tile k steps (king steps between tiles) from the first queue needs launch k + 1.  0 when nothing is raised."""
    first = set()
    for x in changed:
        first |= block_tiles(x, R, C, tile)
    far = 0
    for t in tiles_of(raised, C, tile):
        far = max(far, 1 + min(max(abs(t[0] - f[0]), abs(t[1] - f[1])) for f in first))
    return far


def fresh(grid, cost, sources, ad, rs):
    """The heap Dijkstra's labels on a map: the answer a repair must reproduce bit for bit."""
    grid = np.asarray(grid)
    return ck.dijkstra(grid, fc.move_masks(grid, ad, rs), cost, sources)[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def seeded_change(grid, cost, kind, n, seed, keep=()):
    """n mixed changes on a copy of (grid, cost): a cell toggles between free and obstacle (a cell that opens takes a cost of the
    kind) or a free cell's cost is drawn again, rising or falling; the cells of `keep` are left alone -> (grid, cost)."""
    rnd = np.random.default_rng(seed)
    g, c = np.array(grid).copy(), np.array(cost, np.float64).copy()
    draw = ck.cost_of_kind(kind, g.shape, seed + 977).reshape(-1)
    cells = [v for v in rnd.permutation(g.size) if int(v) not in keep][:n]
    for v in cells:
        r, k = divmod(int(v), g.shape[1])
        if g[r, k] == 1:
            g[r, k], c[r, k] = 0, draw[v]
        elif rnd.random() < 0.5:
            g[r, k] = 1
        else:
            c[r, k] = draw[v] if draw[v] != c[r, k] else min(c[r, k] + 1.0, ck.COST_MAX)
    return g, c


# ---- the maps built for the three rejections (tests/test_repair_checkers.py asserts what each is for)
def closed_corridor_case():
    """A 3 x 7 map with a wall along the middle row, open at its right end; the source in the top left corner.  Closing a cell of
    the top corridor cuts the only way round: everything behind it is out of reach, and a repair without a raise phase keeps the old
    finite labels, which lie below the answer (inf)."""
    g = np.zeros((3, 7), int)
    g[1, :6] = 1
    g2 = g.copy()
    g2[0, 3] = 1
    return g, g2, np.ones(g.shape), [0], (1, 1)


def corner_rule_case():
    """A 2 x 2 block of free cells inside a 3 x 3 map, the source at (1, 0), under the restricted policy: (0, 1) is cheapest by the
    diagonal (1, 0) -> (0, 1), which passes (1, 1) and (0, 0).  Closing x = (1, 1) makes that diagonal illegal, though neither of
    its ends has a legal move from x, before or after; the label sqrt(2) behind it must go, and the answer is 2 by way of (0, 0)."""
    g = np.zeros((3, 3), int)
    g[2, :] = 1
    g2 = g.copy()
    g2[1, 1] = 1
    return g, g2, np.ones(g.shape), [3], (1, 1)


def falling_cost_case():
    """A 1 x 4 corridor a, x, b, s with sources at both ends, all costs 1 but c[x] = 3: D = 0, 2, 1, 0, x by way of a.  When c[x] falls
    to 1, x is still supported -- by b: 1 + 1 == 2 -- and nothing is raised; yet the answer is D[x] = 1.  A repair that queues only the
    tiles with a raised word for lowering leaves 2."""
    g = np.zeros((1, 4), int)
    c = np.ones((1, 4))
    c[0, 1] = 3.0
    c2 = np.ones((1, 4))
    return g, c, c2, [0, 3], (0, 0)


# ---- the maps of the GPU cases whose facts are asserted on the CPU
def sealed_room_map(R=24, C=150):
    """A walled room in the right part with one door in its west wall, reached from the source at (1, 1); a second, fully sealed room
    below it that no source reaches -> (grid, door cell, a cell inside the room, a cell inside the sealed room)."""
    g = np.zeros((R, C), int)
    g[2:14, 70] = g[2:14, C - 2] = 1
    g[2, 70:C - 1] = g[13, 70:C - 1] = 1
    door = 7 * C + 70
    g[7, 70] = 0
    g[16:R - 1, 80] = g[16:R - 1, 100] = 1
    g[16, 80:101] = g[R - 2, 80:101] = 1
    return g, door, 8 * C + 100, 19 * C + 90


def long_corridor(n=200):
    """A 1 x n corridor, the source at its west end: closing cell 1 invalidates cells 2 .. n - 1, across the tiles 0 .. (n - 1) // 64 in
    a chain -- each learns of it from its western neighbour, one launch later."""
    return np.zeros((1, n), int), 0, 1
