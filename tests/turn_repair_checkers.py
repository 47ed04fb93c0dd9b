"""The CPU model of the turn-field repair (pf_turn_field_repair, pathfit.TurnField.repair) on turn_checkers / repair_checkers: the
raise phase over (cell, heading) states -- sweeps in a seeded random order, in place, until one whole sweep raises nothing --; the
rewritten best; the re-seed; the lower phase as a tile queue whose first queue follows the rule; the state words raised, also by one
pass in ascending label order and by a worklist from the changed cells (quick enough for the GPU tests' large maps); and the maps
whose facts the GPU tests lean on.  tests/test_turn_repair_checkers.py pins the model against turn_checkers.dijkstra on the new map,
bit for bit, and makes it reject three wrong repairs.  Plain IEEE double arithmetic, one rounded operation at a time.

The rule.  T is a least fixed point for an old map and cost map.  Under the NEW occupancy, mask and costs a state (v, d) is supported
when v is free and T[d][v] == 0, or v is free with a finite label, the move u -> v (u = v - step(d)) is legal and SOME d' gives
T[d'][u] + e(d', d) == T[d][v] for u's current labels, e = w for d' == d and (w + wt) -- rounded first -- otherwise: the LITERAL form.
form="two_read" is the relax kernel's form, T[d][u] + w == x or M[u] + (w + wt) == x with M[u] the minimum of u's CURRENT labels:
not the rule in general (M rises while states are raised); the checker's test compares the two."""
import numpy as np

import cost_checkers as ck
import field_checkers as fc
import repair_checkers as rc
import turn_checkers as tk

INF = tk.INF
TILE = (tk.TH, tk.TW)                                                # rows x columns of the device's tile
VARIANTS = rc.VARIANTS                                               # the wrong repairs the checker's test must reject
FORMS = ("literal", "two_read")


def ones_if_none(cost, shape):
    return np.ones(shape) if cost is None else np.asarray(cost, np.float64)


def changed_cells(grid0, cost0, grid1, cost1):
    """repair_checkers.changed_cells; a cost map of None is a map of ones."""
    s = np.asarray(grid0).shape
    return rc.changed_cells(grid0, ones_if_none(cost0, s), grid1, ones_if_none(cost1, s))


def _setup(grid, cost, ad, rs):
    grid = np.asarray(grid)
    R, C = grid.shape
    occ = grid.reshape(-1).tolist()
    m = fc.move_masks(grid, ad, rs).reshape(-1).tolist()
    c = ones_if_none(cost, grid.shape).reshape(-1).tolist()
    return R, C, occ, m, c, [fc.DR[k] * C + fc.DC[k] for k in range(8)]


def _w(c, u, v, d):
    h = 0.5 * (c[u] + c[v])
    return h if d < 4 else tk.SQRT2 * h


def supported(T, occ, m, c, step, wt, v, d, form="literal", keep=None):
    """The rule for the finite state (v, d) under the current labels T [8][RC] (keep: only supporters marked there count)."""
    x = T[d][v]
    if occ[v] == 1:
        return False
    if x == 0.0:
        return True
    if not (m[v] >> fc.OPP[d]) & 1:
        return False
    u = v - step[d]
    w = _w(c, u, v, d)
    e = w + wt
    if form == "two_read":
        return T[d][u] + w == x or min(T[k][u] for k in range(8)) + e == x
    for k in range(8):
        if (keep is None or keep[k][u]) and T[k][u] + (w if k == d else e) == x:
            return True
    return False


def raise_phase(T, occ, m, c, C, wt, seed, changed=(), variant=None, form="literal"):
    """In place on T [8][RC] -> the states (v, d) raised, in the order they went.  variant "legal_from_changed": only the changed
    cells, the cells with a legal move from one, and the cells with a legal move from a cell with a raised state are looked at."""
    step = [fc.DR[k] * C + fc.DC[k] for k in range(8)]
    rnd = np.random.default_rng(seed)
    RC = len(T[0])
    look = None
    if variant == "legal_from_changed":
        look = set(int(x) for x in changed)
        look |= {x + step[k] for x in list(look) for k in range(8) if (m[x] >> k) & 1}
    raised = []
    if variant == "no_raise":
        return raised
    while True:
        cells = sorted(look) if look is not None else range(RC)
        states = [(v, d) for v in cells for d in range(8) if T[d][v] != INF]
        moved = False
        for i in rnd.permutation(len(states)):
            v, d = states[i]
            if T[d][v] == INF or supported(T, occ, m, c, step, wt, v, d, form):
                continue
            T[d][v] = INF
            raised.append((v, d))
            moved = True
            if look is not None:
                look |= {v + step[k] for k in range(8) if (m[v] >> k) & 1}
        if not moved:
            return raised


def lower_phase(T, occ, m, c, R, C, wt, first, seed, tile=TILE):
    """The tile queue, in place on T [8][RC]: every queued tile's states are swept in a random order to the tile's own fixed point
    (the relax kernel's form); a tile that holds a cell within one step of a cell with a lowered state goes on the next queue
    -> (rounds, tile visits, states lowered at least once)."""
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
            states = [(r * C + k, d) for r in range(ty * tile[0], min((ty + 1) * tile[0], R)) for k in range(tx * tile[1], min((tx + 1) * tile[1], C))
                      if occ[r * C + k] != 1 for d in range(8) if (m[r * C + k] >> fc.OPP[d]) & 1]
            fell = set()
            while True:
                moved = False
                for j in rnd.permutation(len(states)):
                    v, d = states[j]
                    u = v - step[d]
                    w = _w(c, u, v, d)
                    straight, turned = T[d][u] + w, min(T[k][u] for k in range(8)) + (w + wt)
                    t = straight if straight < turned else turned
                    if t < T[d][v]:
                        T[d][v] = t
                        fell.add((v, d))
                        moved = True
                if not moved:
                    break
            for v in {v for v, _ in fell}:
                nxt |= rc.block_tiles(v, R, C, tile) - {(ty, tx)}
            fell_all |= fell
        queue = nxt
    return rounds, visits, fell_all


class Repair:
    """One repair by the model: .T float64 [8, R, C], .best [R, C], .best_raised (best after the raise phase), .raised (states, in
    order), .n_raised, .first (the lower phase's first queue), .lowered (states), .reseeded (the sources whose words were not all 0)."""


def repair(T_old, grid, cost, sources, wt, changed, ad, rs, seed=0, variant=None, tile=TILE, form="literal"):
    """T_old [8, R, C]: a least fixed point for `sources` on an old map; grid, cost: the NEW map; changed: flat ids -> a Repair."""
    R, C, occ, m, c, _ = _setup(grid, cost, ad, rs)
    T = np.asarray(T_old, np.float64).reshape(8, -1).tolist()
    out = Repair()
    out.raised = raise_phase(T, occ, m, c, C, wt, seed, changed, variant, form)
    out.n_raised = len(out.raised)
    out.best_raised = np.array(T).min(axis=0).reshape(R, C)
    out.reseeded = [s for s in sorted({int(s) for s in sources}) if occ[s] != 1 and any(T[d][s] != 0.0 for d in range(8))]
    for s in out.reseeded:
        for d in range(8):
            T[d][s] = 0.0
    first = rc.tiles_of([v for v, _ in out.raised], C, tile)
    if variant != "lower_touched_only":
        first |= rc.tiles_of(out.reseeded, C, tile)
        for x in changed:
            first |= rc.block_tiles(x, R, C, tile)
    out.first = first
    out.rounds, out.visits, out.lowered = lower_phase(T, occ, m, c, R, C, wt, first, seed + 1, tile)
    out.T = np.array(T).reshape(8, R, C)
    out.best = out.T.min(axis=0)
    return out


def raised_by_label_order(T_old, grid, cost, wt, ad, rs):
    """The states the raise phase raises, without sweeps: a supporter's label is strictly smaller, so one pass over the finite
    states in ascending label order decides every state after its possible supporters -> sorted (v, d) pairs."""
    R, C, occ, m, c, step = _setup(grid, cost, ad, rs)
    flat = np.asarray(T_old, np.float64).reshape(8, -1)
    T = flat.tolist()
    RC = R * C
    keep = [bytearray(RC) for _ in range(8)]
    gone = []
    for i in np.argsort(flat.reshape(-1), kind="stable").tolist():
        d, v = divmod(i, RC)
        if T[d][v] == INF:
            break
        if supported(T, occ, m, c, step, wt, v, d, keep=keep):
            keep[d][v] = 1
        else:
            gone.append((v, d))
    return sorted(gone)


def raised_by_worklist(T_old, grid, cost, wt, changed, ad, rs):
    """The same set from the changed cells outwards: the states of the cells in the 3 x 3 blocks about the changed cells are
    examined, and whenever a state of u is raised, the states its moves lead to are examined again.  Any order of examination
    reaches the unique surviving set; a state outside every block whose supporters all stand is never examined and stands.  The
    work follows the raised set, not the map -> sorted (v, d) pairs."""
    R, C, occ, m, c, step = _setup(grid, cost, ad, rs)
    T = np.asarray(T_old, np.float64).reshape(8, -1).tolist()
    todo = []
    for x in set(int(x) for x in changed):
        r, k = divmod(x, C)
        todo += [(rr * C + kk, d) for rr in range(max(r - 1, 0), min(r + 1, R - 1) + 1) for kk in range(max(k - 1, 0), min(k + 1, C - 1) + 1) for d in range(8)]
    gone = []
    while todo:
        v, d = todo.pop()
        if T[d][v] == INF or supported(T, occ, m, c, step, wt, v, d):
            continue
        T[d][v] = INF
        gone.append((v, d))
        r, k = divmod(v, C)
        for e in range(8):                                            # (the old mask may have had moves the new one lacks: every neighbour in the grid)
            rr, kk = r + fc.DR[e], k + fc.DC[e]
            if 0 <= rr < R and 0 <= kk < C:
                todo.append((rr * C + kk, e))
    return sorted(gone)


def min_raise_launches(raised, changed, R, C, tile=TILE):
    return rc.min_raise_launches([v for v, _ in raised], changed, R, C, tile)


def fresh(grid, cost, sources, wt, ad, rs):
    """The heap Dijkstra's states [8, R, C] on a map: the answer a repair must reproduce bit for bit."""
    grid = np.asarray(grid)
    return tk.dijkstra_fast(grid, fc.move_masks(grid, ad, rs), cost, sources, wt)


same_bits = rc.same_bits


def seeded_change(grid, cost, kind, n, seed, keep=()):
    """repair_checkers.seeded_change; kind None: no cost map, the cells only toggle -> (grid, cost or None)."""
    if kind is not None:
        return rc.seeded_change(grid, cost, kind, n, seed, keep)
    rnd = np.random.default_rng(seed)
    g = np.array(grid).copy()
    for v in [v for v in rnd.permutation(g.size) if int(v) not in keep][:n]:
        r, k = divmod(int(v), g.shape[1])
        g[r, k] = 0 if g[r, k] == 1 else 1
    return g, None


def cost_of_kind(kind, shape, seed):
    return None if kind is None else ck.cost_of_kind(kind, shape, seed)


# ---- the maps built for the three rejections (tests/test_turn_repair_checkers.py asserts what each is for)
def closed_corridor_case():
    """repair_checkers' map: closing a cell of the top corridor cuts the only way round -> (g0, g1, cost, sources, wt, policy)."""
    g, g2, c, s, pol = rc.closed_corridor_case()
    return g, g2, c, s, 0.3, pol


def corner_rule_case():
    """repair_checkers' map under the restricted policy: closing x = (1, 1) makes the diagonal (1, 0) -> (0, 1) illegal though
    neither end has a legal move from x; the state ((0, 1), move 6) must go."""
    g, g2, c, s, pol = rc.corner_rule_case()
    return g, g2, c, s, 0.3, pol


def falling_cost_case():
    """A 1 x 3 corridor a, x, s with sources at both ends, c[x] = 3, wt = 1: both states of x hold 2.  When c[x] falls to 1 each is
    still supported -- by a TURNED offer of its source, 0 + (1 + 1) == 2 -- and nothing is raised; yet the answer is 1.  A repair
    that queues only the tiles with a raised word for lowering leaves 2."""
    g = np.zeros((1, 3), int)
    c = np.ones((1, 3))
    c[0, 1] = 3.0
    return g, c, np.ones((1, 3)), [0, 2], 1.0, (0, 0)


def two_read_case():
    """The seeded 4 x 4 case on which the two forms of the support rule differ (turn weight 0, the free diagonal policy, integer
    costs): three cells change, two costs and one opening; the state (cell 6, move 6) keeps its label under the literal form -- 18
    states are raised -- and is raised by the two-read form, 19 -> (g0, c0, g1, c1, sources, wt, policy)."""
    g0 = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 0, 1, 0]])
    g1 = g0.copy()
    g1[3, 2] = 0
    c0 = np.array([[1.0, 1.0, 3.0, 4.0], [3.0, 2.0, 4.0, 3.0], [3.0, 2.0, 1.0, 4.0], [4.0, 1.0, 1.0, 4.0]])
    c1 = c0.copy()
    c1[1, 0], c1[1, 2], c1[3, 2] = 4.0, 2.0, 4.0
    return g0, c0, g1, c1, [2, 7, 3], 0.0, (1, 0)


# ---- the maps of the GPU cases whose facts are asserted on the CPU
def finite_rise_case(R=3, C=3):
    """An open R x C map under the 4-connected policy, the source at the west end of the middle row, v at its east end: v is cheapest
    straight along the row; closing the cell west of v raises that state, while the states that enter v from the rows above and
    below keep their support: best[v] rises to a finite value -> (g0, g1, source, v, changed cell, wt, policy)."""
    g = np.zeros((R, C), int)
    mid = R // 2
    g1 = g.copy()
    g1[mid, C - 2] = 1
    return g, g1, mid * C, mid * C + C - 1, mid * C + C - 2, 0.5, (0, 0)


def pocket_change():
    """turn_checkers.pocket_map with a change in the pocket: the state (middle cell, entered from the far end) is reached only by
    walking past the middle cell into the dead end and back; closing the dead end raises it and the dead end's own state, and
    opening it again brings both back -> (g0, g1, source, cell, heading)."""
    g, s, cell, heading = tk.pocket_map()
    g1 = np.array(g).copy()
    g1[0, 2] = 1
    return np.array(g, int), g1.astype(int), s, cell, heading
