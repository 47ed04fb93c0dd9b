"""The CPU model of the widest-path fields (include/pathfit.h: pf_clearance_widest), written from the rule and from
nothing else, and the map builders of the widest-path tests.

The rule: the capacity of a move u -> v is min(d2[u], d2[v]); a diagonal under restrict_corner also takes the two side cells' d2 into
the minimum, and does not exist without allow_diag.  w[v] = the largest, over all walks from a source to v, of the smallest capacity
on the walk; d2[s] on a source with d2[s] >= 1; 0 where nothing of capacity >= 1 arrives.  The model is a max-heap widest-path
search (Dijkstra's algorithm on the (max, min) semiring).  tests/test_widest_checkers.py pins it against threshold-then-flood-fill."""
import heapq

import numpy as np

import field_checkers as fc

NONE = 2 ** 31 - 1
POLICIES = fc.POLICIES


def widest_one(d2, sources, ad, rs):
    """-> (w int32 [R, C], the number of sources that counted).  sources: flat cell ids."""
    d2 = np.asarray(d2)
    R, C = d2.shape
    d = d2.reshape(-1).tolist()
    w = [0] * (R * C)
    heap, counted = [], 0
    for s in sources:
        s = int(s)
        if d[s] >= 1 and w[s] == 0:
            w[s] = d[s]
            counted += 1
            heap.append((-d[s], s))
    heapq.heapify(heap)
    nk = 8 if ad else 4
    while heap:
        neg, u = heapq.heappop(heap)
        wu = -neg
        if wu < w[u]:
            continue                                                  # a stale entry: u has been raised since
        r, c = divmod(u, C)
        for k in range(nk):
            rr, cc = r + fc.DR[k], c + fc.DC[k]
            if not (0 <= rr < R and 0 <= cc < C):
                continue
            v = rr * C + cc
            cap = min(d[u], d[v])
            if k >= 4 and rs:
                cap = min(cap, d[r * C + cc], d[rr * C + c])
            t = min(wu, cap)
            if t >= 1 and t > w[v]:
                w[v] = t
                heapq.heappush(heap, (-t, v))
    return np.array(w, np.int32).reshape(R, C), counted


def info_of(w, counted):
    """int64 [4]: the sources that counted, the cells with w >= 1, the smallest w >= 1, the smallest cell id that attains it."""
    flat = np.asarray(w, np.int64).reshape(-1)
    hit = flat >= 1
    if not hit.any():
        return np.array([counted, 0, -1, -1], np.int64)
    low = int(flat[hit].min())
    return np.array([counted, int(hit.sum()), low, int(np.flatnonzero(flat == low)[0])], np.int64)


def widest(d2, sets, ad, rs):
    """sets: a list of lists of flat cell ids -> (w int32 [B, R, C], info int64 [B, 4])."""
    rows, infos = [], []
    for s in sets:
        w, n = widest_one(d2, s, ad, rs)
        rows.append(w)
        infos.append(info_of(w, n))
    return np.stack(rows), np.stack(infos)


def csr(sets):
    off = np.zeros(len(sets) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in sets])
    return off, np.concatenate([np.asarray(s, np.int32) for s in sets]) if off[-1] else np.zeros(0, np.int32)


def inflated_with_markers(grid, d2, msq, source, target):
    """The map widest_path searches: 1 wherever d2 < msq, the START marker on the source and the TARGET marker on the target."""
    g = np.array(grid, dtype=int)
    g[g > 1] = 0
    g[np.asarray(d2) < msq] = 1
    g.reshape(-1)[source] = 2
    if target != source:
        g.reshape(-1)[target] = 3
    return g


def widest_path(grid, d2, source, target, ad, rs, w=None):
    """-> (the cells of the shortest route among the widest ones, w[target]): the reference-shaped Dijkstra's path on the inflated
    map ([] and 0 when no robot gets through).  source, target: flat ids."""
    if w is None:
        w = widest_one(d2, [source], ad, rs)[0]
    t = int(np.asarray(w).reshape(-1)[target])
    if t < 1:
        return [], 0
    g = inflated_with_markers(grid, d2, t, source, target)
    mm = fc.move_masks(g, ad, rs)
    return fc.trace(fc.reference_dijkstra(g, mm, source)[1], target), t


# ---- map builders (uint8, 1 = obstacle)
def seeded(R, C, frac, seed):
    return (np.random.default_rng(seed).random((R, C)) < frac).astype(np.uint8)


def shifted_rows(g):
    out = np.zeros((g.shape[0] + 1, g.shape[1]), np.uint8)
    out[1:] = g
    return out


def shifted_cols(g):
    out = np.zeros((g.shape[0], g.shape[1] + 1), np.uint8)
    out[:, 1:] = g
    return out


def door_ladder(n_rooms, room=9, height=13):
    """A chain of rooms side by side, room k and room k + 1 joined by a door k + 1 cells wide in the wall between them: from a source
    in the LAST room w steps down room by room towards the first -> (grid, the centre cell of every room)."""
    R, C = height, n_rooms * (room + 1) + 1
    g = np.zeros((R, C), np.uint8)
    g[0, :] = g[R - 1, :] = 1
    centres = []
    for k in range(n_rooms + 1):
        c = k * (room + 1)
        g[:, c] = 1
        if 0 < k < n_rooms:
            top = (R - k) // 2
            g[top:top + k, c] = 0
    for k in range(n_rooms):
        centres.append((R // 2) * C + k * (room + 1) + 1 + room // 2)
    return g, centres


def doors_map(n=40, seed=3):
    """An n x n map of 3 x 3 rooms whose walls hold doors of seeded widths 1 to 4."""
    rnd = np.random.default_rng(seed)
    g = np.zeros((n, n), np.uint8)
    cuts = [n // 3, 2 * n // 3]
    for x in cuts:
        g[x, :] = 1
        g[:, x] = 1
    spans = [(0, cuts[0]), (cuts[0] + 1, cuts[1]), (cuts[1] + 1, n)]
    for x in cuts:
        for lo, hi in spans:
            wd = int(rnd.integers(1, 5))
            p = int(rnd.integers(lo + 1, hi - wd - 1))
            g[x, p:p + wd] = 0
            wd = int(rnd.integers(1, 5))
            p = int(rnd.integers(lo + 1, hi - wd - 1))
            g[p:p + wd, x] = 0
    return g


def corner_gap(R, C, r, c):
    """A full wall down column c - 1 above row r and down column c from row r on (component_checkers.split_wall): the free cells
    (r - 1, c) and (r, c - 1) touch diagonally across the wall cells (r - 1, c - 1) and (r, c), and nothing else joins the two
    sides.  With r and c multiples of the tile's height and width the four cells lie in four different tiles."""
    m = np.zeros((R, C), np.uint8)
    m[:r, c - 1] = 1
    m[r:, c] = 1
    return m


def plateau_map(R, C, gap):
    """Parallel full-width walls `gap` rows apart with a staggered door each: between two walls d2 is constant along the rows, so
    large areas of equal d2 cross several tiles."""
    g = np.zeros((R, C), np.uint8)
    for i, r in enumerate(range(gap, R - 1, gap + 1)):
        g[r, :] = 1
        p = (7 + 37 * i) % (C - 6)
        g[r, p:p + 1 + i % 3] = 0
    return g
