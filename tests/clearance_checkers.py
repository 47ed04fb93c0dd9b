"""The CPU models of the clearance fields (include/pathfit.h: pf_clearance_field, pf_clearance_paths, pf_clearance_segments;
DESIGN.md 4.16), written from the rule and from nothing else, and the map builders of the clearance tests.

The rule: d2[v] = the smallest (rv - ro)^2 + (cv - co)^2 over the obstacle cells o (grid value 1), PF_CLEAR_NONE without one; with
`border` min(r + 1, R - r, c + 1, C - c)^2 takes part too; near[v] = the obstacle of smallest id r C + c among the nearest ones
(never the border).  tests/test_clearance_checkers.py pins the brute force against an independently written separable transform
and against the reference's own safety term."""
import math

import numpy as np

import smooth_model as sm

NONE = 2 ** 31 - 1
LIST_BUDGET = 60_000_000                                              # obstacles x cells the plain list form may cost


def _by_list(obst, rr, cc, C):
    """Every obstacle of `obst` (ids in increasing order) offered to the cells (rr, cc) in turn, a strict `<`: the first of the
    nearest ones, that is the smallest id, stays -> (d2 int64, near int64)."""
    best = np.full(rr.shape, NONE, np.int64)
    near = np.full(rr.shape, -1, np.int64)
    for o in obst:
        ro, co = int(o) // C, int(o) % C
        d = (rr - ro) ** 2 + (cc - co) ** 2
        upd = d < best
        best[upd] = d[upd]
        near[upd] = o
    return best, near


def _by_offsets(ob, w):
    """The same offers made offset by offset, (dr, dc) from (-w, -w) to (w, w) in id order, a strict `<` -> (d2, near, settled):
    a cell is settled when its best is below (w + 1)^2, the least any obstacle outside the window can reach."""
    R, C = ob.shape
    pad = np.zeros((R + 2 * w, C + 2 * w), bool)
    pad[w:w + R, w:w + C] = ob
    ids = np.arange(R * C, dtype=np.int64).reshape(R, C)
    best = np.full((R, C), NONE, np.int64)
    near = np.full((R, C), -1, np.int64)
    for dr in range(-w, w + 1):
        for dc in range(-w, w + 1):
            d = dr * dr + dc * dc
            upd = pad[w + dr:w + dr + R, w + dc:w + dc + C] & (d < best)
            best[upd] = d
            near[upd] = ids[upd] + dr * C + dc
    return best, near, best < (w + 1) ** 2


def brute_force(grid, border=False, window=None):
    """-> (d2 int32 [R, C], near int32 [R, C], info int64 [4]).  Brute force over the obstacle list in id order with a strict `<`.
    A map whose list form would cost more than LIST_BUDGET (or any map when `window` is given) makes the same offers offset by
    offset inside a window first and runs the list only for the cells the window does not settle."""
    g = np.asarray(grid)
    R, C = g.shape
    ob = g == 1
    obst = np.flatnonzero(ob.reshape(-1))
    rr, cc = (v.astype(np.int64) for v in np.mgrid[0:R, 0:C])
    if window is None and len(obst) * R * C <= LIST_BUDGET:
        best, near = _by_list(obst, rr, cc, C)
    else:
        best, near, settled = _by_offsets(ob, 8 if window is None else int(window))
        open_ = ~settled
        if open_.any():
            best[open_], near[open_] = _by_list(obst, rr[open_], cc[open_], C)
    if border:
        m = np.minimum(np.minimum(rr + 1, R - rr), np.minimum(cc + 1, C - cc))
        best = np.minimum(best, m * m)
    return best.astype(np.int32), near.astype(np.int32), info_of(g, best)


def info_of(grid, d2):
    """int64 [4]: obstacle cells, free cells, the largest d2 over the free cells, the smallest cell id that attains it (-1, -1
    without a free cell)."""
    free = (np.asarray(grid) != 1).reshape(-1)
    d = np.asarray(d2, np.int64).reshape(-1)
    nfree = int(free.sum())
    if nfree == 0:
        return np.array([free.size, 0, -1, -1], np.int64)
    top = int(d[free].max())
    return np.array([free.size - nfree, nfree, top, int(np.flatnonzero(free & (d == top))[0])], np.int64)


def margin_sq(margin):
    """The smallest integer n with math.sqrt(n) >= margin, found by counting up."""
    n = 0
    while math.sqrt(n) < margin:
        n += 1
    return n


def inflated(grid, d2, msq):
    out = np.array(grid, dtype=int)
    out[np.asarray(d2) < msq] = 1
    return out


def path_row(d2, cells, cap, margin_d2):
    """What pf_clearance_paths leaves for one row -> (status, out int32 [4], profile int32 [len] or None)."""
    flat = np.asarray(d2).reshape(-1)
    cells = np.asarray(cells, np.int64)
    if len(cells) == 0 or len(cells) > cap or ((cells < 0) | (cells >= flat.size)).any():
        return 1, np.array([NONE, -1, 0, -1], np.int32), None
    prof = flat[cells].astype(np.int32)
    low = int(prof.min())
    below = np.flatnonzero(prof < margin_d2)
    return 0, np.array([low, int(np.flatnonzero(prof == low)[0]), len(below), int(below[0]) if len(below) else -1], np.int32), prof


def segment(d2, a, b, touched):
    """(the smallest d2 over the cells the segment a -> b crosses -- and touches, when asked --, the smallest cell id that attains
    it); a, b: (r, c) pairs; (NONE, -1) when an endpoint lies beside the grid."""
    d2 = np.asarray(d2)
    R, C = d2.shape
    if not (0 <= a[0] < R and 0 <= a[1] < C and 0 <= b[0] < R and 0 <= b[1] < C):
        return NONE, -1
    crossed, touch = sm.segment_cells(a, b)
    cells = crossed + (touch if touched else [])
    return min((int(d2[r, c]), r * C + c) for r, c in cells)


def safety_term(d2, cells, min_safe):
    """helper.py:67-80 from the field: the naive left-to-right fp64 sum of pow(min_safe - sqrt(d2), 2.0) over the cells with
    sqrt(d2) < min_safe, divided by the row length -> (the term, the number of cells that paid)."""
    flat = np.asarray(d2).reshape(-1)
    total, paid = 0.0, 0
    for v in cells:
        x = int(flat[int(v)])
        dist = math.sqrt(x) if x != NONE else math.inf
        if dist < min_safe:
            total += math.pow(min_safe - dist, 2.0)
            paid += 1
    return (total / len(cells) if len(cells) else 0.0), paid


# ---- map builders (uint8, 1 = obstacle)
def seeded(R, C, frac, seed):
    return (np.random.default_rng(seed).random((R, C)) < frac).astype(np.uint8)


def few(R, C, n, seed):
    g = np.zeros((R, C), np.uint8)
    g.reshape(-1)[np.random.default_rng(seed).choice(R * C, n, replace=False)] = 1
    return g


def shifted_copy(g):
    out = np.zeros((g.shape[0] + 1, g.shape[1] + 1), np.uint8)
    out[1:, 1:] = g
    return out


def one_per_row(R, C, seed):
    """One obstacle per row at a seeded column: most of a column's parabolas are dominated."""
    g = np.zeros((R, C), np.uint8)
    g[np.arange(R), np.random.default_rng(seed).integers(0, C, R)] = 1
    return g


def first_column_only(R, C, n, seed):
    """Obstacles in column 0 only, at n seeded rows: in column c every parabola has the same height c^2."""
    g = np.zeros((R, C), np.uint8)
    g[np.random.default_rng(seed).choice(R, n, replace=False), 0] = 1
    return g


def tie_maps():
    """Pairs of obstacles placed symmetrically about the centre cell of a 9 x 11 map: left / right, up / down, the four diagonals,
    at distances 1 to 4, and all of them at once."""
    R, C, r, c = 9, 11, 4, 5
    out = []
    for k in (1, 2, 3, 4):
        for (ar, ac), (br, bc) in (((0, -k), (0, k)), ((-k, 0), (k, 0)), ((-k, -k), (k, k)), ((-k, k), (k, -k)), ((-k, -k), (-k, k)),
                                   ((k, -k), (k, k)), ((-k, -k), (k, -k)), ((-k, k), (k, k)), ((0, -k), (-k, 0)), ((0, k), (k, 0))):
            g = np.zeros((R, C), np.uint8)
            g[r + ar, c + ac] = g[r + br, c + bc] = 1
            out.append(g)
        g = np.zeros((R, C), np.uint8)
        for dr in (-k, 0, k):
            for dc in (-k, 0, k):
                if dr or dc:
                    g[r + dr, c + dc] = 1
        out.append(g)
    return out
