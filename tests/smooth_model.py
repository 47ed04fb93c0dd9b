"""The CPU model of any-angle smoothing (include/pathfit.h: pf_line_of_sight_batch, pf_smooth_batch), written from the
rule alone with Python integers and numpy, and the case tables the smoothing tests share.

Cells are (r, c); a cell's square is [r - 1/2, r + 1/2] x [c - 1/2, c + 1/2].  For a = (r0, c0), b = (r1, c1), dr = r1 - r0,
dc = c1 - c0, s = |dr| + |dc| and a cell of the bounding box, k = dr (c - c0) - dc (r - r0): the segment between the centres crosses
the open square iff |2k| < s and touches it in a corner point only iff |2k| == s.  tests/test_smooth_model.py pins this against exact
rational clipping."""
import functools

import numpy as np

import golden_io as gio
import thin_maps

MAPS20 = ("fig7", "fig13", "img1", "img2", "img3")
PATHS_PER_MAP = 61


# ---------------------------------------------------------------------------- the rule
def _box(a, b):
    """|2k| over the bounding box of a and b -> (lowest row, lowest column, int64 [rows, columns], s)."""
    (r0, c0), (r1, c1) = a, b
    dr, dc = r1 - r0, c1 - c0
    rlo, clo = min(r0, r1), min(c0, c1)
    r = np.arange(rlo, max(r0, r1) + 1, dtype=np.int64)[:, None]
    c = np.arange(clo, max(c0, c1) + 1, dtype=np.int64)[None, :]
    return rlo, clo, np.abs(2 * (dr * (c - c0) - dc * (r - r0))), abs(dr) + abs(dc)


def _cells(rlo, clo, mask):
    return [(int(r) + rlo, int(c) + clo) for r, c in np.argwhere(mask)]


def segment_cells(a, b):
    """-> (crossed, touched): lists of (r, c) in row-major order.  a == b: the cell itself is crossed."""
    if tuple(a) == tuple(b):
        return [tuple(a)], []
    rlo, clo, k2, s = _box(a, b)
    return _cells(rlo, clo, k2 < s), _cells(rlo, clo, k2 == s)


def blockers(occ, a, b, strict):
    """The obstacle cells that hide b from a, in row-major order."""
    rlo, clo, k2, s = _box(a, b)
    ob = occ[rlo:rlo + k2.shape[0], clo:clo + k2.shape[1]] == 1
    if tuple(a) != tuple(b):
        ob = ob & ((k2 <= s) if strict else (k2 < s))
    return _cells(rlo, clo, ob) if ob.any() else []


def visible(occ, a, b, strict):
    return not blockers(occ, a, b, strict)


def first_block(occ, a, b, strict):
    """The blocking cell of the major index nearest a (columns if |dc| >= |dr|, else rows), the smallest r C + c among that
    index's blocking cells, as a cell id; -1 when b is visible."""
    bl = blockers(occ, a, b, strict)
    if not bl:
        return -1
    C = occ.shape[1]
    ax = 1 if abs(b[1] - a[1]) >= abs(b[0] - a[0]) else 0
    return min((abs(p[ax] - a[ax]), p[0] * C + p[1]) for p in bl)[1]


def smooth(occ, cells, strict, log=None):
    """Forward string pulling, first failure -> the list of kept positions in `cells` (cell ids).  log: a list that takes
    (anchor position, tested position, visible) per test."""
    C = occ.shape[1]
    p = [(int(x) // C, int(x) % C) for x in cells]
    L = len(p)
    if L == 0:
        return []
    out, a, j = [0], 0, 1
    while j + 1 < L:
        v = visible(occ, p[a], p[j + 1], strict)
        if log is not None:
            log.append((a, j + 1, v))
        if v:
            j += 1
        else:
            out.append(j)
            a = j
            j = a + 1
    if L > 1:
        out.append(L - 1)
    return out


def stats(cells, C):
    """(length, turns) of a waypoint list (cell ids): the naive left-to-right fp64 sum of the segments' lengths; the interior waypoints
    whose two segments are not parallel and equally directed."""
    p = [(int(x) // C, int(x) % C) for x in cells]
    length, turns = np.float64(0.0), 0
    for i in range(1, len(p)):
        dr, dc = p[i][0] - p[i - 1][0], p[i][1] - p[i - 1][1]
        length = length + np.sqrt(np.float64(dr * dr + dc * dc))
        if i > 1:
            pr, pc = p[i - 1][0] - p[i - 2][0], p[i - 1][1] - p[i - 2][1]
            if pr * dc - pc * dr != 0 or pr * dr + pc * dc < 0:
                turns += 1
    return float(length), turns


def smooth_row(occ, cells, strict, way_cap=None):
    """What pf_smooth_batch leaves for one row -> (status, waypoint cells, positions, length, turns)."""
    cells = np.asarray(cells, np.int64)
    if len(cells) == 0 or ((cells < 0) | (cells >= occ.size)).any():
        return 1, np.zeros(0, np.int32), np.zeros(0, np.int32), 0.0, 0
    idx = np.array(smooth(occ, cells, strict), np.int32)
    if way_cap is not None and len(idx) > way_cap:
        return 3, np.zeros(0, np.int32), np.zeros(0, np.int32), 0.0, 0
    way = cells[idx].astype(np.int32)
    length, turns = stats(way, occ.shape[1])
    return 0, way, idx, length, turns


# ---------------------------------------------------------------------------- the rule for every pair of a small map at once
def all_pairs(occ, strict):
    """visible [RC, RC] bool and first_block [RC, RC] int32 of every ordered pair (a, b) of a small map, numpy over (b, cell)."""
    R, C = occ.shape
    RC = R * C
    rr, cc = (v.reshape(-1) for v in np.mgrid[0:R, 0:C])
    ob = occ.reshape(-1) == 1
    vis, fb = np.zeros((RC, RC), bool), np.full((RC, RC), -1, np.int32)
    ids = np.arange(RC)
    for a in range(RC):
        r0, c0 = a // C, a % C
        dr, dc = (rr - r0)[:, None], (cc - c0)[:, None]                     # [b, 1]
        s = np.abs(dr) + np.abs(dc)
        k2 = np.abs(2 * (dr * (cc - c0)[None, :] - dc * (rr - r0)[None, :]))    # [b, cell]
        box = (rr[None, :] >= np.minimum(r0, rr)[:, None]) & (rr[None, :] <= np.maximum(r0, rr)[:, None]) & \
              (cc[None, :] >= np.minimum(c0, cc)[:, None]) & (cc[None, :] <= np.maximum(c0, cc)[:, None])
        hit = box & ob[None, :] & ((k2 < s) | ((k2 == s) if strict else False))
        hit[a, :] = False
        hit[a, a] = ob[a]                                                  # a == b: the cell itself
        colmaj = (np.abs(dc) >= np.abs(dr))
        major = np.where(colmaj, np.abs(cc - c0)[None, :], np.abs(rr - r0)[None, :])
        key = np.where(hit, major.astype(np.int64) * RC + ids[None, :], np.int64(1) << 40).min(axis=1)
        vis[a] = ~hit.any(axis=1)
        fb[a] = np.where(vis[a], -1, key % RC)
    return vis, fb


# ---------------------------------------------------------------------------- case tables
@functools.lru_cache(maxsize=None)
def astar_cases(name, count=PATHS_PER_MAP, seed=7):
    """`count` non-empty paths of the oracle's A* on a golden map: variants 0, 1, 2 in turn, between seeded free cells
    -> (grid, [int32 cell arrays])."""
    import pf_oracle as po
    g, _, _ = gio.grid(name)
    o = po.Oracle(g)
    free = np.flatnonzero(g.reshape(-1) != 1)
    rnd = np.random.default_rng(seed)
    paths = []
    while len(paths) < count:
        s, t = (int(v) for v in rnd.choice(free, 2, replace=False))
        p, _ = o.astar(s, t, None, len(paths) % 3)
        if len(p):
            paths.append(np.asarray(p, np.int32))
    return g, paths


@functools.lru_cache(maxsize=None)
def thin_cases():
    """The thin maps of tests/thin_maps.py with the oracle's A* path start -> target (variant 0) -> [(name, grid, path)]."""
    import pf_oracle as po
    out = []
    for R, C, ob in thin_maps.all_maps():
        g, s, t = thin_maps.thin_map(R, C, ob)
        p, _ = po.Oracle(g).astar(s, t, None, 0)
        out.append((thin_maps.name_of(R, C, ob), g, np.asarray(p, np.int32)))
    return out


def occ_of(g):
    return (np.asarray(g) == 1).astype(np.uint8)


def input_length(cells, C):
    return stats(cells, C)[0]
