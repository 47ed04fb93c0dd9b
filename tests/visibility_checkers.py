"""The CPU model of the visibility fields (include/pathfit.h: pf_visibility_field, pf_visibility_count, pf_visibility_paths; DESIGN.md
4.24), in integers only, built on the rule of tests/smooth_model.py (blockers / all_pairs), and the cases the visibility tests share.

`seen` is the definition: one smooth_model.visible per target.  `seen_map` computes the same mask for a whole map at once by asking,
per obstacle cell, which targets it hides (numpy over targets x obstacles); tests/test_visibility_checkers.py pins it to `seen`."""
import functools

import numpy as np

import smooth_model as sm


def occ_of(g):
    return (np.asarray(g) == 1).astype(np.uint8)


def in_range(R, C, a, max_range_sq):
    """bool [R, C]: dr^2 + dc^2 <= max_range_sq (-1: everywhere)."""
    rr, cc = np.mgrid[0:R, 0:C]
    d2 = (rr - a[0]) ** 2 + (cc - a[1]) ** 2
    return np.ones((R, C), bool) if max_range_sq < 0 else d2 <= max_range_sq


def seen(occ, a, strict, max_range_sq=-1, targets=None):
    """What the cell a = (r, c) sees: bool [R, C] (targets None), else bool [len(targets)] for the (r, c) pairs of `targets`."""
    R, C = occ.shape
    cells = [(r, c) for r in range(R) for c in range(C)] if targets is None else [tuple(int(v) for v in t) for t in targets]
    a = (int(a[0]), int(a[1]))
    out = np.zeros(len(cells), bool)
    for i, b in enumerate(cells):
        if max_range_sq >= 0 and (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2 > max_range_sq:
            continue
        out[i] = occ[a] != 1 and occ[b] != 1 and sm.visible(occ, a, b, strict)
    return out.reshape(R, C) if targets is None else out


def seen_map(occ, a, strict, max_range_sq=-1, chunk=1 << 22):
    """`seen` for every cell of the map at once: a target is hidden iff some obstacle cell of its bounding box has |2k| < s (<= s when
    strict); int64 throughout."""
    R, C = occ.shape
    r0, c0 = int(a[0]), int(a[1])
    out = np.zeros((R, C), bool)
    if occ[r0, c0] == 1:
        return out
    ob = np.argwhere(occ == 1).astype(np.int64)
    rr, cc = (v.reshape(-1).astype(np.int64) for v in np.mgrid[0:R, 0:C])
    dr, dc = rr - r0, cc - c0
    s = np.abs(dr) + np.abs(dc)
    hidden = occ.reshape(-1) == 1
    step = max(1, chunk // max(len(ob), 1))
    for i in range(0, R * C, step) if len(ob) else ():
        j = slice(i, i + step)
        orr, occ_c = ob[:, 0][None, :], ob[:, 1][None, :]
        k2 = np.abs(2 * (dr[j, None] * (occ_c - c0) - dc[j, None] * (orr - r0)))
        box = (orr >= np.minimum(r0, rr[j])[:, None]) & (orr <= np.maximum(r0, rr[j])[:, None]) & \
              (occ_c >= np.minimum(c0, cc[j])[:, None]) & (occ_c <= np.maximum(c0, cc[j])[:, None])
        hit = box & ((k2 <= s[j, None]) if strict else (k2 < s[j, None]))
        hidden[j] |= hit.any(axis=1)
    out = ~hidden.reshape(R, C)
    return out & in_range(R, C, (r0, c0), max_range_sq)


def corner_lines(occ, strict):
    """What (0, 0) sees along the three pure lines through it, for a map too large for `seen` -> (diagonal, row 0, column 0) bool.
    On a pure diagonal k = i (c - r): the cells with c == r are crossed and those with |c - r| == 1 inside the box [0, i]^2 touched;
    on a pure row or column only the line's own cells count and nothing is touched (2 |d| |offset| == |d| has no solution)."""
    n = min(occ.shape)
    ob = occ == 1
    d = np.arange(n)
    on = np.cumsum(ob[d, d]) > 0                                      # an obstacle on the diagonal at or before i
    beside = np.zeros(n, bool)
    if n > 1:
        j = np.arange(n - 1)
        beside[1:] = np.cumsum(ob[j, j + 1] | ob[j + 1, j]) > 0        # (j, j + 1) and (j + 1, j) lie in the box of i iff j < i
    diag = ~(on | (beside if strict else False))
    return diag & ~ob[0, 0], (np.cumsum(ob[0, :]) == 0), (np.cumsum(ob[:, 0]) == 0)


def field_info(mask, a):
    """pf_visibility_field's info words for one mask."""
    ids = np.flatnonzero(mask.reshape(-1))
    if len(ids) == 0:
        return [0, -1, -1, 0]
    C = mask.shape[1]
    d2 = (ids // C - a[0]) ** 2 + (ids % C - a[1]) ** 2
    return [len(ids), int(d2.max()), int(ids[d2 == d2.max()].min()), 0]


def exposure(occ, views, strict, max_range_sq=-1):
    """int32 [R, C]: the number of viewpoints (duplicates count again) that see each cell."""
    out = np.zeros(occ.shape, np.int32)
    for a in views:
        out += seen_map(occ, a, strict, max_range_sq)
    return out


def count_info(occ, counts):
    """pf_visibility_count's info words."""
    free = np.flatnonzero(occ.reshape(-1) != 1)
    if len(free) == 0:
        return [0, 0, -1, -1]
    n = counts.reshape(-1)[free]
    return [int((n > 0).sum()), len(free), int(n.max()), int(free[n == n.max()].min())]


def path_exposure(counts, rows, path_cap):
    """What pf_visibility_paths leaves -> (out int64 [n, 4], status int32 [n], profiles list)."""
    flat = np.asarray(counts).reshape(-1)
    out, st, prof = np.zeros((len(rows), 4), np.int64), np.zeros(len(rows), np.int32), []
    for i, row in enumerate(rows):
        row = np.asarray(row, np.int64)
        if len(row) < 1 or len(row) > path_cap or ((row < 0) | (row >= flat.size)).any():
            out[i], st[i] = [0, -1, -1, 0], 1
            prof.append(None)
            continue
        v = flat[row].astype(np.int64)
        out[i] = [v.sum(), v.max(), int(np.flatnonzero(v == v.max())[0]), int((v > 0).sum())]
        prof.append(v.astype(np.int32))
    return out, st, prof


# ---------------------------------------------------------------------------- shared cases
def sample_targets(R, C, seed, n):
    """n seeded cells of an R x C map as (r, c) pairs (with repeats on a small map)."""
    ids = np.random.default_rng(seed).integers(0, R * C, n)
    return [(int(v) // C, int(v) % C) for v in ids]


def diagonal_gap_map():
    """Two obstacles that meet in a corner point: the diagonal between them is open under the loose rule only."""
    g = np.zeros((6, 7), np.uint8)
    g[2, 3] = g[3, 2] = 1
    return g, (2, 2), (3, 3)


LARGE_SHAPE = (300, 517)
LARGE_VIEWS = [(150, 258), (7, 9), (291, 500)]
LARGE_SAMPLE = 2000


@functools.lru_cache(maxsize=None)
def large_map(open_map=False):
    g = np.zeros(LARGE_SHAPE, np.uint8)
    if not open_map:
        g[np.random.default_rng(24).random(LARGE_SHAPE) < 0.012] = 1
        for a in LARGE_VIEWS:
            g[a] = 0
    return g


@functools.lru_cache(maxsize=None)
def large_sample(open_map, strict):
    """-> [(viewpoint, targets, seen bool [LARGE_SAMPLE])] for the three viewpoints of the 300 x 517 map, by the definition."""
    occ = occ_of(large_map(open_map))
    out = []
    for i, a in enumerate(LARGE_VIEWS):
        t = sample_targets(*LARGE_SHAPE, 100 + i, LARGE_SAMPLE)
        out.append((a, t, seen(occ, a, strict, -1, t)))
    return out
