"""The CPU model of the connected components (include/pathfit.h: pf_components, pf_component_sizes, pf_components_same; DESIGN.md
4.15), written from the rule and from nothing else, and the map builders of the component tests.

The rule: a cell is free iff its grid value is not 1; two free cells are adjacent iff field_checkers.move_masks allows the move;
labels[v] = -1 on an obstacle, else the rank of v's component when the components are ordered by their smallest cell id r * C + c.
tests/test_component_checkers.py pins the flood fill against the transitive closure of the adjacency matrix."""
import numpy as np

import field_checkers as fc


def flood_fill(grid, ad, rs):
    """-> (labels int32 [R, C], sizes int64 [count], first cells int32 [count]): an explicit-stack flood fill over the move masks,
    seeds taken in cell order, so a component's number is the rank of its smallest cell."""
    g = np.asarray(grid)
    R, C = g.shape
    mm = fc.move_masks(g, ad, rs).reshape(-1).tolist()
    free = (g.reshape(-1) != 1).tolist()
    steps_of = [tuple(fc.DR[k] * C + fc.DC[k] for k in range(8) if (m >> k) & 1) for m in range(256)]   # the legal moves of a mask byte
    lab = [-1] * (R * C)
    sizes, first = [], []
    for s in range(R * C):
        if not free[s] or lab[s] >= 0:
            continue
        k = len(sizes)
        lab[s] = k
        stack, n = [s], 0
        while stack:
            v = stack.pop()
            n += 1
            for d in steps_of[mm[v]]:
                u = v + d
                if lab[u] < 0:
                    lab[u] = k
                    stack.append(u)
        sizes.append(n)
        first.append(s)
    return np.array(lab, np.int32).reshape(R, C), np.array(sizes, np.int64), np.array(first, np.int32)


def info_of(sizes):
    """int64 [4]: count, free cells, the largest size, its label (the lowest on a tie; -1 without a component)."""
    if len(sizes) == 0:
        return np.array([0, 0, 0, -1], np.int64)
    return np.array([len(sizes), int(sizes.sum()), int(sizes.max()), int(np.argmax(sizes))], np.int64)


def closure_labels(grid, ad, rs):
    """The components from the transitive closure of the adjacency matrix (small maps only) -> labels int32 [R, C]."""
    g = np.asarray(grid)
    R, C = g.shape
    n = R * C
    mm = fc.move_masks(g, ad, rs).reshape(-1)
    free = g.reshape(-1) != 1
    A = np.zeros((n, n), bool)
    for v in range(n):
        if free[v]:
            A[v, v] = True
        for k in range(8):
            if (mm[v] >> k) & 1:
                A[v, v + fc.DR[k] * C + fc.DC[k]] = True
    for _ in range(max(1, int(np.ceil(np.log2(n))) + 1)):             # reach within 2^t steps
        A = A | ((A.astype(np.int32) @ A.astype(np.int32)) > 0)
    lab = np.full(n, -1, np.int32)
    nxt = 0
    for v in range(n):
        if free[v] and lab[v] < 0:
            lab[A[v] & (lab < 0)] = nxt
            nxt += 1
    return lab.reshape(R, C)


def masks_symmetric(grid, ad, rs):
    """Move k is legal from v iff the move that undoes it is legal from v + move k."""
    mm = fc.move_masks(grid, ad, rs)
    for k in range(8):
        there = (mm >> k) & 1
        back = fc.shifted((mm >> fc.OPP[k]) & 1, fc.DR[k], fc.DC[k], 0)
        if not np.array_equal(there, back):
            return False
    return True


# ---- map builders (uint8, 1 = obstacle)
def checkerboard(R, C):
    """Free where r + c is even: one component under (1, 0), every free cell its own component under the other three policies."""
    rr, cc = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
    return ((rr + cc) % 2 == 1).astype(np.uint8)


def row_serpentine(R, C):
    """Every other row a wall with one gap, at alternating ends: one corridor of about R * C / 2 cells."""
    g = np.zeros((R, C), np.uint8)
    for i, r in enumerate(range(1, R, 2)):
        g[r, :] = 1
        g[r, C - 1 if i % 2 == 0 else 0] = 0
    return g


def col_serpentine(R, C):
    return np.ascontiguousarray(row_serpentine(C, R).T)


def rings(R, C, gap=3):
    """Concentric sealed rectangular walls, `gap` cells apart: nested components, one per band between two walls."""
    g = np.zeros((R, C), np.uint8)
    for d in range(gap - 1, min(R, C) // 2, gap):
        g[d, d:C - d] = 1
        g[R - 1 - d, d:C - d] = 1
        g[d:R - d, d] = 1
        g[d:R - d, C - 1 - d] = 1
    return g


def seeded_random(R, C, frac, seed):
    return (np.random.default_rng(seed).random((R, C)) < frac).astype(np.uint8)


def shifted_copy(g):
    """The map behind one free row and one free column: every structure meets the tile borders one cell further on."""
    out = np.zeros((g.shape[0] + 1, g.shape[1] + 1), np.uint8)
    out[1:, 1:] = g
    return out


def split_wall(R, C, w, g):
    """A full wall that runs down column w for the rows above g and down column w + 1 from row g on: the free cells (g - 1, w + 1)
    and (g, w) touch diagonally across two wall cells, so the two sides are joined by one corner-cutting diagonal and by nothing
    else (split_wall_labels)."""
    m = np.zeros((R, C), np.uint8)
    m[:g, w] = 1
    m[g:, w + 1] = 1
    return m


def split_wall_labels(R, C, w, g, ad, rs):
    """The answer for split_wall, written down -> (labels, sizes, first cells).  Cell (0, 0) is free, so the left side is component 0;
    the right side begins at (0, w + 1).  Under (1, 0) the diagonal joins them into one component."""
    assert 0 < g < R and 0 < w < C - 2
    lab = np.zeros((R, C), np.int32)
    lab[:g, w + 1:] = 1
    lab[g:, w + 2:] = 1
    left, right = g * w + (R - g) * (w + 1), g * (C - w - 1) + (R - g) * (C - w - 2)
    if ad and not rs:
        lab[:] = 0
    lab[:g, w] = -1
    lab[g:, w + 1] = -1
    if ad and not rs:
        return lab, np.array([left + right], np.int64), np.array([0], np.int32)
    return lab, np.array([left, right], np.int64), np.array([0, w + 1], np.int32)
