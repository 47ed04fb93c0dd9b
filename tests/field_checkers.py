"""CPU checkers for the routing trees (pf_dist_field_parents / pf_dist_field_paths): a plain Dijkstra shaped like the reference's
(dijkstra.py:43-96: heap entries (g, cell), a closed set, came_from overwritten on a strict improvement only), the FIELD-ONLY parent
rule in numpy, and a path tracer.  tests/test_field_parent_rule.py pins them against each other on any host; the GPU tests compare
the device against them.  Cells are flat ids r * C + c, which order like the reference's (r, c) tuples.

Parent codes (uint8 [R, C]): 0..7 = the move index k (helper.py:30-36 order) of the tree's last step into v, v = parent + move k;
8 = the source; 255 = an obstacle or a cell out of reach."""
import heapq
import math

import numpy as np

INF = float("inf")
SQRT2 = math.sqrt(2.0)
DR = (0, 0, 1, -1, 1, 1, -1, -1)          # helper.py:30-36 move order
DC = (1, -1, 0, 0, 1, -1, 1, -1)
OPP = (1, 0, 3, 2, 7, 6, 5, 4)            # the move that undoes move k
W = (1.0, 1.0, 1.0, 1.0, SQRT2, SQRT2, SQRT2, SQRT2)
POLICIES = ((1, 1), (1, 0), (0, 1), (0, 0))
SOURCE, NONE = 8, 255


def shifted(a, dr, dc, fill):
    """out[r, c] = a[r + dr, c + dc], `fill` outside."""
    R, C = a.shape
    out = np.full_like(a, fill)
    if abs(dr) < R and abs(dc) < C:
        out[max(0, -dr):R - max(0, dr), max(0, -dc):C - max(0, dc)] = a[max(0, dr):R - max(0, -dr), max(0, dc):C - max(0, -dc)]
    return out


def move_masks(grid, ad, rs):
    """bit k of [r, c]: move k from (r, c) is legal -- target inside and free, the cell itself free; a diagonal needs allow_diag
    and, under restrict_corner, both orthogonal neighbours free (helper.py get_valid_neighbors)."""
    free = np.asarray(grid) != 1
    mm = np.zeros(free.shape, np.uint8)
    for k in range(8 if ad else 4):
        ok = free & shifted(free, DR[k], DC[k], False)
        if k >= 4 and rs:
            ok &= shifted(free, DR[k], 0, False) & shifted(free, 0, DC[k], False)
        mm |= ok.astype(np.uint8) << k
    return mm


def reference_dijkstra(grid, mm, src):
    """dijkstra.py:43-96 with no target: -> (labels float64 [R, C], parent codes uint8 [R, C]).  The reference keeps one heap entry
    per open cell and lowers it in place; here a lowered cell is pushed again and its stale entries are skipped as closed, which
    pops the live entries in the same (g, cell) order."""
    R, C = mm.shape
    dist = [INF] * (R * C)
    code = [NONE] * (R * C)
    if np.asarray(grid).reshape(-1)[src] == 1:
        return np.array(dist).reshape(R, C), np.array(code, np.uint8).reshape(R, C)
    m = mm.reshape(-1).tolist()
    step = [DR[k] * C + DC[k] for k in range(8)]
    dist[src], code[src] = 0.0, SOURCE
    closed = set()
    heap = [(0.0, src)]
    while heap:
        g, u = heapq.heappop(heap)
        if u in closed:
            continue
        closed.add(u)
        for k in range(8):
            if (m[u] >> k) & 1:
                v = u + step[k]
                if v in closed:
                    continue
                t = g + W[k]
                if t < dist[v]:                                       # :84, strict
                    dist[v], code[v] = t, k
                    heapq.heappush(heap, (t, v))
    return np.array(dist).reshape(R, C), np.array(code, np.uint8).reshape(R, C)


def rule_parents(field, mm, largest_u=False):
    """The field-only rule: parent(v) = the u with the smallest (D[u], u) among the cells with a legal move u -> v and
    D[u] + w == D[v]; legality from v's own mask (bit OPP[k]: the graph is symmetric).  largest_u: the deliberately WRONG tie-break
    (the largest u among the cells that offer the final label) that the checker's own test must reject."""
    R, C = field.shape
    ids = np.arange(R * C, dtype=np.int64).reshape(R, C)
    best_d = np.full((R, C), INF)
    best_u = np.full((R, C), -1, np.int64)
    code = np.full((R, C), NONE, np.uint8)
    finite = np.isfinite(field)
    for k in range(8):
        du = shifted(field, -DR[k], -DC[k], INF)
        u = ids - (DR[k] * C + DC[k])
        ok = ((mm >> OPP[k]) & 1 == 1) & finite & (du + W[k] == field)
        if largest_u:
            take = ok & (u > best_u)
        else:
            take = ok & ((du < best_d) | ((du == best_d) & ((best_u < 0) | (u < best_u))))
        best_d = np.where(take, du, best_d)
        best_u = np.where(take, u, best_u)
        code = np.where(take, np.uint8(k), code)
    code[field == 0.0] = SOURCE
    return code


def trace(code, target):
    """The tree's path source -> target as a list of flat cells ([] where the target's code is 255)."""
    R, C = code.shape
    flat = code.reshape(-1)
    if not 0 <= target < R * C or flat[target] == NONE:
        return []
    out, v = [int(target)], int(target)
    while flat[v] != SOURCE:
        k = int(flat[v])
        assert k < 8 and len(out) <= R * C, (v, k)
        v -= DR[k] * C + DC[k]
        out.append(v)
    return out[::-1]


def seeded_map(R=18, C=23, frac=0.25, seed=7):
    """The seeded 18 x 23 map with 25 % obstacles."""
    return (np.random.default_rng(seed).random((R, C)) < frac).astype(np.uint8)


def serpentine(n):
    """Every other row a wall with one gap, at alternating ends: one corridor of about n * n / 2 cells."""
    g = np.zeros((n, n), np.uint8)
    for i, r in enumerate(range(1, n, 2)):
        g[r, :] = 1
        g[r, n - 1 if i % 2 == 0 else 0] = 0
    return g
