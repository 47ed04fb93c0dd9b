"""CPU checkers for the tours (pf_tour_matrix / pf_tour_solve): the Held-Karp rule in its literal dictionary form,
a numpy layer form for m = 16, brute force over permutations with left-to-right sums, route_cost, seeded matrices of five kinds
and four deliberately WRONG solvers that tests/test_tour_checkers.py must tell from the rule.  Nodes are 0..n - 1, node 0 the start;
mode 0 open, 1 return, 2 last; need[j] = the bit set of nodes that must come before j (None: no needs).  Doubles are compared as
64-bit words (`bits`)."""
import itertools
import struct

import numpy as np

INF = float("inf")
KINDS = ("ints", "uniform", "euclid", "asym", "holes")
MODES = (0, 1, 2)


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def middle(n, mode):
    """The middle nodes, ascending."""
    return list(range(1, n - 1 if mode == 2 else n))


def matrix(kind, n, seed):
    """A seeded n x n matrix: "ints" small integers with ties everywhere, "uniform" symmetric non-dyadic, "euclid" distances of
    seeded points, "asym" independent entries each way, "holes" asym with 25 % +inf entries.  The diagonal is 0."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    if kind == "ints":
        d = rng.integers(1, 4, (n, n)).astype(np.float64)
    elif kind == "uniform":
        u = rng.random((n, n)) * 9.7 + 0.1
        d = np.triu(u, 1) + np.triu(u, 1).T
    elif kind == "euclid":
        p = rng.random((n, 2)) * 100.0
        d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    else:
        d = rng.random((n, n)) * 9.7 + 0.1
        if kind == "holes":
            d[rng.random((n, n)) < 0.25] = INF
    d = np.ascontiguousarray(d, np.float64)
    d[np.arange(n), np.arange(n)] = 0.0
    return d


def chain_need(n, mode, perm=None):
    """need words that admit exactly one order of the middle nodes: perm (default ascending)."""
    mid = middle(n, mode) if perm is None else list(perm)
    need = [0] * n
    for a, b in zip(mid[:-1], mid[1:]):
        need[b] |= 1 << a
    return need


def route_cost(d, order, mode):
    """The left-to-right sum of the legs of `order`, closed by the leg back to order[0] in mode 1; 0.0 for fewer than two nodes."""
    seq = [int(v) for v in order]
    if mode == 1 and len(seq) > 1:
        seq = seq + [seq[0]]
    if len(seq) < 2:
        return 0.0
    t = float(d[seq[0]][seq[1]])
    for a, b in zip(seq[1:-1], seq[2:]):
        t = t + float(d[a][b])
    return t


def admissible(order, n, mode, need):
    """order is a permutation of the nodes that begins with 0 (ends with n - 1 in mode 2) and meets every need."""
    seq = [int(v) for v in order]
    if sorted(seq) != list(range(n)) or seq[0] != 0 or (mode == 2 and seq[-1] != n - 1):
        return False
    if need is None:
        return True
    seen = 0
    for v in seq:
        if mode == 2 and v == n - 1:
            break                                                     # the end's own needs are always met
        if int(need[v]) & ~seen & ~1:
            return False
        seen |= 1 << v
    return True


def _closing(d, mode, n, j):
    return None if mode == 0 else float(d[j][0] if mode == 1 else d[j][n - 1])


def held_karp(d, mode, need=None, right_to_left=False, largest_on_tie=False, need_final_only=False):
    """The rule, literally: f is a dictionary over (frozenset S, j).  -> (total, order, finite_states, last): order a list of n nodes
    (all -1 where total is +inf), finite_states the number of finite f[S][j], last the last middle node or -1.  The three flags
    switch on the WRONG solvers (summing right to left is solved by its own recursion below)."""
    n = len(d)
    if right_to_left:
        return _right_to_left(d, mode, need)
    M = middle(n, mode)
    m = len(M)
    mset = frozenset(M)
    mbits = sum(1 << v for v in M)
    if m == 0:
        total = float(d[0][1]) if mode == 2 else 0.0
        ok = total < INF
        return total, (list(range(n)) if ok else [-1] * n), 0, -1

    def blocked(S, j):
        if need is None:
            return False
        nd = int(need[j])
        if mode == 2 and (nd >> (n - 1)) & 1:
            return True
        if need_final_only and len(S) != m:
            return False
        have = sum(1 << v for v in S if v != j)
        return (nd & mbits & ~have) != 0

    f = {}
    finite = 0
    for c in range(1, m + 1):
        for comb in itertools.combinations(M, c):
            S = frozenset(comb)
            for j in comb:
                if blocked(S, j):
                    v = INF
                elif c == 1:
                    v = float(d[0][j])
                else:
                    rest = S - {j}
                    v = INF
                    for i in sorted(rest):
                        t = f[(rest, i)] + float(d[i][j])
                        if t < v or (largest_on_tie and t == v):
                            v = t
                f[(S, j)] = v
                finite += v < INF
    total, last = INF, -1
    close = {}
    for j in M:
        cl = _closing(d, mode, n, j)
        close[j] = f[(mset, j)] if cl is None else f[(mset, j)] + cl
        if close[j] < total:
            total = close[j]
    if not total < INF:
        return INF, [-1] * n, finite, -1
    hits = [j for j in M if bits(close[j]) == bits(total)]
    last = hits[-1] if largest_on_tie else hits[0]
    rev, S, j = [], mset, last
    while True:
        rev.append(j)
        rest = S - {j}
        if not rest:
            break
        hits = [i for i in sorted(rest) if bits(f[(rest, i)] + float(d[i][j])) == bits(f[(S, j)])]
        S, j = rest, (hits[-1] if largest_on_tie else hits[0])
    order = [0] + rev[::-1] + ([n - 1] if mode == 2 else [])
    return total, order, finite, last


def _right_to_left(d, mode, need):
    """A WRONG solver: the same optimum in exact arithmetic, the legs summed from the tour's end backwards."""
    n = len(d)
    M = middle(n, mode)
    mbits = sum(1 << v for v in M)
    memo = {}

    def ok(i, left):
        if need is None:
            return True
        nd = int(need[i])
        if mode == 2 and (nd >> (n - 1)) & 1:
            return False
        return (nd & left & mbits) == 0                               # nothing i needs is still to come

    def h(left, j):
        """(cost of finishing from j with the set `left` still to visit, the next node)"""
        if left == 0:
            cl = _closing(d, mode, n, j)
            return (0.0 if cl is None else cl), -1
        key = (left, j)
        if key not in memo:
            best, arg = INF, -1
            for i in M:
                if (left >> i) & 1 and ok(i, left & ~(1 << i)):
                    t = float(d[j][i]) + h(left & ~(1 << i), i)[0]
                    if t < best:
                        best, arg = t, i
            memo[key] = (best, arg)
        return memo[key]

    if not M:
        total = float(d[0][1]) if mode == 2 else 0.0
        return total, (list(range(n)) if total < INF else [-1] * n), 0, -1
    total = h(mbits, 0)[0]
    if not total < INF:
        return INF, [-1] * n, 0, -1
    order, left, j = [0], mbits, 0
    while left:
        j = h(left, j)[1]
        order.append(j)
        left &= ~(1 << j)
    return total, order + ([n - 1] if mode == 2 else []), 0, order[-1]


def held_karp_layers(d, mode, need=None):
    """The rule in numpy, layer by layer over a [2^m, m] table (bit k = node k + 1; the states with j outside S stay +inf, so a
    row's minimum over all columns is the minimum over S \\ {j}) -> held_karp's tuple.  A row minimum is the first smallest
    candidate's value, as the rule's strict `<` leaves it."""
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    M = middle(n, mode)
    m = len(M)
    if m == 0:
        return held_karp(d, mode, need)
    full = (1 << m) - 1
    nm = np.zeros(m, np.int64)
    if need is not None:
        for k in range(m):
            nd = int(need[k + 1])
            nm[k] = -1 if (mode == 2 and (nd >> (n - 1)) & 1) else (nd >> 1) & full
    masks = np.arange(1 << m, dtype=np.int64)
    pop = np.zeros(1 << m, np.int64)
    for k in range(m):
        pop += (masks >> k) & 1
    tab = np.full((1 << m, m), INF)
    for c in range(1, m + 1):
        layer = masks[pop == c]
        for k in range(m):
            S = layer[(layer >> k) & 1 == 1]
            rest = S & ~(1 << k)
            if c == 1:
                v = np.full(S.shape, d[0, k + 1])
            else:
                v = (tab[rest] + d[1:m + 1, k + 1][None, :]).min(axis=1)
            if nm[k] < 0:
                v = np.full(S.shape, INF)
            else:
                v = np.where((nm[k] & ~rest) != 0, INF, v)
            tab[S, k] = v
    finite = int(np.isfinite(tab).sum())
    close = tab[full].copy()
    if mode != 0:
        close = close + d[1:m + 1, 0 if mode == 1 else n - 1]
    total = float(close.min())
    if not total < INF:
        return INF, [-1] * n, finite, -1
    k = int(np.flatnonzero(close.view(np.int64) == np.float64(total).view(np.int64))[0])
    last = k + 1
    rev, S = [], full
    while True:
        rev.append(k + 1)
        rest = S & ~(1 << k)
        if rest == 0:
            break
        cand = tab[rest] + d[1:m + 1, k + 1]
        hit = (cand.view(np.int64) == tab[S, k].view(np.int64)) & (((rest >> np.arange(m)) & 1) == 1)
        S, k = rest, int(np.flatnonzero(hit)[0])
    return total, [0] + rev[::-1] + ([n - 1] if mode == 2 else []), finite, last


def brute_force(d, mode, need=None):
    """The minimum over all admissible orders of the left-to-right sum -> (total, an order that attains it or [-1] * n)."""
    n = len(d)
    best, arg = INF, [-1] * n
    tail = [n - 1] if mode == 2 else []
    for p in itertools.permutations(middle(n, mode)):
        order = [0] + list(p) + tail
        if not admissible(order, n, mode, need):
            continue
        t = route_cost(d, order, mode)
        if t < best:
            best, arg = t, order
    return best, arg


def nearest_neighbour(d, mode):
    """The greedy order: from the node it stands on to the nearest middle node not yet visited (the lowest index on a tie)."""
    n = len(d)
    left, order = middle(n, mode), [0]
    while left:
        j = min(left, key=lambda v: (float(d[order[-1]][v]), v))
        order.append(j)
        left.remove(j)
    return order + ([n - 1] if mode == 2 else [])


def free_cells(grid, count, seed):
    """`count` distinct free cells of the grid as (r, c) pairs, seeded."""
    g = np.asarray(grid)
    ids = np.flatnonzero(g.reshape(-1) != 1)
    pick = np.random.default_rng(seed).choice(ids, size=count, replace=False)
    return [(int(v) // g.shape[1], int(v) % g.shape[1]) for v in pick]


# Eight free cells of the golden 20 x 20 map "fig7" on which, under the default policy and end="open", the greedy order costs
# 61.45584412271571 and the optimum 49.62741699796952 (test_tour_checkers.py derives both with a heap Dijkstra; the GPU file
# confirms them against the device).
NN_MAP = "fig7"
NN_STOPS = [(16, 9), (12, 19), (9, 12), (0, 8), (10, 11), (16, 3), (13, 9), (5, 14)]

# The seeded cases on which each wrong solver differs from the rule: (kind, n, mode, seed[, need]).
WRONG_RIGHT_TO_LEFT = ("uniform", 7, 0, 2)
WRONG_LARGEST_ON_TIE = ("ints", 6, 0, 2)
WRONG_NEED = ("asym", 6, 0, 2, [0, 1 << 5, 1 << 3, 0, 0, 0])         # node 1 after node 5, node 2 after node 3
