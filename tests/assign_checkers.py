"""CPU checkers for the assignments (pf_assign_matrix / pf_assign_solve): the rule in its literal loop form for the
three modes, a numpy form vectorised over the columns of a tree step (fast enough for 1024 x 1024), brute force over all injections
with left-to-right sums, the exact-rational dual certificate, greedy_nearest, seeded matrices and five deliberately WRONG solvers that
tests/test_assign_checkers.py must tell from the rule.  A problem is an n x m matrix (n <= m), rows robots and columns tasks, +inf =
no way; mode 0 sum, 1 max, 2 max_sum.  Doubles are compared as 64-bit words (`bits`)."""
import collections
import itertools
import struct
from fractions import Fraction

import numpy as np

INF = float("inf")
MODES = (0, 1, 2)
OBJECTIVES = {"sum": 0, "max": 1, "max_sum": 2}
INT_KINDS = ("ties", "ints", "neg", "inf30", "inf55")                # every operation of the rule is exact on these
REAL_KINDS = ("real", "sqrt2")
KINDS = INT_KINDS + REAL_KINDS

# col: list of n columns (all -1 where infeasible); sum, max: the value; dual: float64 [n + m] = u then v; info: 4 ints; status 0 / 1
Result = collections.namedtuple("Result", "col sum max dual info status")


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def words(res):
    """A Result as a tuple of integers: every double as its 64-bit word."""
    return (tuple(res.col), bits(res.sum), bits(res.max), tuple(bits(x) for x in res.dual), tuple(int(x) for x in res.info), int(res.status))


def matrix(kind, n, m, seed):
    """A seeded n x m matrix: "ties" small integers with ties everywhere, "ints" integers up to 1000, "neg" integers in [-50, 50],
    "inf30" / "inf55" integers in [-20, 20] with 30 % / 55 % +inf, "real" uniform doubles, "sqrt2" k1 + k2 sqrt(2)."""
    rng = np.random.default_rng([seed, n, m, KINDS.index(kind)])
    if kind == "ties":
        a = rng.integers(1, 4, (n, m)).astype(np.float64)
    elif kind == "ints":
        a = rng.integers(0, 1001, (n, m)).astype(np.float64)
    elif kind == "neg":
        a = rng.integers(-50, 51, (n, m)).astype(np.float64)
    elif kind in ("inf30", "inf55"):
        a = rng.integers(-20, 21, (n, m)).astype(np.float64)
        a[rng.random((n, m)) < (0.30 if kind == "inf30" else 0.55)] = INF
    elif kind == "real":
        a = rng.random((n, m)) * 97.3 + 0.1
    else:
        a = rng.integers(0, 200, (n, m)) + rng.integers(0, 200, (n, m)) * np.sqrt(2.0)
    return np.ascontiguousarray(a, np.float64)


def product(n, m=None):
    """a[i][j] = (i + 1)(j + 1): row i's tree takes i + 1 steps, n (n + 1) / 2 in all (the most the rule takes at m = n)."""
    m = n if m is None else m
    return np.outer(np.arange(1, n + 1), np.arange(1, m + 1)).astype(np.float64)


def assignment_cost(a, col, right_to_left=False):
    """(the left-to-right float64 sum, the max) of a[i][col[i]] over the rows with col[i] >= 0; (0.0, -inf) for none."""
    xs = [float(a[i][c]) for i, c in enumerate(col) if c >= 0]
    if not xs:
        return 0.0, -INF
    if right_to_left:
        xs = xs[::-1]
    s = xs[0]
    for x in xs[1:]:
        s = s + x
    return s, max(xs)


def _infeasible(n, m, steps_sum, steps_max, row):
    return Result([-1] * n, INF, INF, np.zeros(n + m), [steps_sum, steps_max, row, 0], 1)


def solve(a, mode, largest_on_tie=False, fused_potentials=False, right_to_left=False, ignore_limit=False):
    """The rule, literally (include/pathfit.h).  The four flags switch on the WRONG solvers."""
    n, m = len(a), len(a[0])
    a = [[float(x) for x in row] for row in a]

    def phase(summing, limit):
        u, v, p = [0.0] * n, [0.0] * m, [-1] * m
        t, steps = -INF, 0
        for i in range(n):
            minv, way, used = [INF] * m, [-1] * m, [False] * m
            i0, j0 = i, -1
            while True:
                steps += 1
                for j in range(m):                                    # 1.
                    if used[j]:
                        continue
                    x = a[i0][j]
                    if summing:
                        if x > limit:
                            x = INF
                        cur = x - (u[i0] + v[j]) if fused_potentials else (x - u[i0]) - v[j]
                    else:
                        cur = x
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                delta, j1 = INF, -1                                   # 2.
                for j in range(m):
                    if not used[j] and (minv[j] < delta or (largest_on_tie and minv[j] == delta and minv[j] < INF)):
                        delta, j1 = minv[j], j
                if j1 < 0:
                    return None, i, steps, t
                if summing:                                           # 3.
                    u[i] += delta
                    for j in range(m):
                        if used[j]:
                            u[p[j]] += delta
                            v[j] -= delta
                        else:
                            minv[j] -= delta
                else:
                    t = max(t, delta)
                j0 = j1                                               # 4.
                used[j0] = True
                if p[j0] < 0:
                    break
                i0 = p[j0]
            while j0 >= 0:
                j1 = way[j0]
                p[j0] = i if j1 < 0 else p[j1]
                j0 = j1
        return (u, v, p), -1, steps, t

    steps_sum = steps_max = 0
    limit = INF
    if mode != 0:
        state, row, steps_max, t = phase(False, INF)
        if state is None:
            return _infeasible(n, m, 0, steps_max, row)
        if not ignore_limit:
            limit = t
    if mode != 1:
        state, row, steps_sum, _ = phase(True, limit)
        if state is None:
            return _infeasible(n, m, steps_sum, steps_max, row)
    u, v, p = state
    col = [-1] * n
    for j, r in enumerate(p):
        if r >= 0:
            col[r] = j
    s, mx = assignment_cost(a, col, right_to_left)
    dual = np.zeros(n + m) if mode == 1 else np.array(u + v, np.float64)
    return Result(col, s, mx, dual, [steps_sum, steps_max, -1, 0], 0)


def solve_np(a, mode):
    """The same rule with each tree step's loops over the columns as numpy operations: word for word `solve`'s Result."""
    a = np.ascontiguousarray(a, np.float64)
    n, m = a.shape

    def phase(summing, limit):
        al = np.where(a > limit, INF, a) if summing else a
        u, v, p = np.zeros(n), np.zeros(m), np.full(m, -1, np.int64)
        t, steps = -INF, 0
        for i in range(n):
            minv, way, used = np.full(m, INF), np.full(m, -1, np.int64), np.zeros(m, bool)
            i0, j0 = i, -1
            while True:
                steps += 1
                cur = (al[i0] - u[i0]) - v if summing else al[i0]
                better = ~used & (cur < minv)
                minv[better] = cur[better]
                way[better] = j0
                key = np.where(used, INF, minv)
                j1 = int(np.argmin(key))                              # (the first of the smallest)
                delta = float(key[j1])
                if not delta < INF:
                    return None, i, steps, t
                if summing:
                    u[i] += delta
                    u[p[used]] += delta
                    v[used] -= delta
                    minv[~used] -= delta
                else:
                    t = max(t, delta)
                j0 = j1
                used[j0] = True
                if p[j0] < 0:
                    break
                i0 = int(p[j0])
            while j0 >= 0:
                j1 = int(way[j0])
                p[j0] = i if j1 < 0 else p[j1]
                j0 = j1
        return (u, v, p), -1, steps, t

    steps_sum = steps_max = 0
    limit = INF
    if mode != 0:
        state, row, steps_max, limit = phase(False, INF)
        if state is None:
            return _infeasible(n, m, 0, steps_max, row)
    if mode != 1:
        state, row, steps_sum, _ = phase(True, limit)
        if state is None:
            return _infeasible(n, m, steps_sum, steps_max, row)
    u, v, p = state
    col = np.full(n, -1, np.int64)
    col[p[p >= 0]] = np.flatnonzero(p >= 0)
    s, mx = assignment_cost(a, col)
    dual = np.zeros(n + m) if mode == 1 else np.concatenate([u, v])
    return Result([int(c) for c in col], s, mx, dual, [steps_sum, steps_max, -1, 0], 0)


def brute(a):
    """All injections rows -> columns: (the smallest left-to-right sum, the smallest max, the smallest left-to-right sum among the
    injections with that max); (inf, inf, inf) where none is finite."""
    n, m = len(a), len(a[0])
    a = [[float(x) for x in row] for row in a]
    best_sum, best = INF, (INF, INF)
    for perm in itertools.permutations(range(m), n):
        s = mx = a[0][perm[0]]
        for i in range(1, n):
            x = a[i][perm[i]]
            s = s + x
            mx = max(mx, x)
        if s < INF:
            best_sum = min(best_sum, s)
            best = min(best, (mx, s))
    return best_sum, best[0], best[1]


def certificate(a, res):
    """In exact rationals: (sum of the matched pairs' slack a - u - v) - n min(0, the smallest reduced cost over the finite
    entries).  With v <= 0 and v == 0 on unmatched columns (asserted) it bounds the distance of `res`'s exact total from the exact
    optimum: every assignment costs at least sum u + sum v + n min(0, smallest reduced cost)."""
    n, m = len(a), len(a[0])
    u = [Fraction(float(x)) for x in res.dual[:n]]
    v = [Fraction(float(x)) for x in res.dual[n:]]
    taken = set(res.col)
    assert all(x <= 0 for x in v) and all(v[j] == 0 for j in range(m) if j not in taken)
    low = Fraction(0)
    for i in range(n):
        for j in range(m):
            if a[i][j] < INF:
                low = min(low, Fraction(float(a[i][j])) - u[i] - v[j])
    slack = sum(Fraction(float(a[i][c])) - u[i] - v[c] for i, c in enumerate(res.col))
    return slack - n * low


def greedy_nearest(a):
    """Row by row, the nearest task still free (the smallest column on a tie); -1 where no free task can be reached."""
    n, m = len(a), len(a[0])
    free, out = [True] * m, []
    for i in range(n):
        best, at = INF, -1
        for j in range(m):
            if free[j] and float(a[i][j]) < best:
                best, at = float(a[i][j]), j
        if at >= 0:
            free[at] = False
        out.append(at)
    return out


def wrong_greedy(a, mode):
    """A solver that answers with greedy_nearest's pairing."""
    n, m = len(a), len(a[0])
    col = greedy_nearest(a)
    if min(col) < 0:
        return _infeasible(n, m, 0, 0, col.index(-1))
    s, mx = assignment_cost(a, col)
    return Result(col, s, mx, np.zeros(n + m), [0, 0, -1, 0], 0)


def free_cells(grid, count, seed):
    """`count` distinct free cells of the grid as (r, c) pairs, seeded."""
    g = np.asarray(grid)
    ids = np.flatnonzero(g.reshape(-1) != 1)
    pick = np.random.default_rng(seed).choice(ids, count, replace=False)
    return [(int(v) // g.shape[1], int(v) % g.shape[1]) for v in pick]


# The worst figures test_assign_checkers.py measured on its seeded real-valued cases (it asserts them again): the gap of the rule's
# sum to the brute-force minimum of left-to-right sums, and the exact-rational certificate.
WORST_GAP = 0.0
WORST_CERTIFICATE = 1.2789769243681803e-13                           # ("sqrt2", entries up to 480; "real": 4.97e-14)

# The seeded cases on which each wrong solver differs from the rule: (kind, n, m, mode, seed).
WRONG_LARGEST_ON_TIE = ("ties", 4, 5, 0, 0)
WRONG_FUSED = ("real", 5, 5, 0, 3)
WRONG_RIGHT_TO_LEFT = ("real", 4, 5, 0, 0)
WRONG_IGNORES_LIMIT = ("ints", 4, 5, 2, 0)
WRONG_GREEDY = ("ints", 4, 5, 0, 0)

# The map fact: eight robots and eight tasks on the golden 20 x 20 map whose nearest-task greedy pairing costs more than the optimum
GREEDY_MAP = "fig7"
GREEDY_ROBOTS = [(11, 11), (8, 7), (11, 4), (6, 13), (8, 19), (0, 18), (19, 15), (6, 5)]
GREEDY_TASKS = [(18, 3), (17, 6), (0, 10), (7, 0), (14, 11), (5, 5), (7, 9), (15, 19)]
GREEDY_COST = 73.97056274847715
GREEDY_OPTIMUM = 50.071067811865476
