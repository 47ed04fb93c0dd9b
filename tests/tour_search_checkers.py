"""CPU checkers for the tour search (pf_tour_improve / pathfit.TourSearch): the 2-opt rule in its literal loop form,
a vectorised numpy form, the rounds of perturbed restarts around it, and four deliberately WRONG solvers that
tests/test_tour_search_checkers.py must tell from the rule.  Nodes are 0..n - 1, node 0 the start; mode 0 open, 1 return, 2 last.
Only the upper triangle of a matrix is read.  Doubles are compared as 64-bit words (tour_checkers.bits)."""
import numpy as np

import tour_checkers as tc

INF = float("inf")
BIG = 2.0 ** 1000
MODES = (0, 1, 2)
MAX_N = 1024
MAX_MOVES = 1 << 20


def hi_of(n, mode):
    """The last movable position."""
    return n - 2 if mode == 2 else n - 1


def mirror(d):
    """The weights the rule reads: the upper triangle on both sides, the diagonal +0.0 (w(x, x) is never a leg but for n == 1)."""
    d = np.asarray(d, np.float64)
    u = np.triu(d, 1)
    return u + u.T


def upper(d):
    d = np.asarray(d, np.float64)
    return d[np.triu_indices(d.shape[0], 1)]


def first_bad_entry(mats):
    """(b, i, j) of the first upper-triangle entry that is NaN, negative or finite above 2^1000, in flat order; None."""
    m = np.asarray(mats, np.float64)
    n = m.shape[-1]
    m = m.reshape(-1, n, n)
    with np.errstate(invalid="ignore"):
        ok = (m >= 0.0) & ((m <= BIG) | (m == INF))
    ok |= ~np.triu(np.ones((n, n), bool), 1)[None]
    bad = np.argwhere(~ok)
    return None if not len(bad) else tuple(int(v) for v in bad[0])


def first_bad_start(orders, n, mode):
    """(b, position) of the first position whose node lies outside [0, n), repeats the node of a smaller position or breaks a
    fixed end; None."""
    for b, row in enumerate(np.asarray(orders).reshape(-1, n)):
        seen = set()
        for p, v in enumerate(row):
            v = int(v)
            if not 0 <= v < n or v in seen or (p == 0 and v != 0) or (mode == 2 and p == n - 1 and v != n - 1):
                return b, p
            seen.add(v)
    return None


def total(w, order, mode):
    """The left-to-right sum of the n legs w(order[k], order[k + 1]), the last one the closing leg in mode 1 and +0.0 otherwise."""
    n = len(order)
    seq = [int(v) for v in order] + [int(order[0]) if mode == 1 else -1]
    legs = [0.0 if (b < 0 or a == b) else float(w[a][b]) for a, b in zip(seq[:-1], seq[1:])]
    t = legs[0]
    for x in legs[1:n]:
        t = t + x
    return t


def _not_searched(n):
    return [-1] * n, (INF, INF), 1, (0, 0, 0, 0)


def two_opt(d, order, mode, max_moves, largest_on_tie=False, first_improvement=False, other_sum=False, skip_last=False):
    """The rule, literally -> (order list, (total after, total before), status, (moves, sweeps, 0, 0)).  The four flags switch on the
    WRONG solvers: the largest (i, j) on a tie, the first improving pair, (w(a,c) - w(a,b)) + (w(b,e) - w(c,e)), and no pair with
    j = n - 1 in mode 0."""
    n = len(order)
    if np.isinf(upper(d)).any():
        return _not_searched(n)
    w = mirror(d)
    o = [int(v) for v in order]
    hi = hi_of(n, mode)

    def wt(x, y):
        return 0.0 if y < 0 else float(w[x][y])

    before = total(w, o, mode)
    moves = sweeps = 0
    while True:
        sweeps += 1
        seq = o + [o[0] if mode == 1 else -1]
        best, arg = None, None
        for i in range(1, hi + 1):
            for j in range(i + 1, hi + 1):
                if skip_last and mode == 0 and j == n - 1:
                    continue
                a, b, c, e = seq[i - 1], seq[i], seq[j], seq[j + 1]
                if other_sum:
                    delta = (wt(a, c) - wt(a, b)) + (wt(b, e) - wt(c, e))
                else:
                    delta = (wt(a, c) + wt(b, e)) - (wt(a, b) + wt(c, e))
                if first_improvement:
                    if delta < 0 and best is None:
                        best, arg = delta, (i, j)
                elif best is None or delta < best or (largest_on_tie and delta == best):
                    best, arg = delta, (i, j)
        if best is None or not best < 0:
            status = 0
            break
        if moves == max_moves:
            status = 2
            break
        i, j = arg
        o[i:j + 1] = o[i:j + 1][::-1]
        moves += 1
    return o, (total(w, o, mode), before), status, (moves, sweeps, 0, 0)


def two_opt_numpy(d, order, mode, max_moves):
    """The rule in numpy: all deltas of a sweep at once, in ascending (i, j), argmin the first smallest -> two_opt's tuple."""
    n = len(order)
    if np.isinf(upper(d)).any():
        return _not_searched(n)
    w = np.zeros((n + 1, n + 1))
    w[:n, :n] = mirror(d)                                             # (row and column n: "none")
    o = np.array([int(v) for v in order] + [0], np.int64)
    hi = hi_of(n, mode)
    I, J = np.triu_indices(hi + 1, 1)
    keep = I >= 1
    I, J = I[keep], J[keep]
    o[n] = o[0] if mode == 1 else n
    before = total(w, o[:n], mode)
    moves = sweeps = 0
    while True:
        sweeps += 1
        status = 0
        if len(I):
            a, b, c, e = o[I - 1], o[I], o[J], o[J + 1]
            delta = (w[a, c] + w[b, e]) - (w[a, b] + w[c, e])
            k = int(np.argmin(delta))
            if delta[k] < 0:
                if moves == max_moves:
                    status = 2
                    break
                i, j = int(I[k]), int(J[k])
                o[i:j + 1] = o[i:j + 1][::-1].copy()
                moves += 1
                continue
        break
    out = [int(v) for v in o[:n]]
    return out, (total(w, out, mode), before), status, (moves, sweeps, 0, 0)


def improving_pairs(d, order, mode):
    """An independent look at a local optimum: the pairs (i, j) whose reversal shortens the sum of the (up to) two changed legs,
    recomputed from the edges themselves."""
    w = mirror(d)
    n = len(order)
    o = [int(v) for v in order]
    hi = hi_of(n, mode)
    nxt = o + [o[0] if mode == 1 else None]
    out = []
    for i in range(1, hi + 1):
        for j in range(i + 1, hi + 1):
            old = w[nxt[i - 1]][nxt[i]] + (0.0 if nxt[j + 1] is None else w[nxt[j]][nxt[j + 1]])
            new = w[nxt[i - 1]][nxt[j]] + (0.0 if nxt[j + 1] is None else w[nxt[i]][nxt[j + 1]])
            if new - old < 0:
                out.append((i, j))
    return out


def double_bridge(o, cuts):
    a, b, d = (int(v) for v in cuts)
    o = [int(v) for v in o]
    return o[:a] + o[b:d] + o[a:b] + o[d:]


def perturbations(rng, o, hi, starts):
    """`starts` double-bridge perturbations of o: the cuts a < b < d are three different positions of 1 .. hi + 1."""
    return [double_bridge(o, np.sort(rng.choice(np.arange(1, hi + 2), 3, replace=False))) for _ in range(starts)]


def search(d, mode, starts=32, rounds=8, seed=0, max_moves=None, improve=two_opt_numpy):
    """TourSearch's search over one matrix -> dict(order, total, feasible, start_total, history, moves): round 0 improves the
    nearest-neighbour order over the mirrored matrix, every later round improves `starts` perturbations of the incumbent and keeps
    the strictly smallest total at the smallest start index."""
    n = len(d)
    cap = 16 * n if max_moves is None else max_moves
    w = mirror(d)
    nn = tc.nearest_neighbour(w, mode)[:n]                            # (n = 1 in mode 2: node 0 is the start and the end)
    o, val, st, info = improve(d, nn, mode, cap)
    if st == 1:
        return dict(order=[-1] * n, total=INF, feasible=False, start_total=INF, history=[INF], moves=0)
    best, hist, moves = val[0], [val[0]], info[0]
    hi = hi_of(n, mode)
    rng = np.random.default_rng(seed)
    if hi >= 3:
        for _ in range(rounds):
            for cand in perturbations(rng, o, hi, starts):
                o2, v2, _, i2 = improve(d, cand, mode, cap)
                moves += i2[0]
                if v2[0] < best:
                    best, o = v2[0], o2                               # (the later starts perturb nothing: the round's were drawn)
            hist.append(best)
    return dict(order=o, total=best, feasible=True, start_total=val[1], history=hist, moves=moves)


def matrix(kind, n, seed):
    """tour_checkers.matrix, and "tenths": multiples of 0.1 in [0.1, 0.9], where sums that tie as real numbers differ by roundings."""
    if kind != "tenths":
        return tc.matrix(kind, n, seed)
    return np.random.default_rng([seed, n]).integers(1, 10, (n, n)).astype(np.float64) / 10.0


# Twenty-four free cells of the golden 20 x 20 map "fig7" (tour_checkers.free_cells(grid, 24, 2)) on which, under the default policy,
# end="open" and MAP_SEARCH, the nearest-neighbour order's total, its 2-opt optimum and the total after the rounds are three
# different numbers (test_tour_search_checkers.py derives them with a heap Dijkstra; the GPU file confirms them against the device).
MAP = "fig7"
MAP_STOPS = [(5, 4), (3, 11), (15, 16), (11, 5), (8, 18), (2, 16), (1, 7), (1, 11), (4, 15), (15, 18), (14, 8), (8, 0), (13, 8), (19, 7), (0, 17), (6, 4),
             (16, 0), (5, 9), (6, 12), (3, 19), (11, 11), (17, 7), (11, 18), (5, 7)]
MAP_SEARCH = dict(starts=8, rounds=3, seed=0)
MAP_NN_TOTAL = 100.69848480983498
MAP_TWO_OPT_TOTAL = 98.45584412271569
MAP_ROUNDS_TOTAL = 98.0416305603426

# The seeded cases on which each wrong solver differs from the rule: (kind, n, mode, seed) of `matrix`, the start the
# nearest-neighbour order over the mirrored matrix.
WRONG_LARGEST_ON_TIE = ("ints", 8, 1, 2)
WRONG_FIRST_IMPROVEMENT = ("uniform", 5, 2, 5)
WRONG_OTHER_SUM = ("tenths", 5, 0, 8)
WRONG_SKIP_LAST = ("euclid", 6, 0, 2)
