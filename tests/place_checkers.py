"""CPU checkers for the placement search (pf_place_improve / pathfit.Placement): the rule in its literal loop form, a
numpy form (per slot one [m, n] minimum against the minimum over the other slots, left-to-right sums by cumsum over the finite
terms), the validators, the perturbations and the rounds around it, brute force over all p-subsets, and six deliberately WRONG
solvers that tests/test_place_checkers.py must tell from the rule.  m sites, n demands, p slots; a[i][j] is what demand j pays at
site i, +inf or in [+0.0, 2^1000]; a row holds sites or -1 (an empty slot), the slots below `fixed` never change.  mode 0 "sum":
the key is (unserved, sum); mode 1 "max": (unserved, max, sum).  Doubles are compared as 64-bit words (tour_checkers.bits) by
the tests."""
import itertools

import numpy as np

INF = float("inf")
BIG = 2.0 ** 1000
MODES = (0, 1)
SITES_MAX, DEMANDS_MAX, OPEN_MAX = 1024, 4096, 64
MAX_MOVES = 1 << 20
KINDS = ("euclid", "ints", "tenths", "holes")
WRONG = ("largest_on_tie", "first_improvement", "no_unserved_count", "max_without_sum", "pairwise_sum", "never_fills")


def matrix(kind, m, n, seed):
    """euclid: distances between seeded points of the unit square; ints: 1 .. 3, ties everywhere; tenths: 0.1 .. 0.9; holes:
    euclid with 35 % of the entries +inf."""
    rng = np.random.default_rng([seed, m, n, KINDS.index(kind)])
    if kind == "ints":
        return rng.integers(1, 4, (m, n)).astype(np.float64)
    if kind == "tenths":
        return rng.integers(1, 10, (m, n)) / 10.0
    s, d = rng.random((m, 2)), rng.random((n, 2))
    a = np.sqrt(((s[:, None, :] - d[None, :, :]) ** 2).sum(-1))
    if kind == "holes":
        a[rng.random((m, n)) < 0.35] = INF
    return np.ascontiguousarray(a)


def two_rooms():
    """4 sites, 6 demands: sites 0, 1 reach demands 0 .. 2 only, sites 2, 3 demands 3 .. 5 only."""
    a = np.full((4, 6), INF)
    a[:2, :3] = [[1.0, 2.0, 3.0], [2.0, 1.0, 1.5]]
    a[2:, 3:] = [[4.0, 1.0, 2.0], [1.0, 1.0, 1.25]]
    return a


# ---- the validators
def first_bad_entry(mats):
    """(b, i, j) of the first entry, in flat order, that is neither +inf nor a number in [+0.0, 2^1000] (-0.0 is one); None."""
    a = np.asarray(mats, np.float64)
    a = a.reshape((-1,) + a.shape[-2:])
    with np.errstate(invalid="ignore"):
        ok = ~np.signbit(a) & ((a <= BIG) | (a == INF))
    bad = np.argwhere(~ok)
    return None if not len(bad) else tuple(int(v) for v in bad[0])


def first_bad_row(rows, m, p, fixed):
    """(b, slot) of the first slot that lies outside [-1, m), repeats the site of a smaller slot, or is empty below `fixed`; None."""
    for b, row in enumerate(np.asarray(rows).reshape(-1, p)):
        seen = set()
        for s, v in enumerate(row):
            v = int(v)
            if not -1 <= v < m or v in seen or (v < 0 and s < fixed):
                return b, s
            if v >= 0:
                seen.add(v)
    return None


def valid_row(row, m, p, fixed):
    return len(row) == p and first_bad_row([list(row)], m, p, fixed) is None


# ---- the rule, literally
def near_own(a, sel, j):
    """(near(sel, j), own(sel, j))."""
    best, own = INF, -1
    for s, site in enumerate(sel):
        if site >= 0 and float(a[site][j]) < best:
            best, own = float(a[site][j]), s
    return best, own


def cost(a, sel, pairwise=False):
    """(uns, sum, max): the walk over j = 0 .. n - 1 in order."""
    uns, total, largest, terms = 0, 0.0, 0.0, []
    for j in range(len(a[0])):
        x = near_own(a, sel, j)[0]
        if x == INF:
            uns += 1
        else:
            total = total + x
            largest = x if x > largest else largest
            terms.append(x)
    if pairwise:                                                     # (a WRONG solver's sum)
        while len(terms) > 1:
            terms = [terms[t] + terms[t + 1] if t + 1 < len(terms) else terms[t] for t in range(0, len(terms), 2)]
        total = terms[0] if terms else 0.0
    return uns, total, largest


def key_of(c, mode, wrong=None):
    uns, total, largest = c
    if wrong == "no_unserved_count":
        return (total,) if mode == 0 else (largest, total)
    if wrong == "max_without_sum" and mode == 1:
        return uns, largest
    return (uns, total) if mode == 0 else (uns, largest, total)


def owners(a, sel):
    return [sel[o] if o >= 0 else -1 for o in (near_own(a, sel, j)[1] for j in range(len(a[0])))]


def improve(a, sel, mode, fixed, max_moves, wrong=None, trace=None):
    """The rule's loop -> (row, owner, (sum after, max after, sum before, max before), status, (moves, sweeps, uns after, uns
    before)).  wrong: one of WRONG.  trace: a list that takes (row before, o, i, key of the candidate) per applied move."""
    m, p = len(a), len(sel)
    row = [int(v) for v in sel]
    first = cost(a, row, wrong == "pairwise_sum")
    moves = sweeps = 0
    while True:
        sweeps += 1
        mine = key_of(cost(a, row, wrong == "pairwise_sum"), mode, wrong)
        best = None
        for o in range(fixed, p):
            if wrong == "never_fills" and row[o] < 0 and any(v >= 0 for v in row):
                continue
            for i in range(m):
                if i in row:
                    continue
                k = key_of(cost(a, row[:o] + [i] + row[o + 1:], wrong == "pairwise_sum"), mode, wrong)
                if wrong == "first_improvement":
                    if best is None and k < mine:
                        best = (k, o, i)
                elif best is None or (k, o, i) < best or (wrong == "largest_on_tie" and k == best[0]):
                    best = (k, o, i)
        if best is None or not best[0] < mine:
            status = 0
            break
        if moves == max_moves:
            status = 2
            break
        if trace is not None:
            trace.append((list(row), best[1], best[2], best[0]))
        row[best[1]] = best[2]
        moves += 1
    last = cost(a, row, wrong == "pairwise_sum")
    return row, owners(a, row), (last[1], last[2], first[1], first[2]), status, (moves, sweeps, last[0], first[0])


# ---- the rule in numpy
def cost_numpy(a, sel):
    on = [s for s in sel if s >= 0]
    near = a[on].min(0) if on else np.full(a.shape[1], INF)
    fin = near != INF
    t = np.where(fin, near, 0.0)
    return int((~fin).sum()), float(np.cumsum(t)[-1]), float(t.max())


def sweep_numpy(a, row, mode, fixed):
    """The smallest ((uns, sum, max), o, i) under the key of `mode` over the candidates of a sweep; None with no candidate."""
    m, n = a.shape
    p = len(row)
    free = np.ones(m, bool)
    free[[s for s in row if s >= 0]] = False
    if not free.any():
        return None
    best = None
    for o in range(fixed, p):
        rest = [s for x, s in enumerate(row) if s >= 0 and x != o]
        base = a[rest].min(0) if rest else np.full(n, INF)
        cand = np.minimum(a, base[None, :])
        fin = cand != INF
        t = np.where(fin, cand, 0.0)
        uns, total, largest = (~fin).sum(1), np.cumsum(t, axis=1)[:, -1], t.max(1)
        keys = (uns, total) if mode == 0 else (uns, largest, total)
        live = free.copy()
        for k in keys:                                               # the smallest key, column by column; then the smallest i
            live &= k == k[live].min()
        i = int(np.flatnonzero(live)[0])
        c = (int(uns[i]), float(total[i]), float(largest[i]))
        if best is None or key_of(c, mode) < key_of(best[0], mode):
            best = (c, o, i)
    return best


def improve_numpy(a, sel, mode, fixed, max_moves):
    """improve() over whole rows of the matrix; the applied candidate's cost is the next row's."""
    a = np.ascontiguousarray(a, np.float64)
    row = [int(v) for v in sel]
    first = mine = cost_numpy(a, row)
    moves = sweeps = 0
    while True:
        sweeps += 1
        best = sweep_numpy(a, row, mode, fixed)
        if best is None or not key_of(best[0], mode) < key_of(mine, mode):
            status = 0
            break
        if moves == max_moves:
            status = 2
            break
        row[best[1]] = best[2]
        mine = best[0]
        moves += 1
    on = np.array([s if s >= 0 else 0 for s in row])
    vals = np.where(np.array(row)[:, None] >= 0, a[on], INF)
    own = np.where(vals.min(0) != INF, np.array(row)[vals.argmin(0)], -1)      # (argmin: the first smallest slot)
    return row, [int(v) for v in own], (mine[1], mine[2], first[1], first[2]), status, (moves, sweeps, mine[0], first[0])


def better_candidates(a, row, mode, fixed):
    """Every (o, i) whose row has a key strictly below the row's own, found by rebuilding the rows (an independent look)."""
    mine = key_of(cost(a, list(row)), mode)
    out = []
    for o in range(fixed, len(row)):
        for i in range(len(a)):
            if i not in row:
                new = list(row)
                new[o] = i
                if key_of(cost(a, new), mode) < mine:
                    out.append((o, i))
    return out


def brute_force(a, p, mode, keep=()):
    """The smallest key over all sets of at most p sites that hold `keep` (the cost of a set is that of its ascending row: a
    minimum does not depend on the order of the slots)."""
    m = len(a)
    rest = [i for i in range(m) if i not in keep]
    best = None
    for q in range(0, p - len(keep) + 1):
        for extra in itertools.combinations(rest, q):
            k = key_of(cost(a, list(keep) + list(extra)), mode)
            best = k if best is None or k < best else best
    return best


# ---- the rounds
def key_of_result(got, mode):
    return key_of((int(got[4][2]), float(got[2][0]), float(got[2][1])), mode)


def perturbed(row, fixed, draws):
    """Per draw (s, i): slot fixed + s takes site i if i is not in the row, else the draw is dropped."""
    out = [int(v) for v in row]
    for s, i in draws:
        if int(i) not in out:
            out[fixed + int(s)] = int(i)
    return out


def perturbations(rng, row, fixed, m, starts):
    """`starts` perturbed rows: ONE rng.integers(0, [p - f, m], (starts, Q, 2)) draw, Q = max(1, (p - f) // 4)."""
    p = len(row)
    draws = rng.integers(0, [p - fixed, m], (starts, max(1, (p - fixed) // 4), 2))
    return [perturbed(row, fixed, draws[s]) for s in range(starts)]


def search(a, p, mode, keep=(), starts=8, rounds=3, seed=0, max_moves=None, solver=None):
    """Round 0 improves [keep..., -1, ...]; each later round improves `starts` perturbations of the incumbent and keeps the
    strictly smallest key at the smallest start index -> dict(row, owner, total, radius, unserved, history, moves)."""
    solver = improve_numpy if solver is None else solver
    a = np.ascontiguousarray(a, np.float64)
    f = len(keep)
    limit = 16 * p if max_moves is None else max_moves
    got = solver(a, [int(v) for v in keep] + [-1] * (p - f), mode, f, limit)
    best, moves = got, int(got[4][0])
    history = [key_of_result(got, mode)]
    rng = np.random.default_rng(seed)
    for _ in range(rounds if p > f else 0):
        for row in perturbations(rng, best[0], f, len(a), starts):
            got = solver(a, row, mode, f, limit)
            moves += int(got[4][0])
            if key_of_result(got, mode) < key_of_result(best, mode):      # (in start order: the first smallest of the round wins)
                best = got
        history.append(key_of_result(best, mode))
    return dict(row=list(best[0]), owner=list(best[1]), total=float(best[2][0]), radius=float(best[2][1]), unserved=int(best[4][2]), history=history,
                moves=moves)


# ---- the map case the GPU file leans on: every free cell of the golden 20 x 20 map is a site and a demand
MAP_NAME, MAP_COUNT = "fig7", 4
MAP_SEARCH = dict(starts=4, rounds=2, seed=3)


def map_cells(g):
    return [(int(r), int(c)) for r, c in np.argwhere(np.asarray(g) != 1)]


# ---- the seeded cases that tell each WRONG solver from the rule: (kind, m, n, p, seed, mode), from the empty row
WRONG_CASES = {"largest_on_tie": ("euclid", 6, 8, 2, 0, 0), "first_improvement": ("euclid", 7, 9, 3, 0, 1), "no_unserved_count": ("euclid", 6, 8, 2, 0, 0),
               "max_without_sum": ("euclid", 9, 12, 4, 0, 1), "pairwise_sum": ("euclid", 7, 9, 3, 0, 0), "never_fills": ("euclid", 6, 8, 2, 0, 0)}
