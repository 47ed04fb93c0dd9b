"""CPU checkers for the fleet routes (pf_fleet_improve / pathfit.FleetTours): the rule in its literal loop form, a
vectorised numpy form, the start rule, the perturbations and the rounds around it, brute force over all partitions and orders,
and six deliberately WRONG solvers that tests/test_fleet_checkers.py must tell from the rule.  k robots (nodes 0 .. k - 1), n
tasks (nodes k .. N - 1), N = k + n; mode 0 open, 1 return.  A row is a permutation of the nodes that begins with node 0 and holds
the robots in increasing order: the tasks behind robot r's marker are its route.  Only the upper triangle of a matrix is read, the
robot-robot entries never.  Doubles are compared as 64-bit words (tour_checkers.bits) by the tests."""
import itertools

import numpy as np

import tour_search_checkers as ts

INF = float("inf")
BIG = 2.0 ** 1000
MODES = (0, 1)
MAX_N = 1024
MAX_MOVES = 1 << 20
SEGMENTS = (1, 2, 3)                                                 # the family codes of the relocations: the segment's length
PERTURB_MOVES = 3                                                    # the relocations drawn per perturbed start

mirror = ts.mirror


def readable(k, N):
    """The entries the rule reads: i < j with j a task."""
    m = np.triu(np.ones((N, N), bool), 1)
    m[:, :k] = False
    return m


def first_bad_entry(mats, k):
    """(b, i, j) of the first readable entry that is NaN, negative or finite above 2^1000, in flat order; None."""
    m = np.asarray(mats, np.float64)
    N = m.shape[-1]
    m = m.reshape(-1, N, N)
    with np.errstate(invalid="ignore"):
        ok = (m >= 0.0) & ((m <= BIG) | (m == INF))
    ok |= ~readable(k, N)[None]
    bad = np.argwhere(~ok)
    return None if not len(bad) else tuple(int(v) for v in bad[0])


def first_bad_row(routes, k, N):
    """(b, position) of the first position whose node lies outside [0, N), repeats the node of a smaller position, is not node 0
    at position 0, or is a robot r >= 1 that robot r - 1 does not stand in front of; None."""
    for b, row in enumerate(np.asarray(routes).reshape(-1, N)):
        seen = set()
        for p, v in enumerate(row):
            v = int(v)
            if not 0 <= v < N or v in seen or (p == 0 and v != 0) or (1 <= v < k and v - 1 not in seen):
                return b, p
            seen.add(v)
    return None


def first_over_cap(routes, k, N, cap):
    """(b, robot) of the first robot with more tasks than its capacity; None."""
    if cap is None:
        return None
    for b, row in enumerate(np.asarray(routes).reshape(-1, N)):
        cnt = structure(row, k)[1]
        for r in range(k):
            if cnt[r] > int(cap[r]):
                return b, r
    return None


def valid_row(route, k, N, cap=None):
    return first_bad_row([list(route)], k, N) is None and first_over_cap([list(route)], k, N, cap) is None


def structure(route, k):
    """rob per position, cnt per robot."""
    rob, cnt, r = [], [0] * k, -1
    for v in route:
        if int(v) < k:
            r += 1
        else:
            cnt[r] += 1
        rob.append(r)
    return rob, cnt


def split(route, k):
    """The row -> one list of task NODES per robot."""
    out = [[] for _ in range(k)]
    r = -1
    for v in route:
        if int(v) < k:
            r += 1
        else:
            out[r].append(int(v))
    return out


def row_of(lists):
    """One list of task nodes per robot -> the row."""
    out = []
    for r, tasks in enumerate(lists):
        out += [r] + [int(v) for v in tasks]
    return out


def lengths(w, route, k, mode):
    """len per robot: the left-to-right sum of its legs from its marker on, the END leg last (+0.0 in mode 0, the leg back to the
    robot's own node in mode 1; an empty route is the one leg w(r, END) = +0.0) -> (len list, total, makespan)."""
    lens = []
    for r, tasks in enumerate(split(route, k)):
        seq = [r] + tasks
        legs = [float(w[a][b]) for a, b in zip(seq[:-1], seq[1:])] + [float(w[seq[-1]][r]) if mode == 1 and seq[-1] != r else 0.0]
        t = legs[0]
        for x in legs[1:]:
            t = t + x
        lens.append(t)
    total = lens[0]
    for x in lens[1:]:
        total = total + x
    return lens, total, max(lens)


def _not_searched(N, k):
    return [-1] * N, [INF] * k, (INF, INF, INF), 1, (0, 0, 0, 0)


def relocated(o, L, i, j):
    """The segment at positions i .. i + L - 1 taken out and put back, in the same direction, directly behind position j's node."""
    seg = o[i:i + L]
    if j < i:
        return o[:j + 1] + seg + o[j + 1:i] + o[i + L:]
    return o[:i] + o[i + L:j + 1] + seg + o[j + 1:]


def candidates(w, o, k, mode, cap, other_sum=False, ignore_caps=False, no_markers=False):
    """Every admissible candidate of one sweep over the row o, in ascending (family code, i, j): (delta, code, i, j)."""
    N = len(o)
    rob, cnt = structure(o, k)

    def wt(x, y):
        return 0.0 if (y < 0 or x == y) else float(w[x][y])

    def nxt(p):
        return o[p + 1] if p + 1 < N and o[p + 1] >= k else (rob[p] if mode == 1 else -1)

    for i in range(1, N):
        for j in range(i + 1, N):
            if all(o[p] >= k for p in range(i, j + 1)):
                a, b, c, e = o[i - 1], o[i], o[j], nxt(j)
                yield (wt(a, c) + wt(b, e)) - (wt(a, b) + wt(c, e)), 0, i, j
    for L in SEGMENTS:
        for i in range(1, N - L + 1):
            if not all(o[p] >= k for p in range(i, i + L)):
                continue
            for j in range(N):
                if not (j < i - 1 or j > i + L - 1) or (no_markers and o[j] < k):
                    continue
                if not (rob[j] == rob[i] or cap is None or ignore_caps or cnt[rob[j]] + L <= int(cap[rob[j]])):
                    continue
                a, s1, sL, b, p, q = o[i - 1], o[i], o[i + L - 1], nxt(i + L - 1), o[j], nxt(j)
                if other_sum:
                    delta = ((wt(p, s1) + wt(sL, q)) + wt(a, b)) - ((wt(a, s1) + wt(sL, b)) + wt(p, q))
                else:
                    rem = (wt(a, s1) + wt(sL, b)) - wt(a, b)
                    add = (wt(p, s1) + wt(sL, q)) - wt(p, q)
                    delta = add - rem
                yield delta, L, i, j


def improve(d, route, k, mode, cap, max_moves, largest_on_tie=False, relocate_first=False, first_improvement=False, other_sum=False,
            ignore_caps=False, no_markers=False, trace=None):
    """The rule, literally -> (route list, len list, (total after, total before, makespan after), status, (moves, sweeps, 2-opt
    moves, relocate moves)).  The six flags switch on the WRONG solvers: the largest (i, j) on a tie, relocations preferred to
    2-opt on a tie, the first improving candidate, the relocate delta in another association, capacities ignored, and no marker as
    an insertion position.  `trace` (a list) takes (delta, code, i, j, total before the move, total after it) per move."""
    N = len(route)
    if np.isinf(np.asarray(d, np.float64)[readable(k, N)]).any():
        return _not_searched(N, k)
    w = mirror(d)
    o = [int(v) for v in route]
    before = lengths(w, o, k, mode)[1]
    moves = sweeps = m2 = mr = 0
    while True:
        sweeps += 1
        best = None
        for delta, code, i, j in candidates(w, o, k, mode, cap, other_sum, ignore_caps, no_markers):
            if first_improvement:
                if delta < 0 and best is None:
                    best = (delta, code, i, j)
                continue
            key = (delta, (code or 4) if relocate_first else code, -i if largest_on_tie else i, -j if largest_on_tie else j)
            if best is None or key < best[0]:
                best = (key, delta, code, i, j)
        if best is not None and not first_improvement:
            best = best[1:]
        if best is None or not best[0] < 0:
            status = 0
            break
        if moves == max_moves:
            status = 2
            break
        delta, code, i, j = best
        was = lengths(w, o, k, mode)[1]
        if code == 0:
            o[i:j + 1] = o[i:j + 1][::-1]
            m2 += 1
        else:
            o = relocated(o, code, i, j)
            mr += 1
        moves += 1
        if trace is not None:
            trace.append((delta, code, i, j, was, lengths(w, o, k, mode)[1]))
    lens, total, span = lengths(w, o, k, mode)
    return o, lens, (total, before, span), status, (moves, sweeps, m2, mr)


def improve_numpy(d, route, k, mode, cap, max_moves):
    """The rule in numpy: all deltas of a sweep at once, family by family in ascending (i, j), argmin the first smallest ->
    improve's tuple.  (The candidates that are none are computed and masked: what the unread entries hold may not warn.)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return _improve_numpy(d, route, k, mode, cap, max_moves)


def _improve_numpy(d, route, k, mode, cap, max_moves):
    N = len(route)
    d = np.asarray(d, np.float64)
    if np.isinf(d[readable(k, N)]).any():
        return _not_searched(N, k)
    wm = mirror(d)
    w = np.zeros((N + 1, N + 1))
    w[:N, :N] = wm                                                    # (row and column N: "none"; the diagonal is +0.0)
    o = np.array([int(v) for v in route], np.int64)
    capv = None if cap is None else np.array([int(c) for c in cap], np.int64)
    pos = np.arange(N)
    I, J = pos[:, None], pos[None, :]                                 # a table's cell [i, j]: row-major order is ascending (i, j)
    before = lengths(wm, o, k, mode)[1]
    moves = sweeps = m2 = mr = 0
    status = 0
    while True:
        sweeps += 1
        task = o >= k
        rob = np.cumsum(~task) - 1
        cnt = np.bincount(rob[task], minlength=k)
        nx = np.full(N, N, np.int64) if mode == 0 else rob.copy()
        follow = np.append(task[1:], False)
        nx[follow] = o[1:][follow[:-1]]
        leg = w[o, nx]
        A = w[np.ix_(o, o)]                                           # A[x, y] = w(route[x], route[y])
        C = w[np.ix_(o, nx)]                                          # C[x, y] = w(route[x], nxt(y))
        same = rob[:, None] == rob[None, :]
        found = []                                                    # per family (its smallest delta, code, i, j), the first smallest
        ok = task[:, None] & task[None, :] & same & (I < J)
        delta = (np.roll(A, 1, axis=0) + C) - (np.roll(leg, 1)[:, None] + leg[None, :])
        tables = [(0, ok, delta)]
        for L in SEGMENTS:
            last = np.minimum(pos + L - 1, N - 1)
            seg = task & (pos + L - 1 < N) & task[last] & (rob == rob[last]) & (pos >= 1)
            rem = (np.roll(leg, 1) + leg[last]) - w[np.roll(o, 1), nx[last]]
            ok = seg[:, None] & ((J < I - 1) | (J > I + L - 1))
            if capv is not None:
                ok = ok & (same | (cnt[rob] + L <= capv[rob])[None, :])
            tables.append((L, ok, ((A.T + C[last]) - leg[None, :]) - rem[:, None]))
        for code, ok, delta in tables:
            if ok.any():
                x = int(np.argmin(np.where(ok, delta, INF)))
                found.append((float(delta.reshape(-1)[x]), code, x // N, x % N))
        best = min(found, key=lambda t: (t[0], t[1])) if found else None
        if best is None or not best[0] < 0:
            break
        if moves == max_moves:
            status = 2
            break
        _, code, i, j = best
        if code == 0:
            o[i:j + 1] = o[i:j + 1][::-1].copy()
            m2 += 1
        else:
            o = np.array(relocated([int(v) for v in o], code, i, j), np.int64)
            mr += 1
        moves += 1
    out = [int(v) for v in o]
    lens, total, span = lengths(wm, out, k, mode)
    return out, lens, (total, before, span), status, (moves, sweeps, m2, mr)


def improving_candidates(d, route, k, mode, cap):
    """An independent look at a local optimum: the moves whose row, built by slicing, is valid and has a smaller total than the row
    it came from, both totals summed from the rows themselves (smaller by more than the roundings of a sum: 1e-9)."""
    w = mirror(d)
    o = [int(v) for v in route]
    N = len(o)
    here = lengths(w, o, k, mode)[1]
    found = []

    def look(row, what):
        if valid_row(row, k, N, cap) and lengths(w, row, k, mode)[1] - here < -1e-9:
            found.append(what)

    for i in range(1, N):
        for j in range(i + 1, N):
            if all(v >= k for v in o[i:j + 1]):
                look(o[:i] + o[i:j + 1][::-1] + o[j + 1:], (0, i, j))
    for L in SEGMENTS:
        for i in range(1, N - L + 1):
            if all(v >= k for v in o[i:i + L]):
                for j in range(N):
                    if j < i - 1 or j > i + L - 1:
                        look(relocated(o, L, i, j), (L, i, j))
    return found


def brute_force(d, k, mode, cap=None):
    """The smallest total over all partitions of the tasks among the robots within the caps and all orders of every route."""
    w = mirror(d)
    N = len(w)
    tasks = list(range(k, N))
    best = {}

    def route_best(r, subset):
        key = (r, subset)
        if key not in best:
            low = INF
            for perm in itertools.permutations(subset):
                lists = [[] for _ in range(k)]
                lists[r] = list(perm)
                low = min(low, lengths(w, row_of(lists), k, mode)[0][r])
            best[key] = low
        return best[key]

    low = INF
    for owner in itertools.product(range(k), repeat=len(tasks)):
        parts = [tuple(t for t, r in zip(tasks, owner) if r == x) for x in range(k)]
        if cap is not None and any(len(parts[r]) > int(cap[r]) for r in range(k)):
            continue
        total = route_best(0, parts[0])
        for r in range(1, k):
            total = total + route_best(r, parts[r])
        low = min(low, total)
    return low


def start_row(w, k, cap=None):
    """FleetTours' start: the tasks in index order, each to the robot with room that has the smallest w(robot, task) (the smallest
    index on a tie); then every route in nearest-neighbour order from its robot (the smallest task on a tie)."""
    N = len(w)
    lists = [[] for _ in range(k)]
    for t in range(k, N):
        room = [r for r in range(k) if cap is None or len(lists[r]) < int(cap[r])]
        lists[min(room, key=lambda r: (float(w[r][t]), r))].append(t)
    for r in range(k):
        left, at, out = lists[r], r, []
        while left:
            at = min(left, key=lambda t: (float(w[at][t]), t))
            out.append(at)
            left.remove(at)
        lists[r] = out
    return row_of(lists)


def perturbed(o, k, cap, draws):
    """One perturbed start: per draw (x, i, j) the relocation of the segment of length x % 3 + 1 at position i behind position j,
    applied where the rule admits it (the segment all tasks of one route, j outside i - 1 .. i + L - 1, room in j's route) and
    dropped otherwise."""
    o = [int(v) for v in o]
    N = len(o)
    for x, i, j in draws:
        L, i, j = int(x) % 3 + 1, int(i), int(j)
        if i < 1 or i + L > N or not all(v >= k for v in o[i:i + L]) or not (j < i - 1 or j > i + L - 1):
            continue
        rob, cnt = structure(o, k)
        if rob[j] != rob[i] and cap is not None and cnt[rob[j]] + L > int(cap[rob[j]]):
            continue
        o = relocated(o, L, i, j)
    return o


def perturbations(rng, o, k, cap, starts):
    """`starts` perturbed starts of o: one rng.integers(0, N, (starts, PERTURB_MOVES, 3)) draw per round."""
    draws = rng.integers(0, len(o), (starts, PERTURB_MOVES, 3))
    return [perturbed(o, k, cap, draws[s]) for s in range(starts)]


def search(d, k, mode, cap=None, starts=8, rounds=3, seed=0, max_moves=None, solver=improve_numpy):
    """FleetTours' search over one matrix -> dict(route, routes, lengths, total, makespan, feasible, start_total, history, moves):
    round 0 improves the start row, every later round improves `starts` perturbations of the incumbent and keeps the strictly
    smallest total at the smallest start index."""
    N = len(d)
    limit = 16 * N if max_moves is None else max_moves
    w = mirror(d)
    o, lens, val, st, info = solver(d, start_row(w, k, cap), k, mode, cap, limit)
    if st == 1:
        return dict(route=[-1] * N, routes=[[] for _ in range(k)], lengths=[INF] * k, total=INF, makespan=INF, feasible=False, start_total=INF,
                    history=[INF], moves=0)
    best, span, hist, moves = val[0], val[2], [val[0]], info[0]
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        for cand in perturbations(rng, o, k, cap, starts):
            o2, l2, v2, _, i2 = solver(d, cand, k, mode, cap, limit)
            moves += i2[0]
            if v2[0] < best:
                best, span, o, lens = v2[0], v2[2], o2, l2             # (the later starts perturb nothing: the round's were drawn)
        hist.append(best)
    return dict(route=o, routes=[[t - k for t in tasks] for tasks in split(o, k)], lengths=lens, total=best, makespan=span, feasible=True,
                start_total=val[1], history=hist, moves=moves)


def matrix(kind, N, seed):
    """tour_search_checkers.matrix, and "holes": symmetric non-dyadic entries with 25 % +inf."""
    if kind != "holes":
        return ts.matrix(kind, N, seed)
    d = ts.matrix("uniform", N, seed)
    d[np.random.default_rng([seed, N, 77]).random((N, N)) < 0.25] = INF
    return d


def random_row(k, n, seed, cap=None):
    """A seeded row: the tasks shuffled and dealt to seeded robots (within the caps), so that routes may be empty."""
    rng = np.random.default_rng([seed, k, n])
    lists = [[] for _ in range(k)]
    for t in rng.permutation(np.arange(k, k + n)):
        room = [r for r in range(k) if cap is None or len(lists[r]) < int(cap[r])]
        lists[int(room[int(rng.integers(0, len(room)))])].append(int(t))
    return row_of(lists)


# Three robots and twelve tasks on the golden 20 x 20 map "fig7" (tour_checkers.free_cells(grid, 15, 6): the first three cells the
# robots) on which, under the default policy, end="open", no capacities and MAP_SEARCH, the start's total, the total after round 0
# and the total after the rounds are three different numbers (test_fleet_checkers.py derives them with a heap Dijkstra; the GPU file
# confirms them against the device).
MAP = "fig7"
MAP_ROBOTS = [(15, 14), (3, 15), (10, 1)]
MAP_TASKS = [(6, 15), (19, 17), (13, 18), (12, 18), (7, 9), (8, 17), (13, 3), (10, 12), (7, 5), (9, 5), (19, 11), (18, 11)]
MAP_SEARCH = dict(starts=8, rounds=3, seed=0)
MAP_START_TOTAL = 54.97056274847714
MAP_ROUND0_TOTAL = 48.55634918610404
MAP_ROUNDS_TOTAL = 46.14213562373095
MAP_ROUTES = [[1, 10, 11], [0, 5, 3, 2], [6, 9, 8, 4, 7]]

# The seeded cases on which each wrong solver differs from the rule: (kind, k, n, mode, seed) of `matrix`, the start random_row's
# (under caps of ceil(n / k) for the capacities; all tasks on robot 0 for the markers: the empty route of robot 1 must be filled).
WRONG_LARGEST_ON_TIE = ("ints", 2, 2, 0, 4)
WRONG_RELOCATE_FIRST = ("ints", 2, 3, 1, 2)
WRONG_FIRST_IMPROVEMENT = ("ints", 2, 3, 0, 1)
WRONG_OTHER_SUM = ("tenths", 2, 4, 0, 5)
WRONG_IGNORE_CAPS = ("ints", 2, 2, 0, 0)
WRONG_NO_MARKERS = ("ints", 2, 2, 0, 1)
