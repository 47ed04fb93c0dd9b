"""CPU checkers for the min-max fleet routes (pf_fleet_balance / pathfit.FleetTours(objective="makespan")): the rule
of include/pathfit.h in its literal loop form and in a vectorised numpy form, the rounds around it, brute force over all partitions
and orders, an independent look at a local optimum, and six deliberately WRONG solvers that tests/test_fleet_balance_checkers.py
must tell from the rule.  Rows, weights, nxt, END, capacities, the candidate families and delta / rem / add are fleet_checkers'
(pf_fleet_improve's); what is new is the price span' of a candidate under the lengths len[0 .. k - 1] the rule carries."""
import itertools

import numpy as np

import fleet_checkers as fl

INF = fl.INF
CARRIES = ("incremental", "recomputed")                               # how len is carried between sweeps; the rule is "incremental"


def _not_searched(N, k):
    return [-1] * N, [INF] * k, (INF, INF, INF, INF), 1, (0, 0, 0, 0, 0)


def others_max(lens, skip):
    """The largest length over the robots outside `skip`; -inf where there is none."""
    top = -INF
    for r, x in enumerate(lens):
        if r not in skip and x > top:
            top = x
    return top


def top_three(lens, last_on_tie=False):
    """The three largest lengths with their robots, largest first: [(value, robot)] padded with (-inf, -1).  Among equal lengths the
    smallest robot comes first (the largest with `last_on_tie`: the pick below may not depend on it)."""
    order = sorted(range(len(lens)), key=lambda r: (-lens[r], -r if last_on_tie else r))[:3]
    return [(lens[r], r) for r in order] + [(-INF, -1)] * (3 - len(order))


def pick(top, skip):
    """others_max from the top three: the first of them whose robot is outside `skip` (at most two robots)."""
    for value, r in top:
        if r not in skip:
            return value
    return -INF


def candidates(w, o, k, mode, cap):
    """Every admissible candidate of one sweep over the row o, in ascending (family code, i, j): (delta, (rem, add, inner), code, i, j,
    s, d) with s = rob(i) and d = rob(j); the triple is None for a 2-opt.  delta, rem and add are fleet_checkers.candidates'; inner is
    the length of the segment's own L - 1 legs, which changes routes with it: +0.0, w(s1, s2) or fl(w(s1, s2) + w(s2, s3))."""
    N = len(o)
    rob, cnt = fl.structure(o, k)

    def wt(x, y):
        return 0.0 if (y < 0 or x == y) else float(w[x][y])

    def nxt(p):
        return o[p + 1] if p + 1 < N and o[p + 1] >= k else (rob[p] if mode == 1 else -1)

    for i in range(1, N):
        for j in range(i + 1, N):
            if all(o[p] >= k for p in range(i, j + 1)):
                a, b, c, e = o[i - 1], o[i], o[j], nxt(j)
                yield (wt(a, c) + wt(b, e)) - (wt(a, b) + wt(c, e)), None, 0, i, j, rob[i], rob[i]
    for L in fl.SEGMENTS:
        for i in range(1, N - L + 1):
            if not all(o[p] >= k for p in range(i, i + L)):
                continue
            for j in range(N):
                if not (j < i - 1 or j > i + L - 1):
                    continue
                if not (rob[j] == rob[i] or cap is None or cnt[rob[j]] + L <= int(cap[rob[j]])):
                    continue
                a, s1, sL, b, p, q = o[i - 1], o[i], o[i + L - 1], nxt(i + L - 1), o[j], nxt(j)
                rem = (wt(a, s1) + wt(sL, b)) - wt(a, b)
                add = (wt(p, s1) + wt(sL, q)) - wt(p, q)
                inner = 0.0 if L == 1 else (wt(s1, o[i + 1]) if L == 2 else wt(s1, o[i + 1]) + wt(o[i + 1], sL))
                yield add - rem, (rem, add, inner), L, i, j, rob[i], rob[j]


def priced(lens, top, delta, parts, s, d, old_max=False, add_as_delta=False, no_inner=False):
    """-> (span', the new lengths as {robot: length})."""
    if s == d:
        new = {s: lens[s] + delta}
    else:
        rem, add, inner = parts
        inner = 0.0 if no_inner else inner
        new = {s: (lens[s] - rem) - inner, d: lens[d] + delta if add_as_delta else (lens[d] + add) + inner}
    span = max(lens) if old_max else pick(top, tuple(new))
    if not old_max:
        for x in new.values():
            span = x if x > span else span
    return span, new


def balance(d, route, k, mode, cap, max_moves, carry="incremental", delta_first=False, accept_equal=False, old_max=False, largest_on_tie=False,
            add_as_delta=False, no_inner=False, last_robot_on_tie=False, trace=None):
    """The rule, literally -> (route list, len list, (makespan after, total after, makespan before, total before), status, (moves,
    sweeps, 2-opt moves, relocate moves, moves that lowered the span)).  carry: "incremental" (the rule: the applied candidate's
    len' become len) or "recomputed" (len summed left to right from the row before every sweep: the form that walks in circles).
    The six flags switch on the WRONG solvers: the key (delta, span'), acceptance on span' <= span alone, the maximum over all
    robots' old lengths, the largest (i, j) on a tie, len'[d] = fl(len[d] + delta), and the segment's inner legs left behind
    (len'[s] = fl(len[s] - rem), len'[d] = fl(len[d] + add) for every L).  last_robot_on_tie changes the robot the top three
    name among equal lengths: it must change nothing.  `trace` (a list) takes (span', delta, code, i, j, row before, row after)."""
    N = len(route)
    if np.isinf(np.asarray(d, np.float64)[fl.readable(k, N)]).any():
        return _not_searched(N, k)
    w = fl.mirror(d)
    o = [int(v) for v in route]
    lens, total0, span0 = fl.lengths(w, o, k, mode)
    lens = list(lens)
    moves = sweeps = m2 = mr = low = 0
    while True:
        sweeps += 1
        if carry == "recomputed":
            lens = list(fl.lengths(w, o, k, mode)[0])
        span = max(lens)
        top = top_three(lens, last_robot_on_tie)
        best = None
        for delta, parts, code, i, j, s, dd in candidates(w, o, k, mode, cap):
            sp, new = priced(lens, top, delta, parts, s, dd, old_max, add_as_delta, no_inner)
            assert old_max or sp == max(max(new.values()), others_max(lens, tuple(new)))      # the pick among three is the maximum
            key = ((delta, sp) if delta_first else (sp, delta)) + (code, -i if largest_on_tie else i, -j if largest_on_tie else j)
            if best is None or key < best[0]:
                best = (key, sp, delta, code, i, j, new)
        if best is None:
            status = 0
            break
        _, sp, delta, code, i, j, new = best
        if not (sp < span or (sp == span and (accept_equal or delta < 0))):
            status = 0
            break
        if moves == max_moves:
            status = 2
            break
        was = list(o)
        if code == 0:
            o[i:j + 1] = o[i:j + 1][::-1]
            m2 += 1
        else:
            o = fl.relocated(o, code, i, j)
            mr += 1
        moves += 1
        low += sp < span
        for r, x in new.items():
            lens[r] = x
        if trace is not None:
            trace.append((sp, delta, code, i, j, was, list(o)))
    out, total, span = fl.lengths(w, o, k, mode)
    return o, out, (span, total, span0, total0), status, (moves, sweeps, m2, mr, low)


def balance_numpy(d, route, k, mode, cap, max_moves, carry="incremental"):
    """The rule in numpy: all prices of a sweep at once, family by family in ascending (i, j) -> balance's tuple.  (The candidates
    that are none are computed and masked: what the unread entries hold may not warn.)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return _balance_numpy(d, route, k, mode, cap, max_moves, carry)


def _balance_numpy(d, route, k, mode, cap, max_moves, carry):
    N = len(route)
    d = np.asarray(d, np.float64)
    if np.isinf(d[fl.readable(k, N)]).any():
        return _not_searched(N, k)
    wm = fl.mirror(d)
    w = np.zeros((N + 1, N + 1))
    w[:N, :N] = wm                                                    # (row and column N: "none"; the diagonal is +0.0)
    o = np.array([int(v) for v in route], np.int64)
    capv = None if cap is None else np.array([int(c) for c in cap], np.int64)
    pos = np.arange(N)
    I, J = pos[:, None], pos[None, :]                                 # a table's cell [i, j]: row-major order is ascending (i, j)
    lens, total0, span0 = fl.lengths(wm, o, k, mode)
    lens = np.array(lens, np.float64)
    moves = sweeps = m2 = mr = low = 0
    status = 0
    while True:
        sweeps += 1
        if carry == "recomputed":
            lens = np.array(fl.lengths(wm, o, k, mode)[0], np.float64)
        span = float(lens.max())
        # the largest length outside one robot [k] and outside two [k, k]
        out1, out2 = _outside_one(lens), _outside_two(lens)
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
        ok = task[:, None] & task[None, :] & same & (I < J)
        delta = (np.roll(A, 1, axis=0) + C) - (np.roll(leg, 1)[:, None] + leg[None, :])
        tables = [(0, ok, delta, np.maximum(lens[rob][:, None] + delta, out1[rob][:, None]))]
        for L in fl.SEGMENTS:
            last = np.minimum(pos + L - 1, N - 1)
            seg = task & (pos + L - 1 < N) & task[last] & (rob == rob[last]) & (pos >= 1)
            rem = (np.roll(leg, 1) + leg[last]) - w[np.roll(o, 1), nx[last]]
            ok = seg[:, None] & ((J < I - 1) | (J > I + L - 1))
            if capv is not None:
                ok = ok & (same | (cnt[rob] + L <= capv[rob])[None, :])
            add = (A.T + C[last]) - leg[None, :]
            delta = add - rem[:, None]
            inner = _inner(leg, pos, N, L)
            inside = np.maximum(lens[rob][:, None] + delta, out1[rob][:, None])
            across = np.maximum(np.maximum(((lens[rob] - rem) - inner)[:, None], (lens[rob][None, :] + add) + inner[:, None]), out2[rob[:, None], rob[None, :]])
            tables.append((L, ok, delta, np.where(same, inside, across)))
        found = []                                                    # per family (its smallest (span', delta), code, i, j), the first smallest
        for code, ok, delta, price in tables:
            if ok.any():
                p = np.where(ok, price, INF)
                at = ok & (p == p.min())
                x = int(np.argmin(np.where(at, delta, INF)))
                found.append((float(p.reshape(-1)[x]), float(delta.reshape(-1)[x]), code, x // N, x % N))
        best = min(found) if found else None
        if best is None or not (best[0] < span or (best[0] == span and best[1] < 0)):
            break
        if moves == max_moves:
            status = 2
            break
        sp, dl, code, i, j = best
        s, dd = int(rob[i]), int(rob[j])
        if code and s != dd:                                          # the two lengths of the applied candidate, by the rule's lines
            last = i + code - 1
            rem = (leg[i - 1] + leg[last]) - w[o[i - 1], nx[last]]
            add = (w[o[j], o[i]] + w[o[last], nx[j]]) - leg[j]
            inner = _inner(leg, pos, N, code)[i]
            lens[s], lens[dd] = (lens[s] - rem) - inner, (lens[dd] + add) + inner
        else:
            lens[s] = lens[s] + dl
        if code == 0:
            o[i:j + 1] = o[i:j + 1][::-1].copy()
            m2 += 1
        else:
            o = np.array(fl.relocated([int(v) for v in o], code, i, j), np.int64)
            mr += 1
        moves += 1
        low += sp < span
    out = [int(v) for v in o]
    lens, total, span = fl.lengths(wm, out, k, mode)
    return out, lens, (span, total, span0, total0), status, (moves, sweeps, m2, mr, low)


def _inner(leg, pos, N, L):
    """Per position i the length of the inner legs of the segment i .. i + L - 1 (where it is one: its legs are the row's)."""
    if L == 1:
        return np.zeros(N)
    first = leg[np.minimum(pos, N - 1)]
    return first if L == 2 else first + leg[np.minimum(pos + 1, N - 1)]


def _outside_one(lens):
    order = np.argsort(-lens, kind="stable")
    out = np.full(len(lens), lens[order[0]])
    out[order[0]] = lens[order[1]] if len(lens) > 1 else -INF
    return out


def _outside_two(lens):
    """out[s, d] = the largest length over the robots other than s and d (-inf where there is none): a pick among the top three."""
    k = len(lens)
    order = np.argsort(-lens, kind="stable")[:3]
    vals = np.append(lens[order], [-INF] * (3 - len(order)))
    who = np.append(order, [-1] * (3 - len(order)))
    S, D = np.arange(k)[:, None], np.arange(k)[None, :]
    hit = [(S == who[x]) | (D == who[x]) for x in range(3)]
    return np.where(~hit[0], vals[0], np.where(~hit[1], vals[1], np.where(~hit[2], vals[2], -INF)))


def key_of(w, row, k, mode):
    """(makespan, total) summed from the row itself."""
    _, total, span = fl.lengths(w, row, k, mode)
    return span, total


def improving_candidates(d, route, k, mode, cap):
    """An independent look at a local optimum: the moves whose row, built by slicing, is valid and has a smaller (makespan, total)
    than the row it came from, both summed from the rows themselves (smaller by more than the roundings of a sum: 1e-9)."""
    w = fl.mirror(d)
    o = [int(v) for v in route]
    N = len(o)
    span, total = key_of(w, o, k, mode)
    found = []

    def look(row, what):
        if fl.valid_row(row, k, N, cap):
            s2, t2 = key_of(w, row, k, mode)
            if s2 - span < -1e-9 or (abs(s2 - span) <= 1e-9 and t2 - total < -1e-9):
                found.append(what)

    for i in range(1, N):
        for j in range(i + 1, N):
            if all(v >= k for v in o[i:j + 1]):
                look(o[:i] + o[i:j + 1][::-1] + o[j + 1:], (0, i, j))
    for L in fl.SEGMENTS:
        for i in range(1, N - L + 1):
            if all(v >= k for v in o[i:i + L]):
                for j in range(N):
                    if j < i - 1 or j > i + L - 1:
                        look(fl.relocated(o, L, i, j), (L, i, j))
    return found


def brute_force(d, k, mode, cap=None):
    """The smallest makespan over all partitions of the tasks among the robots within the caps and all orders of every route."""
    w = fl.mirror(d)
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
                low = min(low, fl.lengths(w, fl.row_of(lists), k, mode)[0][r])
            best[key] = low
        return best[key]

    low = INF
    for owner in itertools.product(range(k), repeat=len(tasks)):
        parts = [tuple(t for t, r in zip(tasks, owner) if r == x) for x in range(k)]
        if cap is not None and any(len(parts[r]) > int(cap[r]) for r in range(k)):
            continue
        low = min(low, max(route_best(r, parts[r]) for r in range(k)))
    return low


def search(d, k, mode, cap=None, starts=8, rounds=3, seed=0, max_moves=None, improver=fl.improve_numpy, solver=balance_numpy):
    """FleetTours(objective="makespan")'s search over one matrix -> dict(route, routes, lengths, total, makespan, feasible,
    start_total, start_makespan, history, total_history, moves): round 0 improves the start row with the sum rule, then balances
    it; every later round balances `starts` perturbations of the incumbent and keeps the strictly smallest (makespan, total) at
    the smallest start index."""
    N = len(d)
    limit = 16 * N if max_moves is None else max_moves
    w = fl.mirror(d)
    start = fl.start_row(w, k, cap)
    o, _, val, st, info = improver(d, start, k, mode, cap, limit)
    if st == 1:
        return dict(route=[-1] * N, routes=[[] for _ in range(k)], lengths=[INF] * k, total=INF, makespan=INF, feasible=False, start_total=INF,
                    start_makespan=INF, history=[INF], total_history=[INF], moves=0)
    moves = info[0]
    o, lens, v, _, info = solver(d, o, k, mode, cap, limit)
    moves += info[0]
    best = (v[0], v[1])
    hist, totals = [best[0]], [best[1]]
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        for cand in fl.perturbations(rng, o, k, cap, starts):
            o2, l2, v2, _, i2 = solver(d, cand, k, mode, cap, limit)
            moves += i2[0]
            if (v2[0], v2[1]) < best:
                best, o, lens = (v2[0], v2[1]), o2, l2                # (the later starts perturb nothing: the round's were drawn)
        hist.append(best[0])
        totals.append(best[1])
    return dict(route=o, routes=[[t - k for t in tasks] for tasks in fl.split(o, k)], lengths=lens, total=best[1], makespan=best[0], feasible=True,
                start_total=val[1], start_makespan=fl.lengths(w, start, k, mode)[2], history=hist, total_history=totals, moves=moves)


def capped_runs(carry, kinds=("euclid", "ints", "tenths"), ks=(1, 2, 3, 5), ns=(1, 2, 5, 9, 20), seeds=range(6)):
    """The seeded set of DESIGN.md 4.32: per kind the number of runs from random_row that end at the cap of 16 N moves, of
    len(ks) len(ns) 2 len(seeds) each."""
    out = {}
    for kind in kinds:
        count = 0
        for k, n, mode, seed in itertools.product(ks, ns, fl.MODES, seeds):
            N = k + n
            count += balance_numpy(fl.matrix(kind, N, seed), fl.random_row(k, n, seed), k, mode, None, 16 * N, carry)[3] == 2
        out[kind] = count
    return out


# The capped runs of the seeded set (240 runs a kind) under the rule, which carries len incrementally, and under the form that sums
# len again from the row before every sweep.  tests/test_fleet_balance_checkers.py counts both again.  (Without the inner legs of
# a relocated segment in len' -- the wrong solver `no_inner` -- the counts were 0 / 0 / 10 and 59 / 25 / 47: circles on integers.)
CAPPED_INCREMENTAL = {"euclid": 0, "ints": 0, "tenths": 7}
CAPPED_RECOMPUTED = {"euclid": 0, "ints": 0, "tenths": 13}

# What the searches reach on fleet_checkers' map (MAP, MAP_ROBOTS, MAP_TASKS, MAP_SEARCH) per mode: (makespan, total) of the sum
# search and of the min-max search, and the latter's routes.
MAP_SUM = {0: (22.071067811865476, 46.14213562373095), 1: (64.97056274847714, 64.97056274847714)}
MAP_BALANCED = {0: (19.65685424949238, 48.55634918610404), 1: (29.071067811865476, 77.21320343559643)}
MAP_BALANCED_ROUTES = {0: [[1, 10, 11], [0, 5, 3, 2, 7], [6, 9, 8, 4]], 1: [[1, 10, 11], [0, 5, 3, 2, 7], [6, 9, 4, 8]]}

# The seeded cases on which each wrong solver differs from the rule: (kind, k, n, mode, seed) of fleet_checkers.matrix, the start
# random_row's.
WRONG_DELTA_FIRST = ("ints", 2, 2, 1, 2)
WRONG_ACCEPT_EQUAL = ("ints", 2, 2, 0, 0)
WRONG_OLD_MAX = ("ints", 2, 2, 0, 2)
WRONG_LARGEST_ON_TIE = ("ints", 2, 3, 0, 2)
WRONG_ADD_AS_DELTA = ("ints", 2, 2, 0, 0)
WRONG_NO_INNER = ("ints", 2, 5, 0, 3)                                 # its second move keeps (makespan, total) = (4, 6) as summed from the rows
