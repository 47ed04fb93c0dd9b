"""CPU model of the space-time fields (pf_spacetime_stamp / _field / _paths / _conflicts), written from the rule
and sharing no code with the device.  tests/test_spacetime_checkers.py pins it on any host; the GPU tests compare the device
against it, word for word.

Time runs in ticks 0..T.  S is the static occupancy (bool [R, C]), D the dynamic planes (bool [T + 1, R, C]), A[t] = S | D[t].  A
robot at u at tick t may be at v at tick t + 1 iff
  1. v is inside the grid and A[t + 1][v] == 0                                              (vertex)
  2. v == u, or u -> v is a straight step, or a diagonal one when allow_diag                (shape)
  3. for a move, not both D[t][v] and D[t + 1][u]                                           (swap / pass-through)
  4. for a diagonal move under restrict_corner, (v.r, u.c) and (u.r, v.c) are clear in A[t] | A[t + 1]   (corner)
Cells are flat ids r * C + c; moves are in helper.py:30-36 order."""
import numpy as np

DR = (0, 0, 1, -1, 1, 1, -1, -1)
DC = (1, -1, 0, 0, 1, -1, 1, -1)
POLICIES = ((1, 1), (1, 0), (0, 1), (0, 0))                            # (allow_diag, restrict_corner)
STATIC, VERTEX, SWAP, CORNER = 1, 2, 3, 4
ST_OK, ST_INFEASIBLE, ST_OVERFLOW = 0, 1, 3


# ---------------------------------------------------------------------------------------------------- planes
def pack(bits):
    """bool [..., R, C] -> uint64 [..., R, Wc]: cell (r, c) is bit c & 63 of word (r, c >> 6); the bits at c >= C are 0."""
    bits = np.asarray(bits, bool)
    C = bits.shape[-1]
    Wc = (C + 63) // 64
    pad = np.zeros(bits.shape[:-1] + (Wc * 64,), np.uint8)
    pad[..., :C] = bits
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).view("<u8").astype(np.uint64)


def unpack(words, C):
    """The inverse of pack (every bit of the words, the columns cut at C)."""
    w = np.ascontiguousarray(np.asarray(words, np.uint64).astype("<u8"))
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :C].astype(bool)


def bad_row(row, t0, T, RC, cap=None):
    row = list(row)
    return len(row) < 1 or (cap is not None and len(row) > cap) or not 0 <= t0 <= T or any(not 0 <= int(v) < RC for v in row)


def planes(shape, T, obstacles, start_ticks=None, after_end="stay", corners=False, into=None):
    """The stamp: obstacle i occupies obstacles[i][j] at tick start_ticks[i] + j; after_end == "stay": its last cell to tick T;
    corners: a unit diagonal step over t -> t + 1 also takes its two orthogonal corner cells at t and t + 1.  Ticks beyond T are
    dropped; a bad row (empty, a cell outside the grid, a start tick outside [0, T]) stamps nothing.  -> (bool [T + 1, R, C],
    status per row); `into` is ORed into and returned."""
    R, C = shape
    D = np.zeros((T + 1, R, C), bool) if into is None else into
    status = []
    for i, row in enumerate(obstacles):
        row = [int(v) for v in row]
        t0 = 0 if start_ticks is None else int(start_ticks[i])
        if bad_row(row, t0, T, R * C):
            status.append(1)
            continue
        status.append(0)
        for j, v in enumerate(row):
            t = t0 + j
            if t > T:
                break
            D[t, v // C, v % C] = True
            if corners and j + 1 < len(row):
                x = row[j + 1]
                if abs(x // C - v // C) == 1 and abs(x % C - v % C) == 1:
                    for tt in (t, t + 1):
                        if tt <= T:
                            D[tt, x // C, v % C] = True
                            D[tt, v // C, x % C] = True
        if after_end == "stay":
            v = row[-1]
            D[min(t0 + len(row), T + 1):, v // C, v % C] = True
    return D, np.array(status, np.int32)


# ---------------------------------------------------------------------------------------------------- the rule, literally
def may(S, D, t, u, v, ad, rs):
    """May a robot at cell u at tick t be at cell v at tick t + 1?  (Both inside the grid.)"""
    R, C = S.shape
    ur, uc, vr, vc = u // C, u % C, v // C, v % C
    if S[vr, vc] or D[t + 1, vr, vc]:
        return False
    dr, dc = vr - ur, vc - uc
    if dr == 0 and dc == 0:
        return True
    if max(abs(dr), abs(dc)) != 1:
        return False
    diag = dr != 0 and dc != 0
    if diag and not ad:
        return False
    if D[t, vr, vc] and D[t + 1, ur, uc]:
        return False
    if diag and rs:
        for (r, c) in ((vr, uc), (ur, vc)):
            if S[r, c] or D[t, r, c] or D[t + 1, r, c]:
                return False
    return True


def field(S, D, sources, ad, rs, swap_rule=True, corner_both=True):
    """Cell by cell -> (arrive int32 [R, C], reach bool [T + 1, R, C]).  swap_rule=False and corner_both=False are the two BROKEN
    solvers the checker's own test must tell from the model: no rule 3; rule 4 against A[t + 1] only."""
    S = np.asarray(S, bool)
    R, C = S.shape
    T = D.shape[0] - 1
    reach = np.zeros((T + 1, R, C), bool)
    for s in sources:
        s = int(s)
        if not (S[s // C, s % C] or D[0, s // C, s % C]):
            reach[0, s // C, s % C] = True
    Dm = D if swap_rule else np.zeros_like(D)
    for t in range(T):
        for u in np.flatnonzero(reach[t].reshape(-1)):
            u = int(u)
            ur, uc = u // C, u % C
            for k in range(-1, 8 if ad else 4):
                vr, vc = (ur, uc) if k < 0 else (ur + DR[k], uc + DC[k])
                if not (0 <= vr < R and 0 <= vc < C) or reach[t + 1, vr, vc]:
                    continue
                if swap_rule and corner_both:
                    ok = may(S, D, t, u, vr * C + vc, ad, rs)
                else:
                    ok = not (S[vr, vc] or D[t + 1, vr, vc])
                    if ok and k >= 0 and Dm[t, vr, vc] and Dm[t + 1, ur, uc]:
                        ok = False
                    if ok and k >= 4 and rs:
                        for (r, c) in ((vr, uc), (ur, vc)):
                            if S[r, c] or D[t + 1, r, c] or (corner_both and D[t, r, c]):
                                ok = False
                if ok:
                    reach[t + 1, vr, vc] = True
    return arrival_of(reach), reach


def arrival_of(reach):
    """arrive[v] = the least t with reach[t][v], -1 if none."""
    any_t = reach.any(axis=0)
    return np.where(any_t, reach.argmax(axis=0), -1).astype(np.int32)


def info_of(arrive):
    """{cells reached, the largest arrival tick, the smallest cell id that attains it, 0}; {0, -1, -1, 0} when nothing is reached."""
    a = np.asarray(arrive).reshape(-1)
    n = int((a >= 0).sum())
    if n == 0:
        return np.array([0, -1, -1, 0], np.int64)
    return np.array([n, int(a.max()), int(np.flatnonzero(a == a.max())[0]), 0], np.int64)


# ---------------------------------------------------------------------------------------------------- the rule, 64 cells a word
_ONE, _63 = np.uint64(1), np.uint64(63)


def _from_left(X):                 # bit c <- the row's cell c - 1
    out = X << _ONE
    out[:, 1:] |= X[:, :-1] >> _63
    return out


def _from_right(X):                # bit c <- the row's cell c + 1
    out = X >> _ONE
    out[:, :-1] |= X[:, 1:] << _63
    return out


def _from_above(X):                # row r <- row r - 1
    out = np.zeros_like(X)
    out[1:] = X[:-1]
    return out


def _from_below(X):
    out = np.zeros_like(X)
    out[:-1] = X[1:]
    return out


def field_words(S, Dw, sources, ad, rs, want_reach=True):
    """The same field on packed planes (Dw uint64 [T + 1, R, Wc], S bool [R, C]), 64 cells a word -> (arrive int32 [R, C], reach
    words uint64 [T + 1, R, Wc] or None).  Written independently of field(): shifts and carries, no cell is looked at alone."""
    S = np.asarray(S, bool)
    R, C = S.shape
    Sw = pack(S)
    T = Dw.shape[0] - 1
    valid = pack(np.ones((R, C), bool))
    cur = np.zeros_like(Sw)
    for s in sources:
        s = int(s)
        cur[s // C, (s % C) >> 6] |= _ONE << np.uint64((s % C) & 63)
    cur &= ~(Sw | Dw[0])
    out = np.zeros((T + 1,) + Sw.shape, np.uint64) if want_reach else None
    arrive = np.full((R, C), -1, np.int32)
    seen = cur.copy()
    arrive[unpack(cur, C)] = 0
    if want_reach:
        out[0] = cur
    horiz = ((_from_left, 1), (_from_right, -1))
    vert = ((_from_above, 1), (_from_below, -1))
    for t in range(T):
        d0, d1 = Dw[t], Dw[t + 1]
        nxt = cur.copy()
        for f, _ in horiz + vert:
            nxt |= f(cur) & ~(d0 & f(d1))
        if ad:
            x = Sw | d0 | d1
            for fv, _ in vert:
                for fh, _ in horiz:
                    m = fv(fh(cur)) & ~(d0 & fv(fh(d1)))
                    if rs:
                        m &= ~(fh(x) | fv(x))
                    nxt |= m
        nxt &= ~(Sw | d1) & valid
        fresh = nxt & ~seen
        if fresh.any():
            arrive[unpack(fresh, C)] = t + 1
            seen |= fresh
        if want_reach:
            out[t + 1] = nxt
        cur = nxt
    return arrive, out


# ---------------------------------------------------------------------------------------------------- routes
def hold_tick(reach, D, v):
    """The least t with reach[t][v] and D[t'][v] == 0 for every t <= t' <= T; -1 if none."""
    C = D.shape[2]
    r, c = v // C, v % C
    T = D.shape[0] - 1
    first = T + 1
    for t in range(T, -1, -1):
        if D[t, r, c]:
            break
        first = t
    for t in range(first, T + 1):
        if reach[t, r, c]:
            return t
    return -1


def trace(S, D, reach, target, tick, ad, rs):
    """The route rule: from (tick, target) back; at (t, v) the first u with reach[t - 1][u] and u -> v allowed among v - step(d),
    d = 0..7, then the wait.  -> the cells at ticks 0..tick, or None where some tick has no predecessor."""
    S = np.asarray(S, bool)
    R, C = S.shape
    v = int(target)
    out = [v]
    for t in range(tick, 0, -1):
        vr, vc = v // C, v % C
        for k in list(range(8 if ad else 4)) + [-1]:
            ur, uc = (vr, vc) if k < 0 else (vr - DR[k], vc - DC[k])
            if 0 <= ur < R and 0 <= uc < C and reach[t - 1, ur, uc] and may(S, D, t - 1, ur * C + uc, v, ad, rs):
                v = ur * C + uc
                break
        else:
            return None
        out.append(v)
    return out[::-1]


def route(S, D, reach, target, tick, ad, rs, cap=None):
    """pf_spacetime_paths for one query: tick -1 the earliest arrival, -2 the hold tick -> (cells or None, status, tick used)."""
    R, C = np.asarray(S).shape
    T = D.shape[0] - 1
    if not 0 <= target < R * C or tick < -2 or tick > T:
        return None, ST_INFEASIBLE, -1
    r, c = target // C, target % C
    if tick == -1:
        ts = np.flatnonzero(reach[:, r, c])
        tick = int(ts[0]) if len(ts) else -1
    elif tick == -2:
        tick = hold_tick(reach, D, target)
    elif not reach[tick, r, c]:
        tick = -1
    if tick < 0:
        return None, ST_INFEASIBLE, -1
    if cap is not None and tick + 1 > cap:
        return None, ST_OVERFLOW, tick
    cells = trace(S, D, reach, target, tick, ad, rs)
    return (cells, ST_OK, tick) if cells is not None else (None, ST_OVERFLOW, tick)


# ---------------------------------------------------------------------------------------------------- conflicts
def step_kind(S, D, t, u, v, ad, rs):
    """The kind of the step u -> v over t -> t + 1 by precedence (0: none)."""
    R, C = S.shape
    ur, uc, vr, vc = u // C, u % C, v // C, v % C
    if S[vr, vc]:
        return STATIC
    dr, dc = vr - ur, vc - uc
    wait, diag = dr == 0 and dc == 0, dr != 0 and dc != 0
    if not wait and (max(abs(dr), abs(dc)) != 1 or (diag and not ad)):
        return STATIC
    if diag and rs and (S[vr, uc] or S[ur, vc]):
        return STATIC
    if D[t + 1, vr, vc]:
        return VERTEX
    if not wait and D[t, vr, vc] and D[t + 1, ur, uc]:
        return SWAP
    if diag and rs and (D[t, vr, uc] or D[t + 1, vr, uc] or D[t, ur, vc] or D[t + 1, ur, vc]):
        return CORNER
    return 0


def conflicts(S, D, row, t0, ad, rs, hold=False, cap=None):
    """-> ((first conflicting tick or -1, its kind, the cell entered or -1, conflicting steps), status): the row's first cell as a
    vertex at t0 (kind 1 on a static obstacle), step t -> t + 1 at tick t + 1; hold: the last cell at every later tick up to T.
    status 1: a bad row; 2: the row runs past T (checked up to T, no hold check)."""
    S = np.asarray(S, bool)
    R, C = S.shape
    T = D.shape[0] - 1
    row = [int(v) for v in row]
    if bad_row(row, t0, T, R * C, cap):
        return (-1, 0, -1, 0), 1
    found = []
    past = t0 + len(row) - 1 > T
    for j, v in enumerate(row):
        t = t0 + j
        if t > T:
            break
        if j == 0:
            kind = STATIC if S[v // C, v % C] else (VERTEX if D[t, v // C, v % C] else 0)
        else:
            kind = step_kind(S, D, t - 1, row[j - 1], v, ad, rs)
        if kind:
            found.append((t, kind, v))
    if hold and not past:
        v = row[-1]
        found += [(t, VERTEX, v) for t in range(t0 + len(row), T + 1) if D[t, v // C, v % C]]
    first = found[0] if found else (-1, 0, -1)
    return first + (len(found),), 2 if past else 0


# ---------------------------------------------------------------------------------------------------- fleets
def fleet(S, T, starts, goals, ad, rs, order=None, corners=None, D=None):
    """Prioritised planning: each robot in order takes the arrival field from its start against the planes so far and the route to
    its goal at the hold tick, which is then stamped with after_end "stay" and corners = restrict_corner (or `corners`).  A robot
    without a hold tick gets None and is not stamped.  -> (routes, status per robot, the planes)."""
    S = np.asarray(S, bool)
    R, C = S.shape
    D = np.zeros((T + 1, R, C), bool) if D is None else D.copy()
    corners = bool(rs) if corners is None else bool(corners)
    n = len(starts)
    routes, status = [None] * n, np.full(n, ST_INFEASIBLE, np.int32)
    for i in (range(n) if order is None else order):
        _, rw = field_words(S, pack(D), [starts[i]], ad, rs)
        reach = unpack(rw, C)
        cells, st, _ = route(S, D, reach, int(goals[i]), -2, ad, rs)
        status[i] = st
        if cells is not None:
            routes[i] = cells
            planes((R, C), T, [cells], None, "stay", corners, into=D)
    return routes, status, D


def fleet_violations(routes, T, C, rs):
    """(shared cells, swaps, corner cases, robots checked) among the planned robots, each parked on its last cell to tick T: two
    robots on one cell at a tick; two robots that exchange cells over a tick; under restrict_corner a diagonal step with another
    robot on a corner cell at either tick."""
    pos = {i: [r[min(t, len(r) - 1)] for t in range(T + 1)] for i, r in enumerate(routes) if r is not None}
    shared = swaps = corner = 0
    for i in pos:
        for j in pos:
            if i == j:
                continue
            for t in range(T + 1):
                if i < j and pos[i][t] == pos[j][t]:
                    shared += 1
                if t < T and i < j and pos[i][t] != pos[i][t + 1] and pos[i][t] == pos[j][t + 1] and pos[i][t + 1] == pos[j][t]:
                    swaps += 1
                if t < T and rs:
                    u, v = pos[i][t], pos[i][t + 1]
                    if abs(v // C - u // C) == 1 and abs(v % C - u % C) == 1:
                        cs = ((v // C) * C + u % C, (u // C) * C + v % C)
                        if pos[j][t] in cs or pos[j][t + 1] in cs:
                            corner += 1
    return shared, swaps, corner, len(pos)
