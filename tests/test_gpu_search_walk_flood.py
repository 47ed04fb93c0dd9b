"""The two parts of astar() (pf_astar.h) that are not the pop loop: the parent walk, which fetches the records of a straight run
together, and the pocket flood, which takes up to 64 queue cells a round.  Neither may change an answer, so every search below is
compared with oracle/pf_oracle bit for bit: cells, length, status and, wherever the open list runs, pops and pushes.

Walk    straight runs of 63, 64, 65 and 199 cells (a round holds 63) along all eight moves: 1 x 200 and 200 x 1 corridors and the
        diagonals of an empty 70 x 70 map (69 cells at most there); such a run ends exactly at the start, and the lanes behind it
        lie outside the grid.  A staircase corridor whose runs are 1 - 3 cells.  An L whose first run, followed blindly, leaves
        the grid at the border (four rotations).  Every case in a row of exactly its length (status 0) and in a row one cell
        shorter (status 3, length 0, the canary rows around it untouched).  An MPA rebuild, whose second leg is emitted at an
        offset into its row, the same two ways.
Flood   pockets of 1, 7, 8, 9, 63, 64, 65, 511, 512 and 513 free cells around the target, and around the start: sealed by obstacles
        (the components answer those), and sealed by an avoid wall on an obstacle-free map (only the flood can answer those; MPA
        variant and closed-set variant).  Up to 512 cells the answer is "no path" with no pop at all; 513 cells are one too many
        for the flood, the open list runs and the reference's pops and pushes come back.  The goal just outside a 512-cell pocket:
        the flood has to see it behind the 512 cells it may claim.

The closed-set variants run on the sequential loop (astar_settle 0): its counters are the reference's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = -7777
OVERFLOW = 3
_WORLD = {}


def world(name, make):
    """(engine, oracle, map) -- one per map and test: an engine holds gigabytes of search scratch, so none outlives its test."""
    if name not in _WORLD:
        from pathfit.engine import Engine
        import pf_oracle as po
        g = np.ascontiguousarray(make(), np.uint8)
        e = Engine(g)
        e.set_option("astar_settle", 0)
        _WORLD[name] = (e, po.Oracle(g), g)
    return _WORLD[name]


@pytest.fixture(autouse=True)
def _close_engines():
    yield
    for e, _, _ in _WORLD.values():
        e.set_option("astar_settle", -1)
        e.close()
    _WORLD.clear()


def assert_search(e, o, variant, s, t, avoid, where, expect_path=None, no_pops=False):
    """One search against the oracle: cells, length, status; pops and pushes too unless the answer must come without the open list."""
    want, ost = o.astar(s, t, avoid, variant)
    paths, st, cnt = e.astar_host(variant, [s], [t], None if avoid is None else [avoid], path_cap=e.R * e.C, want_counters=True)
    tag = (where, variant, s, t)
    assert st[0] == ost[5], (tag, st[0], ost[5])
    assert len(paths[0]) == len(want) and np.array_equal(paths[0], want), tag
    if expect_path is not None:
        assert (len(want) > 0) == expect_path, tag
    if no_pops:
        assert cnt[0, 0] == 0 and cnt[0, 1] == 0, (tag, cnt[0])
    else:
        assert (cnt[0, 0], cnt[0, 1]) == (ost[0], ost[1]), (tag, cnt[0], ost)
    return want


class Rows:
    """n output rows of `cap` cells with a guard row before and after, and the same for the length and status columns."""

    def __init__(self, e, n, cap):
        self.e, self.n, self.cap = e, n, cap
        self.cells = e.put(np.full((n + 2, cap), CANARY, np.int32))
        self.len = e.put(np.full(n + 2, CANARY, np.int32))
        self.status = e.put(np.full(n + 2, CANARY, np.int32))

    def ptrs(self):
        return self.cells.at(self.cap), self.len.at(1), self.status.at(1)

    def read(self):
        c, l, s = self.cells.download(), self.len.download(), self.status.download()
        for a in (c, l, s):
            assert (a[0] == CANARY).all() and (a[-1] == CANARY).all(), "a guard row was written"
        return c[1:-1], l[1:-1], s[1:-1]


def assert_exact_fit(e, variant, s, t, want, where):
    """The search between two one-cell searches, in rows of len(want) cells and of one cell fewer."""
    L = len(want)
    assert L >= 2
    ds, dt = e.put(np.array([s, s, t], np.int32)), e.put(np.array([s, t, t], np.int32))
    for cap in (L, L - 1):
        rows = Rows(e, 3, cap)
        pc, pl, ps = rows.ptrs()
        e._ck(e.L.pf_astar_batch(e.h, variant, 1, 1, 3, ds.ptr, dt.ptr, None, None, cap, pc, pl, ps, None))
        c, l, st = rows.read()
        for a, cell in ((0, s), (2, t)):
            assert st[a] == 0 and l[a] == 1 and c[a, 0] == cell and (c[a, 1:] == CANARY).all(), (where, "neighbour row", a)
        if cap == L:
            assert st[1] == 0 and l[1] == L and np.array_equal(c[1], want), (where, cap, st[1], l[1])
        else:
            assert st[1] == OVERFLOW and l[1] == 0, (where, cap, st[1], l[1])
        assert e.counters()["overflow_agents"] == (0 if cap == L else 1)


# ------------------------------------------------------------------ walk
def straight_cases():
    """(map name, maker, start, target, cells of the path): every one of the eight moves as a single run."""
    cases = []
    for n in (63, 64, 65, 199):
        cases += [("row200", lambda: np.zeros((1, 200)), 0, n - 1, n), ("row200", lambda: np.zeros((1, 200)), 199, 200 - n, n),
                  ("col200", lambda: np.zeros((200, 1)), 0, n - 1, n), ("col200", lambda: np.zeros((200, 1)), 199, 200 - n, n)]
    for n in (63, 64, 65, 70):
        k = n - 1
        cases += [("empty70", lambda: np.zeros((70, 70)), 0, k * 70 + k, n), ("empty70", lambda: np.zeros((70, 70)), 69 * 70 + 69, (69 - k) * 70 + (69 - k), n),
                  ("empty70", lambda: np.zeros((70, 70)), 69, k * 70 + (69 - k), n), ("empty70", lambda: np.zeros((70, 70)), 69 * 70, (69 - k) * 70 + k, n)]
    return cases


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_straight_runs_equal_oracle(variant):
    for name, make, s, t, n in straight_cases():
        e, o, g = world(name, make)
        want = assert_search(e, o, variant, s, t, None, name, expect_path=True)
        assert len(want) == n and len(set(np.diff(want).tolist())) == 1, (name, s, t)      # one run, start to target
        assert_exact_fit(e, variant, s, t, want, (name, s, t))


def staircase():
    """A corridor one cell wide from the top left to the bottom right whose stretches are 1, 2 and 3 cells, everything else
    obstacle.  -> (map, cells of the corridor in order)"""
    n = 48
    g = np.ones((n, n), np.uint8)
    r = c = 0
    cells = [(0, 0)]
    k = 0
    while True:
        step = (1, 2, 3, 2, 1, 3)[k % 6]
        dr, dc = ((0, 1), (1, 0))[k % 2]
        if r + dr * step >= n or c + dc * step >= n:
            break
        for _ in range(step):
            r, c = r + dr, c + dc
            cells.append((r, c))
        k += 1
    for rr, cc in cells:
        g[rr, cc] = 0
    return g, [rr * n + cc for rr, cc in cells]


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_staircase_equals_oracle(variant):
    e, o, g = world("staircase", lambda: staircase()[0])
    cells = staircase()[1]
    for s, t in ((cells[0], cells[-1]), (cells[-1], cells[0]), (cells[3], cells[-2])):
        want = assert_search(e, o, variant, s, t, None, "staircase", expect_path=True)
        d = np.diff(want)
        runs = np.diff(np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1], [True]))))
        assert len(want) > 40 and runs.max() <= 3 and runs.min() == 1
        assert_exact_fit(e, variant, s, t, want, ("staircase", s, t))


def ell(rot):
    """An L of free cells in a 30 x 30 block of obstacles: along row 0 and down column 20.  Walking back from the foot, the first
    run points at the border and the cells behind the corner lie outside the grid."""
    g = np.ones((30, 30), np.uint8)
    g[0, :21] = 0
    g[:26, 20] = 0
    mark = np.zeros((30, 30), np.int32)
    mark[0, 0], mark[25, 20] = 1, 2
    g, mark = np.rot90(g, rot), np.rot90(mark, rot)
    return np.ascontiguousarray(g), int(np.flatnonzero(mark.reshape(-1) == 1)[0]), int(np.flatnonzero(mark.reshape(-1) == 2)[0])


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_run_into_the_border_equals_oracle(variant):
    for rot in range(4):
        e, o, g = world("ell%d" % rot, lambda: ell(rot)[0])
        _, a, b = ell(rot)
        for s, t in ((a, b), (b, a)):
            want = assert_search(e, o, variant, s, t, None, ("ell", rot), expect_path=True)
            assert len(want) >= 45
            assert_exact_fit(e, variant, s, t, want, ("ell", rot, s, t))


N = 32


def rebuild_map():
    rnd = np.random.default_rng(32)
    g = (rnd.random((N, N)) < 0.03).astype(np.uint8)
    g[0, 0], g[N - 1, N - 1] = 2, 3
    return g


def test_mpa_rebuild_second_leg_at_an_offset():
    """pf_mpa_rebuild_batch on a nearly empty map (long straight runs): the rebuilt path is prefix + leg 1 + leg 2, each leg walked
    into the row behind what stands there already.  Rows of exactly L cells and of L - 1, the case between two rebuilds that fit
    either row, guard rows around the launch."""
    from pathfit import rng as pfrng
    from pathfit._lib import MpaParams
    from pathfit.engine import score_params
    from pathfit.mpa import levy_sigma
    e, o, g = world("rebuild", rebuild_map)
    s, t = 0, N * N - 1
    base = o.astar(s, t, None, 1)[0]
    elite = base.copy()
    cases, short = [], []
    for agent in range(600):
        idx, is_levy, scale = agent % (len(base) - 1), agent % 2 == 0, (0.5, 5.0, 40.0)[agent % 3]
        out, isnew, _, _ = o.mpa_rebuild(s, t, base, elite, idx, is_levy, scale, 1.5, levy_sigma(1.5), o.rng(31, pfrng.DOM_MPA, 4, agent))
        if isnew and len(out) > len(base) + 8 and idx >= 3 and len(cases) < 8:
            cases.append((agent, idx, is_levy, scale, out))
        if isnew and len(out) <= len(base) and idx >= 2 and len(short) < 2:
            short.append((agent, idx, is_levy, scale, out))
    assert len(cases) == 8 and len(short) == 2
    sp = score_params(1, True, 0.1, 0.05, 1.5, 1000.0)
    e.mpa_setup(MpaParams(0.5, 1.5, levy_sigma(1.5), 0.2, 3, 0, N * N - 1, 1, 1), sp)
    bstats = o.score(base, 1, 0.1, 0.05, 1.5, True, 1000.0)
    for case in cases:
        want = case[4]
        L = len(want)
        trio = (short[0], case, short[1])
        for cap in (L, L - 1):
            pop = np.zeros((3, cap), np.int32); pop[:, :len(base)] = base
            dpop, dlen, dstats, del_ = e.put(pop), e.put(np.full(3, len(base), np.int32)), e.put(np.tile(bstats, (3, 1))), e.put(elite)
            d_idx, d_lv = e.put(np.array([c[1] for c in trio], np.int32)), e.put(np.array([int(c[2]) for c in trio], np.int32))
            d_sc, d_ag = e.put(np.array([c[3] for c in trio], np.float64)), e.put(np.array([c[0] for c in trio], np.int32))
            rows, ost = Rows(e, 3, cap), e.put(np.full((5, 5), -1.0))
            pc, pl, ps = rows.ptrs()
            e._ck(e.L.pf_mpa_rebuild_batch(e.h, 4, 31, 3, cap, dpop.ptr, dlen.ptr, dstats.ptr, del_.ptr, len(elite), d_idx.ptr,
                                           d_lv.ptr, d_sc.ptr, d_ag.ptr, pc, pl, ost.at(5), ps))
            c, l, st = rows.read()
            for a, f in ((0, short[0][4]), (2, short[1][4])):
                assert st[a] == 0 and l[a] == len(f) and np.array_equal(c[a, :len(f)], f) and (c[a, len(f):] == CANARY).all(), ("neighbour row", a)
            if cap == L:
                assert st[1] == 0 and l[1] == L and np.array_equal(c[1], want), (case[:4], st[1], l[1])
                assert np.array_equal(ost.download()[2], o.score(want, 1, 0.1, 0.05, 1.5, True, 1000.0))
            else:
                assert st[1] == OVERFLOW and l[1] == 0, (case[:4], st[1], l[1])


# ------------------------------------------------------------------ flood
M = 50
SIZES = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513)
OUTSIDE = 44 * M + 44


def pocket(k):
    """-> (cells of a pocket of k cells, rows of 24 from (2, 2); cells of its wall: every other cell that touches one, corners too)"""
    cells = [(2 + i // 24, 2 + i % 24) for i in range(k)]
    inside = set(cells)
    wall = {(r + dr, c + dc) for r, c in cells for dr in (-1, 0, 1) for dc in (-1, 0, 1)} - inside
    assert all(0 <= r < M and 0 <= c < M for r, c in wall)
    return [r * M + c for r, c in cells], sorted(r * M + c for r, c in wall)


MO = 120


def obstacle_map():
    """All ten pockets walled in by obstacles on one 120 x 120 map.  -> (map, {k: cells of the pocket of k cells})"""
    g = np.zeros((MO, MO), np.uint8)
    inside = {}
    r0 = c0 = 0
    for k in SIZES:
        h = (k + 23) // 24 + 3
        if r0 + h > MO - 8:
            r0, c0 = 0, c0 + 28
        cells, wall = pocket(k)
        move = lambda v: (v // M + r0) * MO + (v % M + c0)
        inside[k] = [move(v) for v in cells]
        g.reshape(-1)[[move(v) for v in wall]] = 1
        r0 += h
    assert c0 + 28 < MO - 8
    return g, inside


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_pockets_sealed_by_obstacles(variant):
    """Another component: answered before the open list exists, whatever the size."""
    e, o, g = world("obstacles", lambda: obstacle_map()[0])
    OUTSIDE = MO * MO - 1
    for k in SIZES:
        inside = obstacle_map()[1][k]
        for s, t in ((OUTSIDE, inside[0]), (inside[0], OUTSIDE), (OUTSIDE, inside[-1])):
            assert_search(e, o, variant, s, t, None, ("obstacles", k), expect_path=False, no_pops=True)
        if k > 1:
            assert_search(e, o, variant, inside[0], inside[-1], None, ("obstacles, inside", k), expect_path=True)


@pytest.mark.parametrize("variant", [0, 1])
def test_pockets_sealed_by_an_avoid_wall(variant):
    """One component, so only the flood can answer: up to 512 cells without a pop, 513 with the reference's pops and pushes."""
    e, o, g = world("free50", lambda: np.zeros((M, M)))
    for k in SIZES:
        inside, wall = pocket(k)
        wall = np.array(wall, np.int32)
        for s, t in ((OUTSIDE, inside[0]), (inside[0], OUTSIDE), (OUTSIDE, inside[-1]), (inside[-1], OUTSIDE), (inside[k // 2], OUTSIDE)):
            want = assert_search(e, o, variant, s, t, wall, ("avoid wall", k), expect_path=False, no_pops=k <= 512)
            assert len(want) == 0
        if k > 1:                                         # both ends inside: the flood meets the goal (or gives up), the search runs
            assert_search(e, o, variant, inside[0], inside[-1], wall, ("avoid wall, inside", k), expect_path=True)
    assert_search(e, o, variant, 0, OUTSIDE, None, "open", expect_path=True)


@pytest.mark.parametrize("variant", [0, 1])
def test_goal_just_outside_a_512_cell_pocket(variant):
    """The start inside 512 cells behind an avoid wall with the goal as the one way out: a gap in the wall (either variant), and,
    closed-set variant, a cell of the wall itself (the goal is exempt from the avoid set there, astar.py:55-56)."""
    e, o, g = world("free50", lambda: np.zeros((M, M)))
    inside, wall = pocket(512)
    for gap in (wall[0], wall[len(wall) // 2], wall[-1]):
        for s in (inside[0], inside[-1], inside[300]):
            assert_search(e, o, variant, s, gap, np.array([w for w in wall if w != gap], np.int32), ("gap", gap), expect_path=True)
            if variant == 0:
                assert_search(e, o, variant, s, gap, np.array(wall, np.int32), ("wall cell", gap), expect_path=True)
            else:                                         # MPA.py:82: an avoided goal is never pushed
                assert_search(e, o, variant, s, gap, np.array(wall, np.int32), ("wall cell", gap), expect_path=False, no_pops=True)
