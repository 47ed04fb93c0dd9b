"""A path that does not fit path_cap is "never silently truncated" (include/pathfit.h): with a row of exactly L cells the path of
L cells comes back whole, with L - 1 the agent reports PF_ST_OVERFLOW, length 0 and is counted in overflow_agents -- and in both
calls nothing is written outside the agent's own row.  pf_astar_batch (three variants), pf_decode_batch / _multi and
pf_mpa_rebuild_batch, 16 cases each whose length the CPU oracle gives, L = 1 and L = 2 among them for the searches and the
decodes (a rebuild is always longer: see rebuild_cases).  The output rows sit between rows of a canary value: a neighbour
agent's row on either side inside the launch, and guard rows outside it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 24
CANARY = -7777
OVERFLOW = 3


def fit_map():
    rnd = np.random.default_rng(24)
    g = (rnd.random((N, N)) < 0.08).astype(np.uint8)
    g[0, 0], g[N - 1, N - 1] = 2, 3
    return g


@pytest.fixture(scope="module")
def env():
    from pathfit.engine import Engine
    import pf_oracle as po
    g = fit_map()
    e = Engine(g)
    yield e, po.Oracle(g), g
    e.close()


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
        """-> (cells [n][cap], len [n], status [n]) after checking that the guards still hold the canary."""
        c, l, s = self.cells.download(), self.len.download(), self.status.download()
        for a in (c, l, s):
            assert (a[0] == CANARY).all() and (a[-1] == CANARY).all(), "a guard row was written"
        return c[1:-1], l[1:-1], s[1:-1]


def check_rows(rows, want, fits, fillers):
    """Agent 1 is the case, agents 0 and 2 (if present) paths that fit either row (fillers: a one-cell path given as its cell, or
    the cells of a short one): rows 0 and 2 hold their path and the canary behind it."""
    c, l, s = rows.read()
    mid = 1 if rows.n == 3 else 0
    if rows.n == 3:
        for a, f in ((0, np.atleast_1d(fillers[0])), (2, np.atleast_1d(fillers[1]))):
            assert s[a] == 0 and l[a] == len(f) and np.array_equal(c[a, :len(f)], f) and (c[a, len(f):] == CANARY).all(), ("neighbour row", a, c[a])
    if fits:
        assert s[mid] == 0 and l[mid] == len(want) and np.array_equal(c[mid, :len(want)], want), (s[mid], l[mid])
        assert (c[mid, len(want):] == CANARY).all()
    else:
        assert s[mid] == OVERFLOW and l[mid] == 0, (s[mid], l[mid])
    assert rows.e.counters()["overflow_agents"] == (0 if fits else 1)


def search_cases(o, g, variant):
    """16 (start, target, avoid) with a path: start == target, two adjacent cells, then random pairs, half with an avoid list."""
    rnd = np.random.default_rng(5 + variant)
    free = np.flatnonzero(g.reshape(-1) != 1)
    cases = [(int(free[7]), int(free[7]), None), (0, 1 if g[0, 1] != 1 else N, None)]
    while len(cases) < 16:
        s, t = (int(v) for v in rnd.choice(free, 2))
        av = rnd.choice(free, 25).astype(np.int32) if len(cases) % 2 else None
        if len(o.astar(s, t, av, variant)[0]) > 2:
            cases.append((s, t, av))
    return cases


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_astar_batch_exact_fit(env, variant):
    e, o, g = env
    lens = set()
    for s, t, av in search_cases(o, g, variant):
        want = o.astar(s, t, av, variant)[0]
        L = len(want)
        lens.add(L)
        ds, dt = e.put(np.array([s, s, t], np.int32)), e.put(np.array([s, t, t], np.int32))      # neighbours: start == target
        off = np.array([0, 0, len(av) if av is not None else 0, len(av) if av is not None else 0], np.int64)
        doff, dav = e.put(off), e.put(av if av is not None else np.zeros(1, np.int32))
        for cap in (L, L - 1):
            rows = Rows(e, 3, max(cap, 1))
            pc, pl, ps = rows.ptrs()
            rc = e.L.pf_astar_batch(e.h, variant, 1, 1, 3, ds.ptr, dt.ptr, doff.ptr, dav.ptr, cap, pc, pl, ps, None)
            if cap == 0:                                         # L = 1: a row of no cells is an argument error, nothing runs
                assert rc != 0
                c, l, st = rows.read()
                assert (c == CANARY).all() and (l == CANARY).all() and (st == CANARY).all()
                continue
            e._ck(rc)
            check_rows(rows, want, cap == L, (s, t))
    assert {1, 2} <= lens and max(lens) > 12


def decode_cases(o, g):
    """16 decodes (start, target, waypoints) with a path: W = 1..5; in the odd ones the last waypoint IS the target, so the last
    segment adds no cell and the cell that does or does not fit belongs to a middle segment."""
    rnd = np.random.default_rng(9)
    free = np.flatnonzero(g.reshape(-1) != 1)
    cases = []
    while len(cases) < 16:
        W = 1 + len(cases) % 5
        s, t = (int(v) for v in rnd.choice(free, 2))
        wp = np.sort(rnd.choice(free, W)).astype(np.int32)
        if s > t:
            wp = wp[::-1].copy()
        if len(cases) % 2:
            wp[-1] = t
        p = o.decode(s, t, wp)[0]
        if len(p) > 2 and s != t:
            cases.append((s, t, wp, p))
    return cases


def test_decode_batch_exact_fit(env):
    from pathfit.engine import score_params
    e, o, g = env
    sp = score_params(0, True, 0.3, 0.8, 1.8, 100.0)
    mids = 0
    for k, (s, t, wp, want) in enumerate(decode_cases(o, g)):
        L, W = len(want), len(wp)
        mids += int(wp[-1] == t)
        wst = o.score(want, 0, 0.3, 0.8, 1.8, True, 100.0)
        for cap in (L, L - 1):
            # pf_decode_batch: one agent between guard rows
            rows, dw, dst = Rows(e, 1, cap), e.put(wp), e.put(np.full((3, 5), -1.0))
            pc, pl, ps = rows.ptrs()
            e._ck(e.L.pf_decode_batch(e.h, 1, 1, 1, W, dw.ptr, None, s, t, cap, pc, pl, ps, C.byref(sp), dst.at(5)))
            check_rows(rows, want, cap == L, None)
            stats = dst.download()
            assert (stats[0] == -1.0).all() and (stats[2] == -1.0).all() and (cap != L or np.array_equal(stats[1], wst))
            # pf_decode_batch_multi: the case between two one-cell decodes (start == every waypoint == target)
            rows = Rows(e, 3, cap)
            pc, pl, ps = rows.ptrs()
            dw3 = e.put(np.stack([np.full(W, s, np.int32), wp, np.full(W, t, np.int32)]))
            ds, dt = e.put(np.array([s, s, t], np.int32)), e.put(np.array([s, t, t], np.int32))
            e._ck(e.L.pf_decode_batch_multi(e.h, 1, 1, 3, W, dw3.ptr, None, ds.ptr, dt.ptr, cap, pc, pl, ps, None, None))
            check_rows(rows, want, cap == L, (s, t))
    assert mids == 8
    # L = 1 and L = 2: a decode without waypoints is one search
    for s, t in ((5, 5), (0, 1 if g[0, 1] != 1 else N)):
        want = o.decode(s, t, np.zeros(0, np.int32))[0]
        assert len(want) == (1 if s == t else 2)
        for cap in (len(want), len(want) - 1):
            rows = Rows(e, 1, max(cap, 1))
            pc, pl, ps = rows.ptrs()
            rc = e.L.pf_decode_batch(e.h, 1, 1, 1, 0, None, None, s, t, cap, pc, pl, ps, None, None)
            if cap == 0:
                assert rc != 0 and (rows.read()[0] == CANARY).all()
                continue
            e._ck(rc)
            check_rows(rows, want, cap == len(want), None)


def rebuild_cases(o, g):
    """16 MPA._reconstruct_path_segment calls whose rebuilt path is LONGER than the path it modifies, and two whose rebuilt path
    is no longer than it (the neighbours).  The population rows share path_cap with the output rows, so the input has to fit a
    row of L - 1 cells too: a rebuild therefore has L >= len(input) + 1 >= 3, and L = 1 or L = 2 cannot be set up for this
    entry point (path_cap < 2 is an argument error, and MPA.py:286 returns a path of fewer than two cells unmodified)."""
    from pathfit import rng as pfrng
    from pathfit.mpa import levy_sigma
    s, t = 0, N * N - 1
    base = o.astar(s, t, None, 1)[0]
    elite = base.copy()
    cases, short = [], []
    for agent in range(400):
        idx, is_levy, scale = agent % (len(base) - 1), agent % 2 == 0, (0.5, 5.0, 40.0)[agent % 3]
        out, isnew, _, _ = o.mpa_rebuild(s, t, base, elite, idx, is_levy, scale, 1.5, levy_sigma(1.5), o.rng(31, pfrng.DOM_MPA, 4, agent))
        if isnew and len(out) > len(base) and len(cases) < 16:
            cases.append((agent, idx, is_levy, scale, out))
        if isnew and len(out) <= len(base) and idx >= 2 and len(short) < 2:      # on a shortest path: rebuilt to the same cells
            short.append((agent, idx, is_levy, scale, out))
    assert len(cases) == 16 and len(short) == 2
    return base, elite, cases, short


def test_mpa_rebuild_batch_exact_fit(env):
    """Three predators in one launch: the case between two rebuilds that fit either row, so a wrong row stride would show in a
    neighbour's row; guard rows outside the launch."""
    from pathfit._lib import MpaParams
    from pathfit.engine import score_params
    from pathfit.mpa import levy_sigma
    e, o, g = env
    base, elite, cases, short = rebuild_cases(o, g)
    sp = score_params(1, True, 0.1, 0.05, 1.5, 1000.0)
    e.mpa_setup(MpaParams(0.5, 1.5, levy_sigma(1.5), 0.2, 3, 0, N * N - 1, 1, 1), sp)
    bstats = o.score(base, 1, 0.1, 0.05, 1.5, True, 1000.0)
    sstats = [o.score(c[4], 1, 0.1, 0.05, 1.5, True, 1000.0) for c in short]
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
            check_rows(rows, want, cap == L, (short[0][4], short[1][4]))
            stats = ost.download()
            assert (stats[0] == -1.0).all() and (stats[4] == -1.0).all()
            assert np.array_equal(stats[1], sstats[0]) and np.array_equal(stats[3], sstats[1])
            assert cap != L or np.array_equal(stats[2], o.score(want, 1, 0.1, 0.05, 1.5, True, 1000.0))
