"""Pins the CPU model of the space-time fields (tests/spacetime_checkers.py) on any host: the literal and the word-parallel forms
against each other, the static limits against BFS and Dijkstra, the facts DESIGN.md 4.25 quotes, the route rule against the conflict
check, two broken solvers the model must reject, and the three fleet properties."""
from collections import deque

import numpy as np
import pytest

import field_checkers as fc
import spacetime_checkers as sc


def seeded_case(seed, R=None, C=None):
    """A grid of 3 - 11 cells a side (or the given one), 0 - 4 obstacles of both after_end kinds, some sources."""
    rnd = np.random.default_rng(seed)
    R = int(rnd.integers(3, 12)) if R is None else R
    C = int(rnd.integers(3, 12)) if C is None else C
    S = rnd.random((R, C)) < 0.2
    T = int(rnd.integers(0, 2 * (R + min(C, 12)) + 2))
    D = np.zeros((T + 1, R, C), bool)
    for i in range(int(rnd.integers(0, 5))):
        v = int(rnd.integers(0, R * C))
        row = [v]
        for _ in range(int(rnd.integers(0, T + 3))):
            if rnd.random() < 0.1:
                v = int(rnd.integers(0, R * C))                       # an obstacle may jump
            else:
                k = int(rnd.integers(-1, 8))
                r, c = v // C + (0 if k < 0 else sc.DR[k]), v % C + (0 if k < 0 else sc.DC[k])
                if 0 <= r < R and 0 <= c < C:
                    v = r * C + c
            row.append(v)
        sc.planes((R, C), T, [row], [int(rnd.integers(0, T + 1))], "stay" if i % 2 else "vanish", bool(rnd.integers(0, 2)), into=D)
    src = [int(v) for v in rnd.integers(0, R * C, int(rnd.integers(1, 4)))]
    return S, D, src


def bfs_hops(mm, src):
    R, C = mm.shape
    hops = np.full(R * C, -1, np.int32)
    hops[src] = 0
    q = deque([src])
    while q:
        u = q.popleft()
        for k in range(8):
            if (mm.reshape(-1)[u] >> k) & 1:
                v = u + sc.DR[k] * C + sc.DC[k]
                if hops[v] < 0:
                    hops[v] = hops[u] + 1
                    q.append(v)
    return hops.reshape(R, C)


def test_pack_roundtrip_and_layout():
    rnd = np.random.default_rng(1)
    for C in (1, 63, 64, 65, 130):
        b = rnd.random((3, 2, C)) < 0.5
        w = sc.pack(b)
        assert w.shape == (3, 2, (C + 63) // 64) and w.dtype == np.uint64
        assert np.array_equal(sc.unpack(w, C), b)
        for c in range(C):
            assert bool((int(w[1, 1, c >> 6]) >> (c & 63)) & 1) == bool(b[1, 1, c])
        if C & 63:
            assert int(w[0, 0, -1]) >> (C & 63) == 0


@pytest.mark.parametrize("ad,rs", sc.POLICIES)
def test_literal_and_word_forms_agree(ad, rs):
    cases = [seeded_case(s) for s in range(40)] + [seeded_case(100 + C, R=3 + C % 3, C=C) for C in (63, 64, 65)]
    for S, D, src in cases:
        a0, r0 = sc.field(S, D, src, ad, rs)
        a1, w1 = sc.field_words(S, sc.pack(D), src, ad, rs)
        assert np.array_equal(a0, a1)
        assert np.array_equal(sc.pack(r0), w1)
        assert np.array_equal(a0, sc.arrival_of(r0))


@pytest.mark.parametrize("ad,rs", sc.POLICIES)
def test_static_limit_is_bfs_under_the_move_mask(ad, rs):
    for seed in range(12):
        S, D, src = seeded_case(seed)
        R, C = S.shape
        D = np.zeros((R * C + 1, R, C), bool)
        mm = fc.move_masks(S.astype(np.uint8), ad, rs)
        s = src[0]
        arrive, _ = sc.field_words(S, sc.pack(D), [s], ad, rs, want_reach=False)
        want = bfs_hops(mm, s) if not S.reshape(-1)[s] else np.full((R, C), -1, np.int32)
        assert np.array_equal(arrive, want)
        if not ad:
            d, _ = fc.reference_dijkstra(S.astype(np.uint8), mm, s)
            assert np.array_equal(np.where(np.isfinite(d), d, -1.0), arrive.astype(np.float64))


@pytest.mark.parametrize("ad,rs", sc.POLICIES)
def test_parked_obstacle_is_a_closed_cell(ad, rs):
    for seed in range(12):
        S, _, src = seeded_case(seed)
        R, C = S.shape
        T = R * C
        x = int(np.random.default_rng(seed).integers(0, R * C))
        D, _ = sc.planes((R, C), T, [[x]], None, "stay")
        S2 = S.copy()
        S2.reshape(-1)[x] = True
        a0, _ = sc.field(S, D, src, ad, rs)
        a1, _ = sc.field(S2, np.zeros_like(D), src, ad, rs)
        assert np.array_equal(a0, a1)


@pytest.mark.parametrize("ad,rs", sc.POLICIES)
def test_traced_routes_have_no_conflicts(ad, rs):
    traced = 0
    for seed in range(30):
        S, D, src = seeded_case(seed)
        R, C = S.shape
        T = D.shape[0] - 1
        arrive, reach = sc.field(S, D, src, ad, rs)
        for v in np.flatnonzero(arrive.reshape(-1) >= 0)[::3]:
            for tick in (-1, -2):
                cells, st, tk = sc.route(S, D, reach, int(v), tick, ad, rs)
                if tick == -1:
                    assert st == sc.ST_OK and tk == arrive.reshape(-1)[v]
                if cells is None:
                    assert tick == -2 and st == sc.ST_INFEASIBLE
                    continue
                assert len(cells) == tk + 1 and cells[-1] == v and cells[0] in src
                out, status = sc.conflicts(S, D, cells, 0, ad, rs, hold=(tick == -2))
                assert out == (-1, 0, -1, 0) and status == 0, (seed, v, tick, out)
                traced += 1
    assert traced > 100


def test_conflict_kinds_and_precedence():
    S = np.zeros((3, 4), bool)
    S[2, 3] = True
    C, T = 4, 6
    D, _ = sc.planes((3, 4), T, [[1, 0], [6]], [0, 1], "vanish")      # one obstacle walks (0,1) -> (0,0); one stands on (1,2) at tick 1
    assert sc.conflicts(S, D, [0, 1], 0, 1, 1) == ((1, sc.SWAP, 1, 1), 0)
    assert sc.conflicts(S, D, [4, 0], 0, 1, 1) == ((1, sc.VERTEX, 0, 1), 0)
    assert sc.conflicts(S, D, [5, 10], 0, 1, 1) == ((1, sc.CORNER, 10, 1), 0)          # (1,1) -> (2,2): the corner (1,2) is taken at tick 1
    assert sc.conflicts(S, D, [5, 10], 0, 1, 0)[0] == (-1, 0, -1, 0)
    assert sc.conflicts(S, D, [5, 10], 0, 0, 1) == ((1, sc.STATIC, 10, 1), 0)          # no diagonals in the policy
    assert sc.conflicts(S, D, [7, 10], 0, 1, 1) == ((1, sc.STATIC, 10, 1), 0)          # (1,3) -> (2,2) cuts the static corner (2,3)
    assert sc.conflicts(S, D, [7, 11], 0, 1, 1) == ((1, sc.STATIC, 11, 1), 0)
    assert sc.conflicts(S, D, [4, 6], 0, 1, 1) == ((1, sc.STATIC, 6, 1), 0)            # a jump, though the cell is taken too
    assert sc.conflicts(S, D, [1, 1], 0, 1, 1) == ((0, sc.VERTEX, 1, 1), 0)            # the first cell at t0
    assert sc.conflicts(S, D, [11], 2, 1, 1) == ((2, sc.STATIC, 11, 1), 0)
    assert sc.conflicts(S, D, [], 0, 1, 1) == ((-1, 0, -1, 0), 1)
    assert sc.conflicts(S, D, [12], 0, 1, 1) == ((-1, 0, -1, 0), 1)
    assert sc.conflicts(S, D, [0], 7, 1, 1) == ((-1, 0, -1, 0), 1)
    assert sc.conflicts(S, D, [4, 4, 4, 4], 4, 1, 1) == ((-1, 0, -1, 0), 2)
    D2, _ = sc.planes((3, 4), T, [[9, 5, 5, 1]], [2], "stay")
    assert sc.conflicts(S, D2, [4, 5], 0, 1, 1, hold=False) == ((-1, 0, -1, 0), 0)
    assert sc.conflicts(S, D2, [4, 5], 0, 1, 1, hold=True) == ((3, sc.VERTEX, 5, 2), 0)


def test_the_model_rejects_a_solver_without_the_swap_rule():
    S = np.zeros((1, 3), bool)
    D, _ = sc.planes((1, 3), 3, [[1, 0]], None, "vanish")             # the obstacle and the robot would pass through each other
    good, _ = sc.field(S, D, [0], 1, 1)
    broken, _ = sc.field(S, D, [0], 1, 1, swap_rule=False)
    assert good.tolist() == [[0, -1, -1]] and broken.tolist() == [[0, 1, 2]]
    differ = sum(not np.array_equal(sc.field(*seeded_case(s, R=1, C=6), 1, 1)[0], sc.field(*seeded_case(s, R=1, C=6), 1, 1, swap_rule=False)[0])
                 for s in range(40))                                  # seeded corridors, where nothing leads round the obstacle
    assert differ > 0


def test_the_model_rejects_a_solver_with_corners_at_the_later_tick_only():
    S = np.zeros((2, 2), bool)
    D, _ = sc.planes((2, 2), 3, [[1]], None, "vanish")                # the corner (0,1) is taken at tick 0 only
    good, _ = sc.field(S, D, [0], 1, 1)
    broken, _ = sc.field(S, D, [0], 1, 1, corner_both=False)
    assert good.tolist() == [[0, 1], [1, 2]] and broken.tolist() == [[0, 1], [1, 1]]
    differ = sum(not np.array_equal(sc.field(*seeded_case(s), 1, 1)[0], sc.field(*seeded_case(s), 1, 1, corner_both=False)[0]) for s in range(40))
    assert differ > 0


def pocket(col):
    S = np.zeros((2, 9), bool)
    S[1, :] = True
    S[1, col] = False
    D, _ = sc.planes((2, 9), 24, [list(range(8, -1, -1))], None, "vanish")
    return S, D


def test_fact_pocket_at_column_3():
    S, D = pocket(3)
    for ad, rs in ((0, 1), (0, 0), (1, 1)):
        arrive, reach = sc.field(S, D, [0], ad, rs)
        assert arrive[0, 8] == 11 and arrive[1, 3] == 4
        assert reach.reshape(25, -1).sum(axis=1)[:8].tolist() == [1, 2, 3, 4, 5, 4, 4, 5]      # the reach set shrinks
    assert sc.field(S, D, [0], 1, 0)[0][0, 8] == 9


def test_fact_pocket_at_column_4():
    S, D = pocket(4)
    for ad, rs in ((0, 1), (0, 0), (1, 1)):
        arrive, reach = sc.field(S, D, [0], ad, rs)
        assert (arrive[:, 4:] == -1).all() and (arrive[0, :4] >= 0).all()
        assert arrive.max() == 3 and reach[7].any() and not reach[8:].any()                      # nothing new after tick 3; the set dies out
    assert sc.field(S, D, [0], 1, 0)[0][0, 8] == 8


def fleet_case(seed):
    rnd = np.random.default_rng(1000 + seed)
    while True:
        R, C = int(rnd.integers(3, 8)), int(rnd.integers(3, 8))
        S = rnd.random((R, C)) < 0.15
        free = np.flatnonzero(~S.reshape(-1))
        if len(free) >= 8:
            return S, [int(v) for v in rnd.choice(free, 4, replace=False)], [int(v) for v in rnd.choice(free, 4, replace=False)], 3 * (R + C)


def test_fleet_properties():
    robots = planned = failed = checked = corner_without = 0
    for ad, rs in ((1, 1), (1, 0), (0, 1)):
        for seed in range(120):
            S, starts, goals, T = fleet_case(seed)
            C = S.shape[1]
            routes, status, D = sc.fleet(S, T, starts, goals, ad, rs, corners=True)
            shared, swaps, corner, n = sc.fleet_violations(routes, T, C, rs)
            assert (shared, swaps, corner) == (0, 0, 0), (ad, rs, seed)
            assert n == sum(r is not None for r in routes)            # every robot planned is checked
            for i, r in enumerate(routes):
                assert (r is None) == (status[i] != sc.ST_OK)
                if r is not None:
                    assert r[0] == starts[i] and r[-1] == goals[i]
            robots += 4
            planned += n
            checked += n
            failed += 4 - n
            if rs:
                without, _, _ = sc.fleet(S, T, starts, goals, ad, rs, corners=False)
                s2, w2, c2, _ = sc.fleet_violations(without, T, C, rs)
                assert (s2, w2) == (0, 0)
                corner_without += c2
    assert robots == 1440 and checked == planned
    assert corner_without > 0, "without corner stamping the same seeds must produce corner cases"
    assert failed * 4 < robots, (failed, robots)
    print("fleet: robots", robots, "failed", failed, "corner cases without stamping", corner_without)
