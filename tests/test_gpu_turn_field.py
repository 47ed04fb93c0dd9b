"""Turn fields on the device (pf_turn_field / pf_turn_field_paths / pf_turn_paths, pathfit.TurnField) against the model of
tests/turn_checkers.py (a heap Dijkstra over (cell, heading) states, pinned by tests/test_turn_checkers.py against random-order sweeps,
the literal rule, the simple-path minimum and the route rule).  Every comparison is exact equality -- labels bit for bit --; every
output lies between canary words."""
import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc
import golden_io as gio
import thin_maps
import turn_checkers as tk
import widest_checkers as wc

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64
TW, TH = tk.TW, tk.TH
OK, INFEASIBLE, OVERFLOW = 0, 1, 3


def between_canaries(e, n, dtype):
    return e.put(np.full(n + 2 * PAD, CANARY, dtype))


def inner(buf, tag):
    a = buf.download()
    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), tag
    return a[PAD:len(a) - PAD]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def view(e, buf, n, dtype):
    from pathfit.engine import _View
    return _View(e, buf.at(PAD), n, dtype)


class Field:
    """An engine on a map and, when there is one, a cost map in HBM."""

    def __init__(self, g, cost=None):
        from pathfit.engine import Engine
        self.g, self.e = np.asarray(g), Engine(g)
        self.dcost = self.e.buf(self.g.size, np.float64)
        self.set_cost(cost)

    def set_cost(self, cost):
        self.cost = None if cost is None else np.ascontiguousarray(cost, np.float64)
        if cost is not None:
            self.dcost.upload(self.cost.reshape(-1))
        return self

    def run(self, sets, wt, ad, rs, want_info=True):
        """One raw field call, every output between canaries -> (T [B, 8, R, C], best [B, R, C], info [B, 4] or None)."""
        e, B, RC = self.e, len(sets), self.g.size
        off, src = ck.csr(sets)
        sb, bb, ib = between_canaries(e, 8 * B * RC, np.float64), between_canaries(e, B * RC, np.float64), between_canaries(e, 4 * B, np.int64)
        try:
            e.turn_field(self.dcost if self.cost is not None else None, wt, off, src, view(e, sb, 8 * B * RC, np.float64), view(e, bb, B * RC, np.float64), ad, rs,
                         view(e, ib, 4 * B, np.int64) if want_info else None)
            assert e.last_kernel_ms() > 0
            self.work = work = e.turn_field_work()
            assert work[3] == 0 and work[0] <= work[1] and (work[0] > 0) == (work[1] > 0)
            T, best, info = inner(sb, "T").reshape((B, 8) + self.g.shape), inner(bb, "best").reshape((B,) + self.g.shape), inner(ib, "info").reshape(B, 4)
            if not want_info:
                assert np.all(info == CANARY)
            return T, best, (info if want_info else None)
        finally:
            for b in (sb, bb, ib):
                b.free()

    def check(self, sets, wt, policies=tk.POLICIES, tag=None, want_info=(True,)):
        for ad, rs in policies:
            wT, wbest, winfo = tk.fields(self.g, self.cost, sets, wt, ad, rs)
            for wi in want_info:
                T, best, info = self.run(sets, wt, ad, rs, wi)
                assert same_bits(T, wT), (tag, self.g.shape, wt, ad, rs, "T", np.argwhere(T != wT)[:4])
                assert same_bits(best, wbest), (tag, self.g.shape, wt, ad, rs, "best", np.argwhere(best != wbest)[:4])
                assert info is None or np.array_equal(info, winfo), (tag, self.g.shape, wt, ad, rs, info, winfo)

    def close(self):
        self.e.close()


def free_cells(g, n, seed):
    free = np.flatnonzero(np.asarray(g).reshape(-1) != 1)
    return [int(v) for v in np.random.default_rng(seed).choice(free, min(n, len(free)), replace=False)]


def check_map(g, sets, kinds=("none", "u50"), weights=(0.3,), policies=tk.POLICIES, want_info=(True,), tag=None, seed=0):
    f = Field(g)
    try:
        for i, kind in enumerate(kinds):
            f.set_cost(None if kind == "none" else ck.cost_of_kind(kind, f.g.shape, seed + i))
            for wt in weights:
                f.check(sets, wt, policies, (tag, kind), want_info)
    finally:
        f.close()


# ---- 1. golden and thin maps
@pytest.mark.parametrize("name", ["fig7", "fig13", "img1"])
def test_golden_20x20_maps(name):
    g, s, t = gio.grid(name)
    check_map(g, [[s], [t], [s, t]], kinds=("none", "ones", "int14", "u50", "u1e6"), weights=(0.0, 0.3, 3.0), want_info=(True, False))


@pytest.mark.parametrize("R, C", thin_maps.SHAPES)
def test_thin_maps(R, C):
    for ob in (False, True):
        if not ob or thin_maps.has_obstacle_version(R, C):
            g, s, t = thin_maps.thin_map(R, C, ob)
            check_map(g, [[s], [t], [s, t]], want_info=(True, False), tag=ob, seed=R + C)
    if min(R, C) == 1:                                               # one cell wide: states exist for two headings only
        g, s, t = thin_maps.thin_map(R, C, False)
        f = Field(g)
        try:
            T = f.run([[t]], 0.3, 1, 1)[0][0].reshape(8, -1)
            along = (0, 1) if R == 1 else (2, 3)
            rest = [d for d in range(8) if d not in along]
            assert np.all(np.isinf(np.delete(T[rest], t, axis=1))) and np.all(T[:, t] == 0.0)
            assert np.isfinite(T[list(along)]).sum() == 2 * R * C - 1     # every cell by both headings, but no way into the first cell from beyond the map
        finally:
            f.close()


# ---- 2. sizes about the tile
@pytest.mark.parametrize("C", [TW - 1, TW, TW + 1, 2 * TW])
@pytest.mark.parametrize("R", [TH - 1, TH, TH + 1, 2 * TH])
def test_sizes_about_the_tile(R, C):                                 # (the shifted copies are one row and one column larger: 2 T + 1 too)
    g = wc.seeded(R, C, 0.25, 100 * R + C)
    for j, m in enumerate((g, wc.shifted_cols(wc.shifted_rows(g)))):
        src = free_cells(m, 3, R + C + j)
        check_map(m, [src[:1], src], kinds=("u50",), policies=[(1, 1), (0, 1)] if j == 0 else [(1, 0), (0, 0)], seed=R * C)


def test_a_diagonal_gap_across_a_tile_corner():
    r, c = 2 * TH, TW                                                 # the four cells about (r, c) lie in four tiles
    g = wc.corner_gap(4 * TH + 3, 2 * TW + 5, r, c)
    assert g[r - 1, c - 1] == 1 and g[r, c] == 1 and g[r - 1, c] == 0 and g[r, c - 1] == 0
    f = Field(g, ck.cost_of_kind("u50", g.shape, 5))
    try:
        left, right = (r + 5) * g.shape[1] + 3, 3 * g.shape[1] + c + 9
        rows = {}
        for ad, rs in tk.POLICIES:
            f.check([[left], [right]], 0.3, [(ad, rs)])
            rows[ad, rs] = f.run([[left], [right]], 0.3, ad, rs)[1]
        free, restricted = rows[1, 0], rows[1, 1]
        assert np.isfinite(free[0].reshape(-1)[right]) and np.isfinite(free[1].reshape(-1)[left])      # through the gap
        assert np.isinf(restricted[0].reshape(-1)[right]) and np.isinf(restricted[1].reshape(-1)[left])
        assert np.isinf(rows[0, 1][0].reshape(-1)[right]) and np.isinf(rows[0, 0][0].reshape(-1)[right])
    finally:
        f.close()


# ---- 3. the maps of the CPU facts
def test_the_pocket_and_the_zigzag_map():
    g, s, v, d = tk.pocket_map()
    f = Field(g)
    try:
        f.check([[s]], 0.3)
        T = f.run([[s]], 0.3, 1, 1)[0]
        assert T[0].reshape(8, -1)[d, v] == (1.0 + 1.0) + (1.0 + 0.3)                 # out into the dead end and back
    finally:
        f.close()
    g, s, t = tk.zigzag_map()
    f = Field(g)
    try:
        f.check([[s]], 3.0)
        best = f.run([[s]], 3.0, 1, 1)[1]
        short = fc.trace(fc.reference_dijkstra(g, fc.move_masks(g, 1, 1), s)[1], t)
        assert best[0].reshape(-1)[t] < tk.path_cost(None, short, g.shape[1], 3.0)[0]
    finally:
        f.close()


@pytest.mark.parametrize("stacked", [False, True])
def test_a_tile_is_lowered_again_through_its_neighbour(stacked):
    cost, s, probe, in_far_tile = tk.detour_map(stacked)
    f = Field(np.zeros(cost.shape, np.uint8), cost)
    try:
        for ad, rs in ((1, 1), (0, 1)):
            assert tk.needs_the_far_tile(cost, s, probe, in_far_tile, 0.3, ad, rs)
            f.check([[s]], 0.3, [(ad, rs)])
            # the near tile alone is queued in round 1 and is final only after the far tile has run: true under any timing
            assert f.work[0] >= 3 and f.work[1] >= 3, f.work
    finally:
        f.close()


# ---- 4. magnitudes
@pytest.mark.parametrize("c", [1.0, 2.0 ** 20])
def test_a_corridor_of_4096_cells(c):
    g = np.zeros((1, 4096), np.uint8)
    cost = np.full(g.shape, c)
    f = Field(g, cost)
    try:
        for wt in (0.0, 0.3, 2.0 ** 20):
            T, best, info = f.run([[0]], wt, 1, 1)
            sums, total = [0.0], 0.0
            for v in range(1, 4096):
                total = total + c
                sums.append(total)
            assert same_bits(best.reshape(-1), np.array(sums)) and same_bits(T[0, 0].reshape(-1), np.array(sums)) and list(info[0]) == [1, 4096, 4095, 0]
            assert 4096 // TW <= f.work[0] <= 4096 // TW + 3, f.work      # one launch per tile crossed, and the last tiles' second visits
            # westward states: out past the cell and back, one turn
            assert T[0, 1, 0, 4095] == np.inf and T[0, 1, 0, 10] == (sums[11] + (c + wt))
        f.check([[4095], [0, 2048]], 0.3, [(1, 1)])
    finally:
        f.close()


def test_weights_and_costs_at_both_bounds():
    g = wc.seeded(33, 70, 0.2, 8)
    cost = np.where(np.random.default_rng(9).random(g.shape) < 0.5, 1.0, 2.0 ** 20)
    f = Field(g, cost)
    try:
        for wt in (0.0, 0.1, 2.0 ** 20):
            f.check([free_cells(g, 1, 1), free_cells(g, 3, 2)], wt, [(1, 1), (0, 0)])
    finally:
        f.close()


# ---- 5. turn weight 0 is the cost field; no cost map is a map of ones
def cost_field_case(g, sets, policies, cost):
    f = Field(g, cost)
    e, B, RC = f.e, len(sets), f.g.size
    off, src = ck.csr(sets)
    cb = e.buf(B * RC, np.float64)
    try:
        for ad, rs in policies:
            best = f.run(sets, 0.0, ad, rs)[1]
            e.cost_field(f.dcost, off, src, cb, ad, rs)
            assert same_bits(best.reshape(-1), cb.download()), (f.g.shape, ad, rs)
    finally:
        cb.free()
        f.close()


def test_turn_weight_0_is_the_cost_field():
    g, s, t = gio.grid("fig7")
    cost_field_case(g, [[s], [t], [s, t]], tk.POLICIES, ck.cost_of_kind("u50", g.shape, 1))
    g, s, t = gio.grid("g256")
    cost_field_case(g, [[s], [s, t] + free_cells(g, 5, 2)], [(1, 1), (0, 0)], ck.cost_of_kind("u1e6", g.shape, 2))
    g = wc.seeded(130, 200, 0.25, 13)
    cost_field_case(g, [free_cells(g, 1, 3), free_cells(g, 4, 4)], [(1, 1), (1, 0), (0, 1)], np.ones(g.shape))


def test_no_cost_map_is_a_map_of_ones():
    g = wc.seeded(70, 150, 0.2, 6)
    sets = [free_cells(g, 2, 1), free_cells(g, 1, 2)]
    f = Field(g)
    try:
        for wt, (ad, rs) in ((0.3, (1, 1)), (0.0, (0, 1)), (2.0 ** 20, (1, 0))):
            none = f.set_cost(None).run(sets, wt, ad, rs)
            ones = f.set_cost(np.ones(g.shape)).run(sets, wt, ad, rs)
            assert same_bits(none[0], ones[0]) and same_bits(none[1], ones[1]) and np.array_equal(none[2], ones[2])
            assert np.isfinite(none[1]).sum() > g.size // 2
    finally:
        f.close()


# ---- 6. sets
@pytest.mark.parametrize("B", [1, 3, 70])
def test_many_sets_in_one_call(B):
    g = wc.seeded(37, 90, 0.2, 21)
    rnd = np.random.default_rng(B)
    free = np.flatnonzero(g.reshape(-1) != 1)
    sets = [[int(v) for v in rnd.choice(free, int(rnd.integers(1, 5)))] for _ in range(B)]
    check_map(g, sets, kinds=("u50",), policies=[(1, 1)] if B == 70 else [(1, 1), (0, 0)], seed=B)


def test_awkward_sets():
    g = wc.seeded(30, 80, 0.2, 5)
    g[10:17, 30:39] = 0
    g[10, 30:39] = g[16, 30:39] = g[10:17, 30] = g[10:17, 38] = 1          # a sealed room
    wall = [int(v) for v in np.flatnonzero(g.reshape(-1) == 1)[:3]]
    free = free_cells(g, 4, 6)
    room = 13 * 80 + 34
    sets = [[wall[0], free[0]], [free[1], free[1], free[2], free[1]], wall, [room], [free[3], room], [wall[1]]]
    f = Field(g, ck.cost_of_kind("u50", g.shape, 7))
    try:
        f.check(sets, 0.3, want_info=(True, False))
        T, best, info = f.run(sets, 0.3, 1, 1)
        assert list(info[0][:1]) == [1] and info[1][0] == 2 and list(info[2]) == [0, 0, -1, 0] and list(info[5]) == [0, 0, -1, 0]
        assert np.all(np.isinf(T[2])) and np.all(np.isinf(best[2])) and info[3][1] == 5 * 7 and np.isfinite(best[3]).sum() == 35
    finally:
        f.close()
    check_map(np.zeros((21, 67), np.uint8), [[0], [20 * 67 + 66, 5]], kinds=("u50", "none"), policies=[(1, 1), (0, 1)])   # no obstacle at all


def test_a_300x517_map():
    g = wc.seeded(300, 517, 0.2, 77)
    check_map(g, [free_cells(g, 1, 1)], kinds=("u50",), policies=[(1, 1)], seed=3)


# ---- 7. determinism, update_grid, refresh
def test_five_runs_are_bit_equal():
    g = wc.seeded(70, 150, 0.15, 4)
    f = Field(g, ck.cost_of_kind("u1e6", g.shape, 1))
    try:
        sets = [free_cells(g, 2, 1), free_cells(g, 1, 2)]
        first = f.run(sets, 0.3, 1, 1)
        for _ in range(4):
            again = f.run(sets, 0.3, 1, 1)
            assert same_bits(again[0], first[0]) and same_bits(again[1], first[1]) and np.array_equal(again[2], first[2])
    finally:
        f.close()


def test_refresh_after_update_grid_with_a_new_cost_map_and_turn_weight():
    import pathfit
    g = np.zeros((24, 90), np.uint8)
    g[:, 45] = 1                                                      # a wall without a door
    cost = ck.cost_of_kind("u50", g.shape, 2)
    e = pathfit.Engine(g)
    tf = pathfit.TurnField(g, [[(3, 3)], [(20, 80), (3, 3)]], 0.3, cost=cost, engine=e)
    try:
        sets = [[3 * 90 + 3], [20 * 90 + 80, 3 * 90 + 3]]
        want = tk.fields(g, cost, sets, 0.3, True, True)
        assert same_bits(tf.states, want[0]) and same_bits(tf.best, want[1]) and np.array_equal(tf.info, want[2])
        assert np.isinf(tf.best[0][:, 46:]).all() and tf.work[0] >= 1 and tf.kernel_ms > 0
        g2 = g.copy()
        g2[11, 45] = 0                                                # a door
        e.update_grid(g2)
        assert tf.refresh() is tf
        want2 = tk.fields(g2, cost, sets, 0.3, True, True)
        assert same_bits(tf.states, want2[0]) and same_bits(tf.best, want2[1]) and np.array_equal(tf.info, want2[2])
        assert np.isfinite(tf.best[0][:, 46:]).all() and not same_bits(want2[1], want[1])
        tf.refresh(turn_weight=3.0)
        want3 = tk.fields(g2, cost, sets, 3.0, True, True)
        assert tf.turn_weight == 3.0 and same_bits(tf.states, want3[0]) and same_bits(tf.best, want3[1]) and not same_bits(want3[1], want2[1])
        cost4 = ck.cost_of_kind("int14", g.shape, 3)
        tf.refresh(cost=cost4)
        want4 = tk.fields(g2, cost4, sets, 3.0, True, True)
        assert same_bits(tf.states, want4[0]) and same_bits(tf.cost_device.download().reshape(g.shape), cost4)
        for cell in ((11, 46), (3, 3), (0, 89)):
            col = want4[0][1][:, cell[0], cell[1]]
            assert tf.heading(1, cell) == int(np.argmin(col))
        assert tf.heading(0, (5, 45)) is None
    finally:
        tf.close()
        e.close()


# ---- 8. routes
def run_paths(e, dcost, wt, B, dstates, set_idx, targets, cap, reverse, n=None):
    rows = len(targets)
    dk, dt = e.put(np.asarray(set_idx, np.int32)), e.put(np.asarray(targets, np.int32))
    cb, lb, sb = between_canaries(e, rows * cap, np.int32), between_canaries(e, rows, np.int32), between_canaries(e, rows, np.int32)
    try:
        e.turn_field_paths(dcost, wt, B, dstates, dk, dt, rows if n is None else n, cap, view(e, cb, rows * cap, np.int32), view(e, lb, rows, np.int32),
                           view(e, sb, rows, np.int32), reverse)
        return inner(cb, "cells").reshape(rows, cap), inner(lb, "len"), inner(sb, "status")
    finally:
        for b in (dk, dt, cb, lb, sb):
            b.free()


def run_turn_paths(e, dcost, wt, cells, lens, cap, n=None):
    rows = len(lens)
    dc, dl = e.put(np.ascontiguousarray(cells, np.int32)), e.put(np.asarray(lens, np.int32))
    tb, nb, bb = between_canaries(e, rows, np.float64), between_canaries(e, rows, np.int32), between_canaries(e, rows, np.int32)
    try:
        e.turn_paths(dcost, wt, rows if n is None else n, cap, dc, dl, view(e, tb, rows, np.float64), view(e, nb, rows, np.int32), view(e, bb, rows, np.int32))
        return inner(tb, "total"), inner(nb, "turns"), inner(bb, "bad")
    finally:
        for b in (dc, dl, tb, nb, bb):
            b.free()


@pytest.mark.parametrize("ad, rs, kind, wt", [(1, 1, "u50", 0.3), (0, 0, "none", 3.0), (1, 0, "int14", 0.0)])
def test_routes_are_the_checkers_cell_for_cell(ad, rs, kind, wt):
    g = wc.seeded(45, 100, 0.22, 31)
    R, C = g.shape
    cost = None if kind == "none" else ck.cost_of_kind(kind, g.shape, 9)
    src = free_cells(g, 5, 10)
    sets = [src[:1], src[1:], src]
    wT, wbest, _ = tk.fields(g, cost, sets, wt, ad, rs)
    targets = free_cells(g, 40, 11) + src[:2] + [int(np.flatnonzero(g.reshape(-1) == 1)[0]), -1, R * C, 2 ** 31 - 1]
    f = Field(g, cost)
    e = f.e
    dstates = e.put(wT.reshape(-1))                                    # (bit for bit the device's: test 1 and its kin)
    dcost = f.dcost if cost is not None else None
    try:
        assert same_bits(f.run(sets, wt, ad, rs)[0], wT)
        for b in range(3):
            routes = [tk.route(wT[b], cost, t, wt) if 0 <= t < R * C else [] for t in targets]
            longest = max(len(r) for r in routes)
            for reverse in (False, True):
                for cap in (longest, longest - 1, R * C):              # rows of exactly L and L - 1 cells
                    cells, lens, st = run_paths(e, dcost, wt, 3, dstates, [b] * len(targets), targets, cap, reverse)
                    for i, r in enumerate(routes):
                        if not r:
                            assert (lens[i], st[i]) == (0, INFEASIBLE) and np.all(cells[i] == CANARY), (b, i)
                        elif len(r) > cap:
                            assert (lens[i], st[i]) == (0, OVERFLOW) and np.all(cells[i] == CANARY), (b, i)
                        else:
                            assert (lens[i], st[i]) == (len(r), OK) and cells[i, :len(r)].tolist() == (r[::-1] if reverse else r), (b, i, reverse)
                            assert np.all(cells[i, len(r):] == CANARY)
                    assert (st == OVERFLOW).any() == (cap == longest - 1)
            # the rule's cost of the routes is the label, bit for bit
            cap = longest
            cells, lens, st = run_paths(e, dcost, wt, 3, dstates, [b] * len(targets), targets, cap, False)
            tot, turns, bad = run_turn_paths(e, dcost, wt, np.where(cells == CANARY, 0, cells), lens, cap)
            for i, (t, r) in enumerate(zip(targets, routes)):
                if r:
                    assert bad[i] == -1 and tot[i] == wbest[b].reshape(-1)[t] and turns[i] == tk.count_turns(r, C) and len(set(r)) == len(r), (b, i)
                else:
                    assert bad[i] == 0 and np.isnan(tot[i]) and turns[i] == 0
        # a set index outside [0, B), n == 0, and the first query alone
        cells, lens, st = run_paths(e, dcost, wt, 3, dstates, [3, -1, 0], [targets[0]] * 3, 200, False)
        assert list(st) == [INFEASIBLE, INFEASIBLE, OK] and lens[0] == 0 and lens[1] == 0
        cells, lens, st = run_paths(e, dcost, wt, 3, dstates, [0, 0], targets[:2], 200, False, n=0)
        assert np.all(cells == CANARY) and np.all(lens == CANARY) and np.all(st == CANARY)
        cells, lens, st = run_paths(e, dcost, wt, 3, dstates, [0, 0], targets[:2], 200, False, n=1)
        assert st[0] == OK and st[1] == CANARY and lens[1] == CANARY and np.all(cells[1] == CANARY)
    finally:
        dstates.free()
        f.close()


def test_garbage_states_end_every_walk():
    g = wc.seeded(40, 64, 0.2, 3)
    R, C = g.shape
    f = Field(g)
    e = f.e
    rnd = np.random.default_rng(5)
    targets = list(range(0, R * C, 37))
    try:
        for kind in ("random", "ones", "falling", "bits"):
            if kind == "random":
                junk = rnd.random((8, R * C)) * 50.0
            elif kind == "ones":
                junk = np.ones((8, R * C))                             # no state offers a label: fl(1 + e) > 1
            elif kind == "falling":                                    # labels that fall by exactly 1 to the west for ever: a walk to the map's edge
                junk = np.full((8, R * C), np.inf)
                junk[0] = (np.arange(R * C) % C + 1.0)
            else:
                junk = rnd.integers(0, 2 ** 64, (8, R * C), dtype=np.uint64).view(np.float64)
            ds = e.put(np.ascontiguousarray(junk).reshape(-1))
            try:
                for cap in (7, R * C):
                    cells, lens, st = run_paths(e, None, 0.0, 1, ds, [0] * len(targets), targets, cap, False)
                    assert np.all((st == OK) | (st == INFEASIBLE) | (st == OVERFLOW)) and np.all(lens <= min(cap, R * C)) and np.all(lens >= 0)
                    for i in range(len(targets)):
                        row = cells[i]
                        assert np.all(row[lens[i]:] == CANARY) and np.all((row[:lens[i]] >= 0) & (row[:lens[i]] < R * C))
                        assert (lens[i] > 0) == (st[i] == OK)
                    if kind in ("ones", "falling"):
                        assert np.all(st == OVERFLOW)
            finally:
                ds.free()
    finally:
        f.close()


# ---- 9. pf_turn_paths
def model_row(cost, wt, cells, L, cap, R, C):
    """(total, turns, bad) of one row by the rule."""
    if L < 1 or L > cap:
        return np.nan, 0, 0
    row = [int(v) for v in cells[:L]]
    if L == 1:
        return (0.0, 0, -1) if 0 <= row[0] < R * C else (np.nan, 0, 0)
    for i, (a, b) in enumerate(zip(row[:-1], row[1:])):
        ok = 0 <= a < R * C and 0 <= b < R * C
        if ok:
            ok = max(abs(b // C - a // C), abs(b % C - a % C)) == 1
        if not ok:
            return np.nan, 0, i
    total, turns = tk.path_cost(cost, row, C, wt)
    return total, turns, -1


def test_turn_paths_rows():
    g = gio.grid("g256")[0]
    R, C = g.shape
    cost = ck.cost_of_kind("u50", g.shape, 4)
    f = Field(g, cost)
    e = f.e
    try:
        for dcost, hc, wt in ((f.dcost, cost, 0.3), (None, None, 2.0 ** 20), (f.dcost, cost, 0.0)):
            # A* rows where the solver left them
            rnd = np.random.default_rng(12)
            free = np.flatnonzero(g.reshape(-1) != 1)
            n, cap = 40, e.default_path_cap()
            s, t = rnd.choice(free, n).astype(np.int32), rnd.choice(free, n).astype(np.int32)
            ds, dt = e.put(s), e.put(t)
            dc, dl, dst = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
            tb, nb, bb = e.buf(n, np.float64), e.buf(n, np.int32), e.buf(n, np.int32)
            e.astar_batch(0, ds, dt, n, cap, dc, dl, dst)
            e.turn_paths(dcost, wt, n, cap, dc, dl, tb, nb, bb)
            cells, lens, tot, turns, bad = dc.download().reshape(n, cap), dl.download(), tb.download(), nb.download(), bb.download()
            assert (lens > 1).sum() >= 20
            for i in range(n):
                wtot, wturns, wb = model_row(hc, wt, cells[i], int(lens[i]), cap, R, C)
                assert bad[i] == wb and turns[i] == wturns and (tot[i] == wtot or (np.isnan(wtot) and np.isnan(tot[i]))), i
                if wb == -1:
                    assert turns[i] == tk.count_turns(cells[i, :lens[i]].tolist(), C)
            assert turns.max() >= 3
            # a snake of king moves: rows of exactly cap and cap - 1 cells, one cell, none; and the bad rows
            cap = 130
            snake = np.array([(i // 3) * C + 5 + (i % 3 if (i // 3) % 2 == 0 else 2 - i % 3) for i in range(cap)], np.int32)
            assert model_row(hc, wt, snake, cap, cap, R, C)[2] == -1
            rows = [(snake, cap), (snake, cap - 1), (snake, 1), (snake, 0), (snake, 65), (snake, 66), (snake, 2), (snake, cap + 1), (snake, -3)]
            for at in (0, 64, cap - 2):                                   # a non-adjacent step at the start, in the middle (a second trip), at the end
                b = snake.copy()
                b[at + 1:] += 7
                rows.append((b, cap))
            for at, v in ((5, R * C), (0, -1), (cap - 1, 2 ** 31 - 1), (70, -2 ** 31)):    # a cell id outside the grid
                b = snake.copy()
                b[at] = v
                rows.append((b, cap))
            same = snake.copy()
            same[9] = same[8]                                             # a step that does not move
            wrap = np.array([C - 1, C, C + 1], np.int32)                  # consecutive ids across a row end: no king move
            rows += [(same, cap), (np.concatenate([wrap, snake[:cap - 3]]), 3), (np.array([R * C] + [0] * (cap - 1), np.int32), 1)]
            cells = np.array([r for r, _ in rows], np.int32)
            lens = [L for _, L in rows]
            tot, turns, bad = run_turn_paths(e, dcost, wt, cells, lens, cap)
            for i, (r, L) in enumerate(rows):
                wtot, wturns, wb = model_row(hc, wt, r, L, cap, R, C)
                assert bad[i] == wb and turns[i] == wturns and (tot[i] == wtot or (np.isnan(wtot) and np.isnan(tot[i]))), (i, L, bad[i], wb, tot[i], wtot)
            assert list(bad[9:12]) == [0, 64, cap - 2] and list(bad[12:16]) == [4, 0, cap - 2, 69] and bad[16] == 8 and bad[17] == 0 and bad[18] == 0
            assert tot[2] == 0.0 and bad[2] == -1 and bad[3] == 0 and np.isnan(tot[3]) and turns[0] == tk.count_turns(snake.tolist(), C) > 60
            # n == 0 launches nothing; the first row alone leaves the others untouched
            tot, turns, bad = run_turn_paths(e, dcost, wt, cells[:2], lens[:2], cap, n=0)
            assert np.all(tot == CANARY) and np.all(bad == CANARY) and np.all(turns == CANARY)
            tot, turns, bad = run_turn_paths(e, dcost, wt, cells[:2], lens[:2], cap, n=1)
            assert bad[0] == -1 and bad[1] == CANARY and tot[1] == CANARY and turns[1] == CANARY and tot[0] == model_row(hc, wt, snake, cap, cap, R, C)[0]
            for b in (ds, dt, dc, dl, dst, tb, nb, bb):
                b.free()
    finally:
        f.close()


# ---- 10. through the class
def test_the_class_end_to_end_on_a_seeded_map():
    import pathfit
    g = wc.seeded(45, 100, 0.22, 31)
    cost = ck.cost_of_kind("u50", g.shape, 9)
    src = free_cells(g, 4, 10)
    sets = [src[:1], src[1:]]
    tf = pathfit.TurnField(g, [[(v // 100, v % 100) for v in s] for s in sets], 0.3, cost=cost)
    try:
        wT, wbest, winfo = tk.fields(g, cost, sets, 0.3, True, True)
        assert same_bits(tf.states, wT) and same_bits(tf.best, wbest) and np.array_equal(tf.info, winfo) and tf.work[0] >= 1
        targets = free_cells(g, 30, 11) + src[:1] + [int(np.flatnonzero(g.reshape(-1) == 1)[0])]
        tp = [(v // 100, v % 100) for v in targets]
        for b in range(2):
            for reverse in (False, True):
                paths = tf.paths(tp, b=b, reverse=reverse)
                tot, turns, bad = tf.path_costs(paths)
                for t, p, x, n, bd in zip(targets, paths, tot, turns, bad):
                    r = tk.route(wT[b], cost, t, 0.3)
                    assert p.cells.tolist() == (r[::-1] if reverse else r)
                    if r and not reverse:
                        assert bd == -1 and x == wbest[b].reshape(-1)[t] and n == tk.count_turns(r, 100)
                        assert tf.heading(b, (t // 100, t % 100)) == min(range(8), key=lambda k: (wT[b].reshape(8, -1)[k, t], k))
                    elif not r:
                        assert bd == 0 and np.isnan(x) and tf.heading(b, (t // 100, t % 100)) is None
        lists = [p.tolist() for p in tf.paths(tp[:5])]
        arrays = [p.cells for p in tf.paths(tp[:5])]
        a, b_, c = tf.path_costs(lists), tf.path_costs(arrays), tf.path_costs(tf.paths(tp[:5]))
        assert all(same_bits(x, y) and same_bits(x, z) for x, y, z in zip(a[:1], b_[:1], c[:1])) and np.array_equal(a[1], c[1]) and np.array_equal(b_[2], c[2])
        with pytest.raises(pathfit.PathfitError, match="^TurnField: .* paths hold more than path_cap = 2 cells"):
            tf.paths(tp[:5], path_cap=2)
    finally:
        tf.close()


@pytest.mark.parametrize("name", ["fig7", "g256"])
def test_solver_results_against_the_optimum(name):
    """A*, Dijkstra and one seeded MPA result at turn weight 0.3: the rule's cost of the solver's path is at least best[target], and
    pf_score_batch's length + w_t * turns lies within 4 L 2^-53 total of it (the two sums differ by at most 3 L roundings: L - 1
    additions each way, the product and the final addition, each relative 2^-53 of a partial sum <= total)."""
    import pathfit
    g, s, t = gio.grid(name)
    C = g.shape[1]
    wt = 0.3
    e = pathfit.Engine(g)
    tf = pathfit.TurnField(g, [(s // C, s % C)], wt, engine=e)
    try:
        opt = float(tf.best[0].reshape(-1)[t])
        assert np.isfinite(opt)
        kw = dict(turn_penalty_factor=wt, safety_penalty_factor=0.8, min_safe_distance=1.8)
        results = [pathfit.AStarSolver(g, engine=e, **kw).solve(), pathfit.DijkstraSolver(g, engine=e, **kw).solve(),
                   pathfit.MPA(g, 24, 4, seed=3, engine=e, diagonal_obstacle_penalty=100.0, **kw).solve_path_planning()]
        for path, length, turns, _, _, _ in results:
            path = [tuple(int(v) for v in p) for p in path]
            assert path and path[0] == (s // C, s % C) and path[-1] == (t // C, t % C)
            tot, n, bad = tf.path_costs([path])
            L = len(path)
            assert bad[0] == -1 and n[0] == turns and tot[0] >= opt
            assert abs((length + wt * turns) - tot[0]) <= 4 * L * 2.0 ** -53 * tot[0], (length, turns, tot[0])
        route = tf.paths([(t // C, t % C)])[0]
        tot, n, bad = tf.path_costs([route])
        assert tot[0] == opt and bad[0] == -1 and len(route.cells) >= 2
    finally:
        tf.close()
        e.close()


# ---- 11. argument errors of the raw ABI
def test_argument_errors_leave_every_output_untouched():
    from pathfit._lib import PathfitError
    g = wc.seeded(20, 70, 0.2, 3)
    wall, free = np.flatnonzero(g.reshape(-1) == 1), np.flatnonzero(g.reshape(-1) != 1)
    f = Field(g, ck.cost_of_kind("u50", g.shape, 1))
    e, RC, L = f.e, g.size, f.e.L
    sb, bb, ib = between_canaries(e, 16 * RC, np.float64), between_canaries(e, 2 * RC, np.float64), between_canaries(e, 8, np.int64)
    xb = between_canaries(e, 64, np.int32)
    sv, bv, iv, xv = view(e, sb, 16 * RC, np.float64), view(e, bb, 2 * RC, np.float64), view(e, ib, 8, np.int64), view(e, xb, 64, np.int32)

    def untouched():
        return all(np.all(inner(b, "x") == CANARY) for b in (sb, bb, ib, xb))

    def raw(cost, wt, B, off, src, states, best, info, h=None):
        off, src = np.asarray(off, np.int32), np.asarray(src, np.int32)
        return L.pf_turn_field(e.h if h is None else None, 1, 1, cost, wt, B, off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, states, best, info)
    try:
        s0, c = int(free[0]), f.dcost.ptr
        assert raw(c, 0.3, 1, [0, 1], [s0], None, bv.ptr, iv.ptr) == -1 and b"must not be null" in L.pf_last_error(e.h)
        assert raw(c, 0.3, 1, [0, 1], [s0], sv.ptr, None, iv.ptr) == -1
        assert raw(c, 0.3, 1, [], [s0], sv.ptr, bv.ptr, iv.ptr) == -1 and raw(c, 0.3, 1, [0, 1], [], sv.ptr, bv.ptr, iv.ptr) == -1
        assert raw(c, 0.3, -1, [0, 1], [s0], sv.ptr, bv.ptr, iv.ptr) == -1 and raw(c, 0.3, 0, [0], [s0], sv.ptr, bv.ptr, iv.ptr) == -1
        assert raw(c, 0.3, 2, [0, 1, 1], [s0], sv.ptr, bv.ptr, iv.ptr) == -1                     # an empty set
        assert raw(c, 0.3, 1, [0, 2], [s0, RC], sv.ptr, bv.ptr, iv.ptr) == -1 and b"outside the grid" in L.pf_last_error(e.h)
        assert raw(c, 0.3, 1, [0, 2], [-1, s0], sv.ptr, bv.ptr, iv.ptr) == -1
        assert raw(c, 0.3, 1, [0, 1], [s0], sv.ptr, bv.ptr, iv.ptr, h=0) == -2
        for wt in (-1e-300, -1.0, 2.0 ** 20 + 1, np.nan, np.inf, -np.inf):
            assert raw(c, wt, 1, [0, 1], [s0], sv.ptr, bv.ptr, iv.ptr) == -1 and b"pf_turn_field: bad arguments (the turn weight" in L.pf_last_error(e.h), wt
            assert raw(None, wt, 1, [0, 1], [s0], sv.ptr, bv.ptr, iv.ptr) == -1
            assert L.pf_turn_field_paths(e.h, c, wt, 2, sv.ptr, 1, xv.ptr, xv.ptr, 0, 4, xv.ptr, xv.ptr, xv.ptr) == -1
            assert L.pf_turn_paths(e.h, c, wt, 1, 4, xv.ptr, xv.ptr, bv.ptr, xv.ptr, xv.ptr) == -1
        assert L.pf_turn_field_work(e.h, None) == -1 and L.pf_turn_field_work(None, None) == -2
        P, Q = L.pf_turn_field_paths, L.pf_turn_paths
        assert P(None, c, 0.3, 2, sv.ptr, 1, xv.ptr, xv.ptr, 0, 4, xv.ptr, xv.ptr, xv.ptr) == -2 and Q(None, c, 0.3, 1, 4, xv.ptr, xv.ptr, bv.ptr, xv.ptr, xv.ptr) == -2
        assert P(e.h, c, 0.3, 0, sv.ptr, 1, xv.ptr, xv.ptr, 0, 4, xv.ptr, xv.ptr, xv.ptr) == -1 and P(e.h, c, 0.3, 2, sv.ptr, -1, xv.ptr, xv.ptr, 0, 4, xv.ptr, xv.ptr, xv.ptr) == -1
        assert P(e.h, c, 0.3, 2, sv.ptr, 1, xv.ptr, xv.ptr, 0, 0, xv.ptr, xv.ptr, xv.ptr) == -1 and P(e.h, c, 0.3, 2, None, 1, xv.ptr, xv.ptr, 0, 4, xv.ptr, xv.ptr, xv.ptr) == -1
        for hole in range(5):
            args = [xv.ptr] * 5
            args[hole] = None
            assert P(e.h, c, 0.3, 2, sv.ptr, 1, args[0], args[1], 0, 4, args[2], args[3], args[4]) == -1, hole
            args = [xv.ptr, xv.ptr, bv.ptr, xv.ptr, xv.ptr]
            args[hole] = None
            assert Q(e.h, c, 0.3, 1, 4, *args) == -1, hole
        assert Q(e.h, c, 0.3, -1, 4, xv.ptr, xv.ptr, bv.ptr, xv.ptr, xv.ptr) == -1 and Q(e.h, c, 0.3, 1, 0, xv.ptr, xv.ptr, bv.ptr, xv.ptr, xv.ptr) == -1
        assert P(e.h, c, 0.3, 2, sv.ptr, 0, xv.ptr, xv.ptr, 0, 4, xv.ptr, xv.ptr, xv.ptr) == 0 and Q(e.h, c, 0.3, 0, 4, xv.ptr, xv.ptr, bv.ptr, xv.ptr, xv.ptr) == 0
        assert untouched()
        # a bad cost on a free cell: refused by the validation kernel, before any output is written
        where = int(free[len(free) // 2])
        for v in (0.5, 2.0 ** 20 + 1, np.nan, np.inf, -np.inf, 0.0, -4.0):
            bad = f.cost.copy()
            bad.reshape(-1)[where] = v
            f.dcost.upload(bad.reshape(-1))
            with pytest.raises(PathfitError, match=rf"pf_turn_field: bad arguments \(the cost of the free cell \({where // 70}, {where % 70}\)"):
                e.turn_field(f.dcost, 0.3, [0, 1, 2], [s0, int(free[-1])], sv, bv, 1, 1, iv)
            assert raw(c, 0.3, 2, [0, 1, 2], [s0, int(free[-1])], sv.ptr, bv.ptr, iv.ptr) == -1
            assert untouched(), v
        # garbage on obstacle cells is accepted and changes nothing
        junk = f.cost.copy()
        junk.reshape(-1)[wall] = np.resize([np.nan, -1.0, np.inf, 0.0, 1e300, -np.inf], len(wall))
        f.dcost.upload(junk.reshape(-1))
        sets = [[s0], [int(free[-1]), int(wall[0])]]
        e.turn_field(f.dcost, 0.3, *ck.csr(sets), sv, bv, 1, 1, iv)
        wT, wbest, winfo = tk.fields(g, f.cost, sets, 0.3, 1, 1)
        assert same_bits(inner(sb, "T").reshape(wT.shape), wT) and same_bits(inner(bb, "best").reshape(wbest.shape), wbest)
        assert np.array_equal(inner(ib, "info").reshape(2, 4), winfo) and np.all(inner(xb, "x") == CANARY)
    finally:
        for b in (sb, bb, ib, xb):
            b.free()
        f.close()
