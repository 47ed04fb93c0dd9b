"""Cost fields on the device (pf_cost_field / pf_cost_field_parents / pf_cost_paths, pathfit.CostField, Clearance.cost_map) against
the model of tests/cost_checkers.py (a heap Dijkstra with (g, cell id) keys, pinned by tests/test_cost_checkers.py against random-order
sweeps and the field-only parent rule).  Every comparison is exact equality -- labels bit for bit --; every output lies between
canary words."""
import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc
import golden_io as gio
import thin_maps
import widest_checkers as wc

pytestmark = pytest.mark.gpu

CANARY = -77
PCANARY = 179                                                        # no parent code
PAD = 64
TW, TH = 64, 16                                                      # the kernel's tile (PF_WD_TW x PF_WD_TH)


def between_canaries(e, n, dtype, canary=CANARY):
    return e.put(np.full(n + 2 * PAD, canary, dtype))


def inner(buf, tag, canary=CANARY):
    a = buf.download()
    assert np.all(a[:PAD] == canary) and np.all(a[len(a) - PAD:] == canary), tag
    return a[PAD:len(a) - PAD]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class Field:
    """An engine on a map and a cost map in HBM."""

    def __init__(self, g, cost):
        from pathfit.engine import Engine
        self.g, self.e = np.asarray(g), Engine(g)
        self.dcost = self.e.buf(self.g.size, np.float64)
        self.set_cost(cost)

    def set_cost(self, cost):
        self.cost = np.ascontiguousarray(cost, np.float64)
        self.dcost.upload(self.cost.reshape(-1))
        return self

    def run(self, sets, ad, rs, want_info=True, want_parents=True):
        """One raw field call and one raw parent call, every output between canaries -> (D [B, R, C], info [B, 4] or None, parents)."""
        from pathfit.engine import _View
        e, B, RC = self.e, len(sets), self.g.size
        off, src = ck.csr(sets)
        db, ib = between_canaries(e, B * RC, np.float64), between_canaries(e, 4 * B, np.int64)
        pb = between_canaries(e, B * RC, np.uint8, PCANARY)
        try:
            dview = _View(e, db.at(PAD), B * RC, np.float64)
            e.cost_field(self.dcost, off, src, dview, ad, rs, _View(e, ib.at(PAD), 4 * B, np.int64) if want_info else None)
            assert e.last_kernel_ms() > 0
            self.work = work = e.cost_field_work()
            assert work[3] == 0 and work[0] <= work[1] and (work[0] > 0) == (work[1] > 0)
            D, info = inner(db, "D").reshape((B,) + self.g.shape), inner(ib, "info").reshape(B, 4)
            if not want_info:
                assert np.all(info == CANARY)
            P = None
            if want_parents:
                e.cost_field_parents(self.dcost, B, dview, _View(e, pb.at(PAD), B * RC, np.uint8), ad, rs)
                P = inner(pb, "parents", PCANARY).reshape((B,) + self.g.shape)
            return D, (info if want_info else None), P
        finally:
            for b in (db, ib, pb):
                b.free()

    def check(self, sets, policies=ck.POLICIES, tag=None, want_info=(True,)):
        for ad, rs in policies:
            want, wpar, winfo = ck.fields(self.g, self.cost, sets, ad, rs)
            for wi in want_info:
                D, info, P = self.run(sets, ad, rs, wi)
                assert same_bits(D, want), (tag, self.g.shape, ad, rs, "D", np.argwhere(D != want)[:4])
                assert info is None or np.array_equal(info, winfo), (tag, self.g.shape, ad, rs, info, winfo)
                assert np.array_equal(P, wpar), (tag, self.g.shape, ad, rs, "parents", np.argwhere(P != wpar)[:4])

    def close(self):
        self.e.close()


def free_cells(g, n, seed):
    free = np.flatnonzero(np.asarray(g).reshape(-1) != 1)
    return [int(v) for v in np.random.default_rng(seed).choice(free, min(n, len(free)), replace=False)]


def check_map(g, sets, kinds=("ones", "int14", "u50"), policies=ck.POLICIES, want_info=(True,), tag=None, seed=0):
    f = Field(g, np.ones(np.asarray(g).shape))
    try:
        for i, kind in enumerate(kinds):
            f.set_cost(ck.cost_of_kind(kind, f.g.shape, seed + i)).check(sets, policies, (tag, kind), want_info)
    finally:
        f.close()


# ---- 1. golden and thin maps
@pytest.mark.parametrize("name", ["fig7", "fig13", "img1"])
def test_golden_20x20_maps(name):
    g, s, t = gio.grid(name)
    check_map(g, [[s], [t], [s, t]], kinds=("ones", "int14", "u1", "u50", "u1e6"), want_info=(True, False))


@pytest.mark.parametrize("R, C", thin_maps.SHAPES)
def test_thin_maps(R, C):
    for ob in (False, True):
        if not ob or thin_maps.has_obstacle_version(R, C):
            g, s, t = thin_maps.thin_map(R, C, ob)
            check_map(g, [[s], [t], [s, t]], want_info=(True, False), tag=ob, seed=R + C)


# ---- 2. c == 1: the distance fields' rows and parents, on the same handle
def unit_cost_case(g, sets, policies):
    f = Field(g, np.ones(np.asarray(g).shape))
    e, B, RC = f.e, len(sets), f.g.size
    off, src = ck.csr(sets)
    mb, mp = e.buf(B * RC, np.float64), e.buf(B * RC, np.uint8)
    try:
        for ad, rs in policies:
            D, _, P = f.run(sets, ad, rs)
            e.dist_field_merged(off, src, mb, ad, rs)
            e.dist_field_parents(B, mb, mp, ad, rs)
            assert same_bits(D.reshape(-1), mb.download()), (f.g.shape, ad, rs)
            assert np.array_equal(P.reshape(-1), mp.download()), (f.g.shape, ad, rs)
    finally:
        mb.free()
        mp.free()
        f.close()


def test_unit_cost_is_the_distance_field_fig7():
    g, s, t = gio.grid("fig7")
    unit_cost_case(g, [[s], [t], [s, t]], ck.POLICIES)


def test_unit_cost_is_the_distance_field_g256():
    g, s, t = gio.grid("g256")
    unit_cost_case(g, [[s], [s, t] + free_cells(g, 5, 2)], [(1, 1), (0, 0)])


def test_unit_cost_is_the_distance_field_130x200():
    g = wc.seeded(130, 200, 0.25, 13)
    unit_cost_case(g, [free_cells(g, 1, 3), free_cells(g, 4, 4)], [(1, 1), (1, 0), (0, 1)])


# ---- 3. sizes about the tile
@pytest.mark.parametrize("C", [TW - 1, TW, TW + 1, 2 * TW + 1])
@pytest.mark.parametrize("R", [TH - 1, TH, TH + 1, 2 * TH + 1])
def test_sizes_about_the_tile(R, C):
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
        for ad, rs in ck.POLICIES:
            f.check([[left], [right]], [(ad, rs)])
            rows[ad, rs] = f.run([[left], [right]], ad, rs)[0]
        free, restricted = rows[1, 0], rows[1, 1]
        assert np.isfinite(free[0].reshape(-1)[right]) and np.isfinite(free[1].reshape(-1)[left])      # through the gap
        assert np.isinf(restricted[0].reshape(-1)[right]) and np.isinf(restricted[1].reshape(-1)[left])
        assert np.isinf(rows[0, 1][0].reshape(-1)[right]) and np.isinf(rows[0, 0][0].reshape(-1)[right])
    finally:
        f.close()


# ---- 4. the schedule's rare path: a tile lowered again by a route through its neighbour
def detour_map(stacked):
    """Two tiles: side by side (16 x 128) or stacked (32 x 64).  The near tile costs 50 a cell, the far tile 1; a band of cost 2^10
    crosses the near tile between the source and the rest of it; a road of cost 1 runs along the first row (column) through the band
    to the far end.  Cells of the near tile beyond the band are cheapest by the road INTO the far tile, through its cheap cells and
    back."""
    if not stacked:
        cost = np.full((16, 128), 50.0)
        cost[:, 64:] = 1.0
        cost[:, 20:41] = 2.0 ** 10
        cost[0, 3:] = 1.0
        return cost, 8 * 128 + 2, 15 * 128 + 62, lambda v: v % 128 >= 64
    cost = np.full((32, 64), 50.0)
    cost[16:, :] = 1.0
    cost[4:10, :] = 2.0 ** 10
    cost[2:, 0] = 1.0
    return cost, 1 * 64 + 8, 14 * 64 + 62, lambda v: v // 64 >= 16


@pytest.mark.parametrize("stacked", [False, True])
def test_a_tile_is_lowered_again_through_its_neighbour(stacked):
    cost, s, probe, in_far_tile = detour_map(stacked)
    g = np.zeros(cost.shape, np.uint8)
    for ad, rs in ((1, 1), (0, 1)):
        want, wpar, _ = ck.fields(g, cost, [[s]], ad, rs)
        chain = fc.trace(wpar[0], probe)
        assert not in_far_tile(probe) and not in_far_tile(s) and any(in_far_tile(v) for v in chain), (ad, rs)   # on the CPU: out and back
    f = Field(g, cost)
    try:
        for ad, rs in ((1, 1), (0, 1)):
            f.check([[s]], [(ad, rs)])
            # the near tile alone is queued in round 1 and is final only after the far tile has run: true under any timing
            assert f.work[0] >= 3 and f.work[1] >= 3, f.work
    finally:
        f.close()


# ---- 5. magnitudes
def test_costs_at_both_bounds():
    g = wc.seeded(33, 70, 0.2, 8)
    cost = np.where(np.random.default_rng(9).random(g.shape) < 0.5, 1.0, 2.0 ** 20)
    f = Field(g, cost)
    try:
        f.check([free_cells(g, 1, 1), free_cells(g, 3, 2)])
        f.set_cost(np.full(g.shape, 2.0 ** 20)).check([free_cells(g, 2, 3)], [(1, 1)])
    finally:
        f.close()


def test_a_corridor_of_4096_cells_at_the_largest_cost():
    g = np.zeros((1, 4096), np.uint8)
    cost = np.full(g.shape, 2.0 ** 20)
    cost[0, 1::3] = 2.0 ** 20 - 0.375
    f = Field(g, cost)
    try:
        D, info, P = f.run([[0]], 1, 1)
        sums, total = [0.0], 0.0
        for v in range(1, 4096):
            total = total + ck.weight(cost.reshape(-1), v - 1, v, 0)
            sums.append(total)
        assert same_bits(D.reshape(-1), np.array(sums)) and list(info[0]) == [1, 4096, 4095, 0]
        assert np.all(P.reshape(-1)[1:] == 0) and P.reshape(-1)[0] == ck.SOURCE
        assert 4096 // TW <= f.work[0] <= 4096 // TW + 2, f.work          # about one launch per tile crossed
        f.check([[4095], [0, 2048]], [(1, 1)])
    finally:
        f.close()


def test_ties_everywhere():
    g = np.zeros((40, 70), np.uint8)
    for kind, seed in (("int14", 1), ("ones", 2)):
        f = Field(g, ck.cost_of_kind(kind, g.shape, seed))
        try:
            f.check([[20 * 70 + 35], [0, 39 * 70 + 69, 17]])
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
        f.check(sets, want_info=(True, False))
        D, info, P = f.run(sets, 1, 1)
        assert list(info[0][:1]) == [1] and info[1][0] == 2 and list(info[2]) == [0, 0, -1, 0] and list(info[5]) == [0, 0, -1, 0]
        assert np.all(np.isinf(D[2])) and np.all(P[2] == ck.NONE) and info[3][1] == 5 * 7 and np.isfinite(D[3]).sum() == 35
    finally:
        f.close()
    check_map(np.zeros((21, 67), np.uint8), [[0], [20 * 67 + 66, 5]], kinds=("u50", "int14"), policies=[(1, 1), (0, 1)])   # no obstacle at all


def test_a_300x517_map():
    g = wc.seeded(300, 517, 0.2, 77)
    check_map(g, [free_cells(g, 1, 1), free_cells(g, 6, 2)], kinds=("u50",), policies=[(1, 1)], seed=3)


# ---- 7. determinism, update_grid, refresh
def test_five_runs_are_bit_equal():
    g = wc.seeded(70, 150, 0.15, 4)
    f = Field(g, ck.cost_of_kind("u1e6", g.shape, 1))
    try:
        sets = [free_cells(g, 2, 1), free_cells(g, 1, 2)]
        first = f.run(sets, 1, 1)
        for _ in range(4):
            again = f.run(sets, 1, 1)
            assert same_bits(again[0], first[0]) and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    finally:
        f.close()


def test_refresh_after_update_grid_and_with_a_new_cost_map():
    import pathfit
    g = np.zeros((24, 90), np.uint8)
    g[:, 45] = 1                                                      # a wall without a door
    cost = ck.cost_of_kind("u50", g.shape, 2)
    e = pathfit.Engine(g)
    cf = pathfit.CostField(g, cost, [[(3, 3)], [(20, 80), (3, 3)]], engine=e)
    try:
        sets = [[3 * 90 + 3], [20 * 90 + 80, 3 * 90 + 3]]
        want = ck.fields(g, cost, sets, True, True)
        assert same_bits(cf.fields, want[0]) and np.array_equal(cf.parents, want[1]) and np.array_equal(cf.info, want[2])
        assert np.isinf(cf.fields[0][:, 46:]).all() and cf.work[0] >= 1 and cf.kernel_ms > 0
        g2 = g.copy()
        g2[11, 45] = 0                                                # a door
        e.update_grid(g2)
        assert cf.refresh() is cf
        want2 = ck.fields(g2, cost, sets, True, True)
        assert same_bits(cf.fields, want2[0]) and np.array_equal(cf.parents, want2[1]) and np.array_equal(cf.info, want2[2])
        assert np.isfinite(cf.fields[0][:, 46:]).all() and not same_bits(want2[0], want[0])
        cost3 = ck.cost_of_kind("int14", g.shape, 3)
        cf.refresh(cost=cost3)
        want3 = ck.fields(g2, cost3, sets, True, True)
        assert same_bits(cf.fields, want3[0]) and np.array_equal(cf.parents, want3[1]) and np.array_equal(cf.owners[1], ck.owners(want3[1][1], sets[1]))
        assert same_bits(cf.cost_device.download().reshape(g.shape), cost3)
    finally:
        cf.close()
        e.close()


# ---- 8. parents and routes, through the class
@pytest.mark.parametrize("ad, rs", [(True, True), (False, False)])
def test_routes_owners_and_path_costs(ad, rs):
    import pathfit
    g = wc.seeded(45, 100, 0.22, 31)
    cost = ck.cost_of_kind("u50", g.shape, 9)
    src = free_cells(g, 5, 10)
    sets = [src[:1], src[1:], src]
    pairs = [[(v // 100, v % 100) for v in s] for s in sets]
    cf = pathfit.CostField(g, cost, pairs, ad, rs)
    try:
        want, wpar, winfo = ck.fields(g, cost, sets, ad, rs)
        assert same_bits(cf.fields, want) and np.array_equal(cf.parents, wpar) and np.array_equal(cf.info, winfo)
        targets = free_cells(g, 40, 11) + src[:2] + [int(np.flatnonzero(g.reshape(-1) == 1)[0])]
        tp = [(v // 100, v % 100) for v in targets]
        for b in range(3):
            own = ck.owners(wpar[b], sets[b])
            assert np.array_equal(cf.owners[b], own)
            assert np.array_equal(cf.territory_sizes(b), [int((own == i).sum()) for i in range(len(sets[b]))])
            paths = cf.paths(tp, b=b)
            assert np.array_equal(cf.chosen, own.reshape(-1)[targets])
            tot, bad = cf.path_costs(paths)
            for t, p, x, bd in zip(targets, paths, tot, bad):
                cells = fc.trace(wpar[b], t)
                assert p.cells.tolist() == cells
                if cells:
                    assert bd == -1 and x == want[b].reshape(-1)[t] and x == ck.path_cost(cost, cells, 100)   # bit for bit the label
                    hop = cf.next_hop(b, (t // 100, t % 100))
                    assert hop == (None if len(cells) == 1 else (cells[-2] // 100, cells[-2] % 100))
                    assert cf.nearest(b, (t // 100, t % 100)) == (int(own.reshape(-1)[t]), float(want[b].reshape(-1)[t]))
                else:
                    assert bd == 0 and np.isnan(x) and cf.nearest(b, (t // 100, t % 100)) == (None, float("inf"))
    finally:
        cf.close()


# ---- 9. pf_cost_paths
def run_cost_paths(e, dcost, cells, lens, cap, n=None):
    from pathfit.engine import _View
    rows = len(lens)
    dc, dl = e.put(np.ascontiguousarray(cells, np.int32)), e.put(np.asarray(lens, np.int32))
    tb, bb = between_canaries(e, rows, np.float64), between_canaries(e, rows, np.int32)
    try:
        e.cost_paths(dcost, rows if n is None else n, cap, dc, dl, _View(e, tb.at(PAD), rows, np.float64), _View(e, bb.at(PAD), rows, np.int32))
        return inner(tb, "total"), inner(bb, "bad")
    finally:
        for b in (dc, dl, tb, bb):
            b.free()


def model_row(cost, cells, L, cap, R, C):
    """(total, bad) of one row by the rule."""
    if L < 1 or L > cap:
        return np.nan, 0
    row = [int(v) for v in cells[:L]]
    if L == 1:
        return (0.0, -1) if 0 <= row[0] < R * C else (np.nan, 0)
    total = 0.0
    for i, (a, b) in enumerate(zip(row[:-1], row[1:])):
        ok = 0 <= a < R * C and 0 <= b < R * C
        if ok:
            dr, dc = b // C - a // C, b % C - a % C
            ok = max(abs(dr), abs(dc)) == 1
        if not ok:
            return np.nan, i
        total = total + ck.weight(cost.reshape(-1), a, b, 4 if dr and dc else 0)
    return total, -1


def test_cost_paths_rows():
    g = gio.grid("g256")[0]
    R, C = g.shape
    cost = ck.cost_of_kind("u50", g.shape, 4)
    f = Field(g, cost)
    e = f.e
    try:
        # A* rows where the solver left them
        rnd = np.random.default_rng(12)
        free = np.flatnonzero(g.reshape(-1) != 1)
        n, cap = 40, e.default_path_cap()
        s, t = rnd.choice(free, n).astype(np.int32), rnd.choice(free, n).astype(np.int32)
        ds, dt = e.put(s), e.put(t)
        dc, dl, dst = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
        tb, bb = e.buf(n, np.float64), e.buf(n, np.int32)
        e.astar_batch(0, ds, dt, n, cap, dc, dl, dst)
        e.cost_paths(f.dcost, n, cap, dc, dl, tb, bb)
        cells, lens, tot, bad = dc.download().reshape(n, cap), dl.download(), tb.download(), bb.download()
        assert (lens > 1).sum() >= 20
        for i in range(n):
            wt, wb = model_row(cost, cells[i], int(lens[i]), cap, R, C)
            assert bad[i] == wb and (tot[i] == wt or (np.isnan(wt) and np.isnan(tot[i]))), i
        # a snake of king moves: rows of exactly cap and cap - 1 cells, one cell, none; and the bad rows
        cap = 130
        snake = np.array([(i // 3) * C + 5 + (i % 3 if (i // 3) % 2 == 0 else 2 - i % 3) for i in range(cap)], np.int32)
        assert model_row(cost, snake, cap, cap, R, C)[1] == -1
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
        tot, bad = run_cost_paths(e, f.dcost, cells, lens, cap)
        for i, (r, L) in enumerate(rows):
            wt, wb = model_row(cost, r, L, cap, R, C)
            assert bad[i] == wb and (tot[i] == wt or (np.isnan(wt) and np.isnan(tot[i]))), (i, L, bad[i], wb, tot[i], wt)
        assert list(bad[9:12]) == [0, 64, cap - 2] and list(bad[12:16]) == [4, 0, cap - 2, 69] and bad[16] == 8 and bad[17] == 0 and bad[18] == 0
        assert tot[2] == 0.0 and bad[2] == -1 and bad[3] == 0 and np.isnan(tot[3])
        # n == 0 launches nothing; the first row alone leaves the others untouched
        tot, bad = run_cost_paths(e, f.dcost, cells[:2], lens[:2], cap, n=0)
        assert np.all(tot == CANARY) and np.all(bad == CANARY)
        tot, bad = run_cost_paths(e, f.dcost, cells[:2], lens[:2], cap, n=1)
        assert bad[0] == -1 and bad[1] == CANARY and tot[1] == CANARY and tot[0] == model_row(cost, snake, cap, cap, R, C)[0]
    finally:
        f.close()


# ---- 10. Clearance.cost_map end to end
def test_clearance_cost_map_on_g256():
    import pathfit
    g, s, _ = gio.grid("g256")
    R, C = g.shape
    e = pathfit.Engine(g)
    cl = pathfit.Clearance(g, engine=e)
    cost = cl.cost_map(margin=3)
    assert cost.shape == g.shape and cost.dtype == np.float64 and cost.min() == 1.0 and cost.max() > 1.0
    cf = pathfit.CostField(g, cost, [(s // C, s % C)], engine=e)
    unit = pathfit.CostField(g, np.ones(g.shape), [(s // C, s % C)], engine=e)
    try:
        held = cf.cost_device.download().reshape(g.shape)
        assert same_bits(held, cost)
        want, wpar, winfo = ck.fields(g, held, [[s]], True, True)
        assert same_bits(cf.fields, want) and np.array_equal(cf.parents, wpar) and np.array_equal(cf.info, winfo)
        reach = np.flatnonzero(np.isfinite(want[0]).reshape(-1))
        targets = [int(v) for v in np.random.default_rng(50).choice(reach, 50, replace=False)]
        tp = [(v // C, v % C) for v in targets]
        routes, short = cf.paths(tp), unit.paths(tp)
        tot, bad = cf.path_costs(routes)
        stot, sbad = cf.path_costs(short)                             # the unit-cost Dijkstra routes, scored under the cost map
        mm = fc.move_masks(g, 1, 1)
        upar = fc.reference_dijkstra(g, mm, s)[1]
        for t, p, q, x, y in zip(targets, routes, short, tot, stot):
            assert p.cells.tolist() == fc.trace(wpar[0], t) and q.cells.tolist() == fc.trace(upar, t)
            assert x == want[0].reshape(-1)[t] and x <= y
            assert ck.path_cost(held, p.cells.tolist(), C) <= ck.path_cost(held, q.cells.tolist(), C) == y   # on the CPU as well
        assert np.all(bad == -1) and np.all(sbad == -1) and (tot < stot).any()
    finally:
        cf.close()
        unit.close()
        cl.close()
        e.close()


# ---- 11. argument errors of the raw ABI
def test_argument_errors_leave_every_output_untouched():
    from pathfit._lib import PathfitError
    from pathfit.engine import _View
    g = wc.seeded(20, 70, 0.2, 3)
    wall, free = np.flatnonzero(g.reshape(-1) == 1), np.flatnonzero(g.reshape(-1) != 1)
    f = Field(g, ck.cost_of_kind("u50", g.shape, 1))
    e, RC = f.e, g.size
    db, ib, pb = between_canaries(e, 2 * RC, np.float64), between_canaries(e, 8, np.int64), between_canaries(e, 2 * RC, np.uint8, PCANARY)
    dv, iv, pv = _View(e, db.at(PAD), 2 * RC, np.float64), _View(e, ib.at(PAD), 8, np.int64), _View(e, pb.at(PAD), 2 * RC, np.uint8)

    def untouched():
        return np.all(inner(db, "D") == CANARY) and np.all(inner(ib, "info") == CANARY) and np.all(inner(pb, "P", PCANARY) == PCANARY)

    def raw(cost, B, off, src, out, info):
        off, src = np.asarray(off, np.int32), np.asarray(src, np.int32)
        return e.L.pf_cost_field(e.h, 1, 1, cost, B, off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, out, info)
    try:
        s0 = int(free[0])
        assert raw(None, 1, [0, 1], [s0], dv.ptr, iv.ptr) == -1 and b"must not be null" in e.L.pf_last_error(e.h)
        assert raw(f.dcost.ptr, 1, [0, 1], [s0], None, iv.ptr) == -1
        assert raw(f.dcost.ptr, 1, [], [s0], dv.ptr, iv.ptr) == -1 and raw(f.dcost.ptr, 1, [0, 1], [], dv.ptr, iv.ptr) == -1
        assert raw(f.dcost.ptr, -1, [0, 1], [s0], dv.ptr, iv.ptr) == -1 and raw(f.dcost.ptr, 0, [0], [s0], dv.ptr, iv.ptr) == -1
        assert raw(f.dcost.ptr, 2, [0, 1, 1], [s0], dv.ptr, iv.ptr) == -1                        # an empty set
        assert raw(f.dcost.ptr, 1, [0, 2], [s0, RC], dv.ptr, iv.ptr) == -1 and b"outside the grid" in e.L.pf_last_error(e.h)
        assert raw(f.dcost.ptr, 1, [0, 2], [-1, s0], dv.ptr, iv.ptr) == -1
        assert e.L.pf_cost_field(None, 1, 1, f.dcost.ptr, 1, None, None, dv.ptr, None) == -2
        assert e.L.pf_cost_field_work(e.h, None) == -1 and e.L.pf_cost_field_work(None, None) == -2
        assert e.L.pf_cost_field_parents(e.h, 1, 1, None, 2, dv.ptr, pv.ptr) == -1 and e.L.pf_cost_field_parents(e.h, 1, 1, f.dcost.ptr, 0, dv.ptr, pv.ptr) == -1
        assert e.L.pf_cost_field_parents(e.h, 1, 1, f.dcost.ptr, 2, None, pv.ptr) == -1 and e.L.pf_cost_field_parents(e.h, 1, 1, f.dcost.ptr, 2, dv.ptr, None) == -1
        assert e.L.pf_cost_paths(e.h, None, 1, 4, dv.ptr, dv.ptr, dv.ptr, dv.ptr) == -1 and e.L.pf_cost_paths(e.h, f.dcost.ptr, -1, 4, dv.ptr, dv.ptr, dv.ptr, dv.ptr) == -1
        assert e.L.pf_cost_paths(e.h, f.dcost.ptr, 1, 0, dv.ptr, dv.ptr, dv.ptr, dv.ptr) == -1 and e.L.pf_cost_paths(e.h, f.dcost.ptr, 1, 4, dv.ptr, dv.ptr, None, dv.ptr) == -1
        assert untouched()
        # a bad cost on a free cell: refused by the validation kernel, before any output is written
        where = int(free[len(free) // 2])
        for v in (0.5, 2.0 ** 20 + 1, np.nan, np.inf, -np.inf, 0.0, -4.0):
            bad = f.cost.copy()
            bad.reshape(-1)[where] = v
            f.dcost.upload(bad.reshape(-1))
            with pytest.raises(PathfitError, match=rf"pf_cost_field: bad arguments \(the cost of the free cell \({where // 70}, {where % 70}\)"):
                e.cost_field(f.dcost, [0, 1, 2], [s0, int(free[-1])], dv, 1, 1, iv)
            assert raw(f.dcost.ptr, 2, [0, 1, 2], [s0, int(free[-1])], dv.ptr, iv.ptr) == -1
            assert untouched(), v
        # garbage on obstacle cells is accepted and changes nothing
        junk = f.cost.copy()
        junk.reshape(-1)[wall] = np.resize([np.nan, -1.0, np.inf, 0.0, 1e300, -np.inf], len(wall))
        f.dcost.upload(junk.reshape(-1))
        sets = [[s0], [int(free[-1]), int(wall[0])]]
        e.cost_field(f.dcost, *ck.csr(sets), dv, 1, 1, iv)
        e.cost_field_parents(f.dcost, 2, dv, pv, 1, 1)
        want, wpar, winfo = ck.fields(g, f.cost, sets, 1, 1)
        assert same_bits(inner(db, "D").reshape(want.shape), want) and np.array_equal(inner(ib, "info").reshape(2, 4), winfo)
        assert np.array_equal(inner(pb, "P", PCANARY).reshape(wpar.shape), wpar)
    finally:
        for b in (db, ib, pb):
            b.free()
        f.close()
