"""Cost-field repair on the device (pf_cost_field_repair, Engine.cost_field_repair, CostField.repair) against a fresh pf_cost_field
call on the same handle afterwards AND the heap Dijkstra of tests/cost_checkers.py on the new map; d_info against the fresh call's;
the words raised against the model of tests/repair_checkers.py (pinned by tests/test_repair_checkers.py).  Every comparison is exact
equality -- labels as 64-bit words --; every output lies between canary words."""
import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc
import golden_io as gio
import repair_checkers as rc
import thin_maps
import widest_checkers as wc

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64
TW, TH = 64, 16                                                      # the kernels' tile (PF_WD_TW x PF_WD_TH)
BIG = float(2 ** 20)


def between_canaries(e, n, dtype, canary=CANARY):
    return e.put(np.full(n + 2 * PAD, canary, dtype))


def inner(buf, tag, canary=CANARY):
    a = buf.download()
    assert np.all(a[:PAD] == canary) and np.all(a[len(a) - PAD:] == canary), tag
    return a[PAD:len(a) - PAD]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class Rig:
    """An engine on a map, a cost map in HBM, and the rows of B sets between canaries, which every repair updates in place."""

    def __init__(self, g, cost, sets):
        from pathfit.engine import Engine, _View
        self.g = np.array(g, np.uint8)
        self.e = Engine(self.g)
        self.sets, self.B, self.RC = sets, len(sets), self.g.size
        self.off, self.src = ck.csr(sets)
        self.cost = np.array(cost, np.float64)
        self.dcost = self.e.put(self.cost.reshape(-1))
        self.db = between_canaries(self.e, self.B * self.RC, np.float64)
        self.rows = _View(self.e, self.db.at(PAD), self.B * self.RC, np.float64)
        self.D = None

    def set_map(self, g, cost):
        g = np.array(g, np.uint8)
        if not np.array_equal(g, self.g):
            self.e.update_grid(g)
        self.g = g
        self.cost = np.array(cost, np.float64)
        self.dcost.upload(self.cost.reshape(-1))

    def shape(self, flat):
        return flat.reshape((self.B,) + self.g.shape)

    def start(self, ad, rs):
        """The rows become a fresh field of the present map."""
        self.e.cost_field(self.dcost, self.off, self.src, self.rows, ad, rs, None)
        self.D = self.shape(inner(self.db, "start"))
        return self.D

    def fresh(self, ad, rs):
        """pf_cost_field from nothing on the same handle, into buffers of its own -> (D, info, kernel ms)."""
        from pathfit.engine import _View
        e, n = self.e, self.B * self.RC
        db, ib = between_canaries(e, n, np.float64), between_canaries(e, 4 * self.B, np.int64)
        try:
            e.cost_field(self.dcost, self.off, self.src, _View(e, db.at(PAD), n, np.float64), ad, rs, _View(e, ib.at(PAD), 4 * self.B, np.int64))
            assert e.cost_field_work()[3] == 0
            return self.shape(inner(db, "fresh D")), inner(ib, "fresh info").reshape(self.B, 4), e.last_kernel_ms()
        finally:
            db.free()
            ib.free()

    def repair(self, changed, ad, rs, want_info=True):
        """One raw repair of the rows in place -> (D, info or None, work)."""
        from pathfit.engine import _View
        e = self.e
        ib = between_canaries(e, 4 * self.B, np.int64)
        try:
            e.cost_field_repair(self.dcost, changed, self.off, self.src, self.rows, ad, rs, _View(e, ib.at(PAD), 4 * self.B, np.int64) if want_info else None)
            assert e.last_kernel_ms() > 0
            work = e.cost_field_work()
            assert work[0] <= work[1] and (work[0] > 0) == (work[1] > 0)
            info = inner(ib, "info").reshape(self.B, 4)
            if not want_info:
                assert np.all(info == CANARY)
            self.D = self.shape(inner(self.db, "D"))
            return self.D, (info if want_info else None), work
        finally:
            ib.free()

    def step(self, g1, c1, ad, rs, changed=None, tag=None, want_info=True):
        """The map becomes (g1, c1) and the rows are repaired: compared with the fresh call afterwards, with the heap, with the fresh
        call's info and with the model's words raised -> work."""
        old = self.D
        if changed is None:
            changed = rc.changed_cells(self.g, self.cost, g1, c1)
        want_raised = sum(len(rc.raised_by_label_order(old[b], g1, c1, self.sets[b], ad, rs)) for b in range(self.B))
        self.set_map(g1, c1)
        D, info, work = self.repair(changed, ad, rs, want_info)
        fD, finfo, _ = self.fresh(ad, rs)
        where = (tag, self.g.shape, ad, rs)
        assert same_bits(D, fD), (where, "fresh", np.argwhere(D != fD)[:4])
        hD, _, hinfo = ck.fields(self.g, self.cost, self.sets, ad, rs)
        assert same_bits(D, hD), (where, "heap", np.argwhere(D != hD)[:4])
        assert np.array_equal(finfo, hinfo) and (info is None or np.array_equal(info, finfo)), (where, info, finfo, hinfo)
        assert work[3] == want_raised, (where, work, want_raised)
        if len(changed) == 0:
            assert work == (0, 0, 0, 0)
        return work

    def close(self):
        self.e.close()


def free_cells(g, n, seed):
    free = np.flatnonzero(np.asarray(g).reshape(-1) != 1)
    return [int(v) for v in np.random.default_rng(seed).choice(free, min(n, len(free)), replace=False)]


def four_changes(g, c, cell, other):
    """From (g, c): `cell` closes, opens again, the cost of `other` rises, then falls to 1 -> the four maps, each built on the last."""
    g, c = np.array(g, np.uint8), np.array(c, np.float64)
    r, k = divmod(int(cell), g.shape[1])
    p, q = divmod(int(other), g.shape[1])
    g1 = g.copy()
    g1[r, k] = 1
    c2 = c.copy()
    c2[p, q] = min(2.0 * c[p, q] + 3.3, BIG)
    c3 = c.copy()
    c3[p, q] = 1.0
    return [(g1, c, "closes"), (g, c, "opens"), (g, c2, "cost rises"), (g, c3, "cost falls")]


def run_steps(g, c, sets, steps, policies=ck.POLICIES, tag=None, want_info=True):
    """Per policy: a fresh field on (g, c), then the steps (g1, c1, label) one after the other -> the works, per policy."""
    rig = Rig(g, c, sets)
    works = {}
    try:
        for ad, rs in policies:
            rig.set_map(g, c)
            rig.start(ad, rs)
            works[ad, rs] = [rig.step(g1, c1, ad, rs, tag=(tag, label), want_info=want_info) for g1, c1, label in steps]
    finally:
        rig.close()
    return works


# ---- 1. small and thin maps
@pytest.mark.parametrize("kind", ["ones", "u50"])
def test_the_golden_20x20_map(kind):
    g, s, t = gio.grid("fig7")
    free = free_cells(g, 6, 1)
    cells = [v for v in free if v not in (s, t)]
    c = ck.cost_of_kind(kind, g.shape, 2)
    works = run_steps(g, c, [[s], [t, s]], four_changes(g, c, cells[0], cells[1]), tag=kind)
    assert all(w[1][3] == 0 for w in works.values())                  # a cell that opens raises nothing


THIN = [(1, 2), (2, 1), (1, 9), (9, 1), (2, 17), (17, 2), (1, 300), (1, 4096), (4096, 1), (2, 4096), (4096, 2)]


@pytest.mark.parametrize("R, C", THIN)
def test_thin_maps(R, C):
    if min(R, C) == 2 and max(R, C) == 4096:
        g, s, t = thin_maps.few_obstacles_map(R, C)
    else:
        g, s, t = thin_maps.thin_map(R, C, max(R, C) >= 9)
    c = ck.cost_of_kind("u50", g.shape, R + C)
    L = R * C
    free = [int(v) for v in np.flatnonzero(np.asarray(g).reshape(-1) != 1) if int(v) != s]
    cell = free[len(free) // 5]                                       # near the source: most of a corridor loses its support
    other = free[len(free) // 2] if len(free) > 1 else cell
    works = run_steps(g, c, [[s]] if L < 9 else [[s], [t, s]], four_changes(g, c, cell, other), tag=(R, C))
    if min(R, C) == 1 and L >= 9:
        assert all(w[0][3] > 0 for w in works.values())               # a closed corridor cell always raises what lies behind it


# ---- 2. tile edges
@pytest.mark.parametrize("C", [TW - 1, TW, TW + 1, 2 * TW])
@pytest.mark.parametrize("R", [TH - 1, TH, TH + 1])
def test_sizes_about_the_tile(R, C):
    g = wc.seeded(R, C, 0.2, 100 * R + C)
    for j, m in enumerate((g, wc.shifted_cols(wc.shifted_rows(g)))):
        m = m.copy()
        rows, cols = m.shape
        spots = [(min(rows - 1, TH - 1), min(cols - 1, TW - 1)), (min(rows - 1, TH), min(cols - 1, TW)), (rows // 2, cols // 2)]
        src = [v for v in free_cells(m, 4, R + C + j) if divmod(v, cols) not in spots]
        c = ck.cost_of_kind("u50", m.shape, R * C + j)
        steps, cur = [], m
        for r, k in spots:                                            # each spot toggles; the next step builds on it
            nxt = cur.copy()
            nxt[r, k] ^= 1
            steps.append((nxt, c, (r, k)))
            cur = nxt
        run_steps(m, c, [src[:1], src], steps, policies=[(1, 1), (0, 0)] if j == 0 else [(1, 0), (0, 1)], tag=(R, C, j))


def test_a_changed_cell_on_a_tile_corner_border_and_interior():
    R, C = 2 * TH + 1, 2 * TW + 2
    g = wc.seeded(R, C, 0.15, 9)
    spots = [(TH - 1, TW - 1), (TH, TW), (TH - 1, TW), (TH, TW - 1), (TH - 1, 70), (TH, 70), (20, TW - 1), (20, TW), (24, 100), (0, 0), (R - 1, C - 1)]
    for r, k in spots:
        g[r, k] = 0
    c = ck.cost_of_kind("u50", g.shape, 4)
    src = [v for v in free_cells(g, 3, 5) if divmod(v, C) not in spots]
    steps = []
    for r, k in spots:
        closed = g.copy()
        closed[r, k] = 1
        steps += [(closed, c, ("closes", r, k)), (g, c, ("opens", r, k))]
    run_steps(g, c, [src[:1], src], steps, tag="spots")


def test_a_diagonal_gap_across_a_tile_corner():
    r, c = 2 * TH, TW                                                 # the four cells about (r, c) lie in four tiles
    g = wc.corner_gap(4 * TH + 3, 2 * TW + 5, r, c)
    C = g.shape[1]
    shut = g.copy()
    shut[r - 1, c] = 1                                                # one of the two gap cells closed: the sides are apart under every policy
    cost = ck.cost_of_kind("u50", g.shape, 5)
    left, right = (r + 5) * C + 3, 3 * C + c + 9
    rig = Rig(shut, cost, [[left], [right]])
    try:
        for ad, rs in ck.POLICIES:
            rig.set_map(shut, cost)
            D = rig.start(ad, rs)
            assert np.isinf(D[0].reshape(-1)[right]) and np.isinf(D[1].reshape(-1)[left])
            w = rig.step(g, cost, ad, rs, tag="gap opens")
            through = np.isfinite(rig.D[0].reshape(-1)[right])
            assert through == ((ad, rs) == (1, 0)) and np.isfinite(rig.D[1].reshape(-1)[left]) == through   # the free and the restricted policy disagree
            assert w[3] == 0
            w = rig.step(shut, cost, ad, rs, tag="gap closes")
            assert (w[3] > 1000) == through and np.isinf(rig.D[0].reshape(-1)[right])
    finally:
        rig.close()


# ---- 3. the corner-rule map of the checker's second rejection
def test_the_corner_rule_map():
    g0, g1, c, sources, _ = rc.corner_rule_case()
    works = run_steps(g0, c, [sources], [(g1, c, "x closes"), (g0, c, "x opens")])
    assert works[1, 1][0][3] > works[1, 0][0][3] == 2                 # x and (1, 2) behind it -- and, restricted, the labels behind the diagonal
    big = np.zeros((2 * TH + 2, 2 * TW + 2), np.uint8)                # the same four cells about a tile corner
    big2 = big.copy()
    big2[TH, TW] = 1
    src = [TH * big.shape[1] + TW - 1]
    works = run_steps(big, np.ones(big.shape), [src], [(big2, np.ones(big.shape), "x closes"), (big, np.ones(big.shape), "x opens")])
    assert works[1, 1][0][3] > works[1, 0][0][3] > 0


# ---- 4. doors
def test_a_door_that_seals_a_room_and_opens_again():
    g, door, inside, sealed = rc.sealed_room_map()
    C = g.shape[1]
    shut = g.copy()
    shut.reshape(-1)[door] = 1
    for kind in ("ones", "u50"):
        c = ck.cost_of_kind(kind, g.shape, 8)
        works = run_steps(g, c, [[C + 1]], [(shut, c, "door closes"), (g, c, "door opens")], policies=[(1, 1), (0, 0)], tag=kind)
        for w in works.values():
            assert w[0][3] > 500 and w[1][3] == 0 and w[1][2] > 500   # a room raised; then nothing raised and a room lowered


def test_a_closing_in_a_sealed_room_raises_nothing():
    g, door, inside, sealed = rc.sealed_room_map()
    C = g.shape[1]
    g1 = g.copy()
    g1.reshape(-1)[sealed] = 1
    c = ck.cost_of_kind("u50", g.shape, 8)
    rig = Rig(g, c, [[C + 1]])
    try:
        for ad, rs in ck.POLICIES:
            rig.set_map(g, c)
            before = rig.start(ad, rs).copy()
            w = rig.step(g1, c, ad, rs, tag="sealed")
            assert w[3] == 0 and w[2] == 0 and same_bits(rig.D, before)
    finally:
        rig.close()


def test_a_long_corridor_needs_a_launch_per_tile():
    g, src, x = rc.long_corridor(200)
    c = np.ones(g.shape)
    g1 = g.copy()
    g1[0, x] = 1
    need = rc.min_raise_launches(list(range(2, 200)), [x], 1, 200)
    assert need == 4
    works = run_steps(g, c, [[src]], [(g1, c, "closes"), (g, c, "opens")])
    for w in works.values():
        assert w[0][3] == 199 and w[0][0] >= need + 1                 # the raise launches any timing needs, and one lower launch
        assert w[1][3] == 0 and w[1][2] == 199 and w[1][0] >= 1 + 4   # one raise launch, then the corridor again tile by tile


def test_a_serpentine_loses_its_tail_across_three_tiles():
    g = fc.serpentine(41)                                             # rows 0, 2, .., 40: the corridor crosses three tiles of 16 rows
    c = ck.cost_of_kind("u50", g.shape, 6)
    g1 = g.copy()
    g1[0, 5] = 1
    old = rc.fresh(g, c, [0], 1, 1)
    gone = rc.raised_by_label_order(old, g1, c, [0], 1, 1)
    need = rc.min_raise_launches(gone, [5], 41, 41)
    assert need >= 3 and len(rc.tiles_of(gone, 41)) >= 3
    works = run_steps(g, c, [[0]], [(g1, c, "closes"), (g, c, "opens")])
    for w in works.values():
        assert w[0][0] >= need + 1 and w[0][3] == len(gone)


# ---- 5. costs
def test_costs_at_the_bounds():
    g = wc.seeded(30, 100, 0.15, 12)
    rnd = np.random.default_rng(3)
    c = np.where(rnd.random(g.shape) < 0.5, 1.0, BIG)
    cells = free_cells(g, 4, 2)
    src, a, b = cells[0], cells[1], cells[2]
    c.reshape(-1)[a], c.reshape(-1)[b] = 1.0, BIG
    up, down = c.copy(), c.copy()
    up.reshape(-1)[a] = BIG
    down.reshape(-1)[a], down.reshape(-1)[b] = BIG, 1.0
    run_steps(g, c, [[src]], [(g, up, "1 -> 2^20"), (g, down, "2^20 -> 1")] + four_changes(g, down, cells[3], a)[:2], policies=[(1, 1), (0, 0)])


@pytest.mark.parametrize("kind", ["u1e6", "int14"])
def test_non_dyadic_costs_and_ties(kind):
    g = wc.seeded(40, 140, 0.2, 17)
    c = ck.cost_of_kind(kind, g.shape, 5)
    cells = free_cells(g, 3, 8)
    g1, c1 = rc.seeded_change(g, c, kind, 9, 21, keep=cells[:1])
    g2, c2 = rc.seeded_change(g1, c1, kind, 9, 22, keep=cells[:1])
    run_steps(g, c, [cells[:1], cells], [(g1, c1, "nine"), (g2, c2, "nine more"), (g, c, "back")], policies=[(1, 1), (1, 0)], tag=kind)


def test_a_4096_cell_corridor_at_the_largest_cost():
    g = np.zeros((1, 4096), np.uint8)
    c = np.full(g.shape, BIG)
    c1 = c.copy()
    c1[0, 1000] = 1.0
    works = run_steps(g, c, [[0]], [(g, c1, "one cost falls"), (g, c, "and rises")], policies=[(1, 1), (0, 0)])
    for w in works.values():
        assert w[0][3] == w[1][3] == 4096 - 1000                      # the cell and everything behind it: no label matches the new weight


def test_unit_costs_on_an_open_map():
    g = np.zeros((40, 150), np.uint8)
    c = np.ones(g.shape)
    g1 = g.copy()
    g1[20, 3] = 1
    g2 = g1.copy()
    g2[5:35, 75] = 1
    works = run_steps(g, c, [[20 * 150 + 2]], [(g1, c, "next to the source"), (g2, c, "a wall"), (g, c, "all open")])
    assert all(w[0][3] >= 1 and w[2][3] == 0 for w in works.values())  # the closed cell goes at least; opening everything raises nothing


# ---- 6. sources and sets
@pytest.mark.parametrize("B", [1, 3, 70])
def test_many_sets_in_one_call(B):
    g = wc.seeded(37, 90, 0.2, 21)
    rnd = np.random.default_rng(B)
    free = np.flatnonzero(g.reshape(-1) != 1)
    sets = [[int(v) for v in rnd.choice(free, int(rnd.integers(1, 5)))] for _ in range(B)]
    c = ck.cost_of_kind("u50", g.shape, B)
    g1, c1 = rc.seeded_change(g, c, "u50", 5, 30 + B)
    g2, c2 = rc.seeded_change(g1, c1, "u50", 5, 40 + B)
    run_steps(g, c, sets, [(g1, c1, "five"), (g2, c2, "five more")], policies=[(1, 1)] if B == 70 else [(1, 1), (0, 0)], tag=B)


def test_awkward_sources():
    g = wc.seeded(30, 80, 0.2, 5)
    wall = [int(v) for v in np.flatnonzero(g.reshape(-1) == 1)[:3]]
    a, b, x, y = free_cells(g, 4, 6)
    sets = [[wall[0], a], [b, b, x, b], [wall[1], wall[2]], [a], [y, wall[0]]]     # listed on an obstacle; twice; no usable source; alone
    c = ck.cost_of_kind("u50", g.shape, 7)
    g1 = g.copy()
    g1.reshape(-1)[wall[0]], g1.reshape(-1)[a] = 0, 1                 # the listed obstacle opens, a source closes
    g2 = g1.copy()
    g2.reshape(-1)[wall[1]] = 0                                       # the set without a source gets one
    rig = Rig(g, c, sets)
    try:
        for ad, rs in [(1, 1), (0, 1)]:
            rig.set_map(g, c)
            rig.start(ad, rs)
            assert np.all(np.isinf(rig.D[2]))
            rig.step(g1, c, ad, rs, tag="opens and closes")
            D, info, _ = rig.repair([], ad, rs)
            assert np.all(np.isinf(D[3])) and list(info[3]) == [0, 0, -1, 0] and info[0][0] == 1 and info[1][0] == 2 and info[4][0] == 2
            assert D[0].reshape(-1)[wall[0]] == 0.0 and np.isinf(D[0].reshape(-1)[a])
            rig.step(g2, c, ad, rs, tag="a first source")
            assert rig.D[2].reshape(-1)[wall[1]] == 0.0
            rig.step(g, c, ad, rs, tag="back")
            for with_info in (False, True):
                rig.step(g1, c, ad, rs, tag="no info", want_info=with_info)
                rig.step(g, c, ad, rs, tag="no info, back", want_info=with_info)
    finally:
        rig.close()


# ---- 7. batches of changes
@pytest.mark.parametrize("n", [1, 7, 300])
def test_batches_on_a_300x517_map(n):
    g = wc.seeded(300, 517, 0.2, 77)
    c = ck.cost_of_kind("u50", g.shape, 3)
    src = free_cells(g, 3, 1)
    g1, c1 = rc.seeded_change(g, c, "u50", n, 50 + n, keep=src)
    rig = Rig(g, c, [src])
    try:
        rig.start(1, 1)
        changed = rc.changed_cells(g, c, g1, c1)
        assert 1 <= len(changed) <= n
        if n == 7:                                                    # duplicates, and cells that did not change
            changed = changed + changed[::-1] + free_cells(g1, 20, 4) + [0, g.size - 1]
        rig.step(g1, c1, 1, 1, changed=changed, tag=n)
    finally:
        rig.close()


def test_duplicates_and_unchanged_cells_in_the_list():
    g = wc.seeded(50, 130, 0.2, 31)
    c = ck.cost_of_kind("u50", g.shape, 3)
    src = free_cells(g, 2, 1)
    g1, c1 = rc.seeded_change(g, c, "u50", 6, 9, keep=src)
    exact = rc.changed_cells(g, c, g1, c1)
    rig = Rig(g, c, [src])
    try:
        raised = []
        for changed in (exact, exact * 3, exact + list(range(0, g.size, 97)), list(range(g.size))):
            rig.set_map(g, c)
            rig.start(1, 1)
            raised.append(rig.step(g1, c1, 1, 1, changed=changed)[3])
        assert len(set(raised)) == 1 and raised[0] > 0
    finally:
        rig.close()


# ---- 8. repeated repairs
def test_twelve_successive_repairs():
    g = wc.seeded(130, 200, 0.22, 13)
    c = ck.cost_of_kind("u50", g.shape, 2)
    src = free_cells(g, 2, 3)
    rig = Rig(g, c, [src])
    try:
        rig.start(1, 1)
        launches = set()
        for i in range(12):
            g, c = rc.seeded_change(g, c, "u50", 1 + (5 * i) % 9, 100 + i, keep=src[:1])
            launches.add(rig.step(g, c, 1, 1, tag=i)[0])
        assert len(launches) > 1                                      # odd and even numbers of launches: flags, lengths and parity start clean
    finally:
        rig.close()


def test_five_identical_repairs_are_bit_equal():
    g = wc.seeded(70, 150, 0.15, 4)
    c = ck.cost_of_kind("u1e6", g.shape, 1)
    sets = [free_cells(g, 2, 1), free_cells(g, 1, 2)]
    g1, c1 = rc.seeded_change(g, c, "u1e6", 12, 5, keep=sets[1])
    changed = rc.changed_cells(g, c, g1, c1)
    rig = Rig(g, c, sets)
    try:
        start = rig.start(1, 1).copy()
        rig.set_map(g1, c1)
        runs = []
        for _ in range(5):
            rig.rows.upload(start.reshape(-1))
            D, info, work = rig.repair(changed, 1, 1)
            runs.append((D.copy(), info.copy(), work[3]))
        for D, info, raised in runs[1:]:
            assert same_bits(D, runs[0][0]) and np.array_equal(info, runs[0][1]) and raised == runs[0][2]
        assert same_bits(runs[0][0], rig.fresh(1, 1)[0])
    finally:
        rig.close()


def test_the_shared_scratch_after_a_repair():
    from pathfit.engine import Engine
    g = wc.seeded(60, 140, 0.2, 8)
    c = ck.cost_of_kind("u50", g.shape, 1)
    src = free_cells(g, 3, 2)
    g1, c1 = rc.seeded_change(g, c, "u50", 8, 6, keep=src)
    off, ids = ck.csr([src[:1], src])
    n = 2 * g.size

    def others(e, dcost):
        d2, wd, st, best = e.buf(g.size, np.int32), e.buf(n, np.int32), e.buf(8 * n, np.float64), e.buf(n, np.float64)
        try:
            e.clearance_field(d2)
            e.clearance_widest(d2, off, ids, wd, 1, 1)
            e.turn_field(dcost, 2.5, off, ids, st, best, 1, 1)
            return wd.download(), st.download(), best.download()
        finally:
            for b in (d2, wd, st, best):
                b.free()
    rig = Rig(g, c, [src[:1], src])
    e2 = Engine(g1)
    try:
        rig.start(1, 1)
        rig.step(g1, c1, 1, 1)                                        # (its fresh call is pf_cost_field after the repair)
        got = others(rig.e, rig.dcost)
        want = others(e2, e2.put(c1.reshape(-1)))
        assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])
        rig.step(g, c, 1, 1)                                          # and a repair after them
    finally:
        rig.close()
        e2.close()


# ---- 9. through the class
def test_the_class_repairs_after_update_grid_and_with_a_new_cost_map():
    import pathfit
    g = wc.seeded(45, 100, 0.2, 31)
    cost = ck.cost_of_kind("u50", g.shape, 9)
    src = free_cells(g, 4, 10)
    sets = [src[:1], src[1:]]
    pairs = [[(v // 100, v % 100) for v in s] for s in sets]
    targets = free_cells(g, 30, 11)
    e = pathfit.Engine(g)
    cf = pathfit.CostField(g, cost, pairs, engine=e)

    def same_as_a_fresh_field(grid, c):
        new = pathfit.CostField(grid, c, pairs)
        try:
            want = ck.fields(grid, c, sets, True, True)
            assert same_bits(cf.fields, new.fields) and same_bits(cf.fields, want[0])
            assert np.array_equal(cf.info, new.info) and np.array_equal(cf.info, want[2])
            assert np.array_equal(cf.parents, new.parents) and np.array_equal(cf.parents, want[1])
            tp = [(v // 100, v % 100) for v in targets]
            for b in range(2):
                assert np.array_equal(cf.owners[b], new.owners[b]) and np.array_equal(cf.territory_sizes(b), new.territory_sizes(b))
                mine, theirs = cf.paths(tp, b=b), new.paths(tp, b=b)
                assert [p.cells.tolist() for p in mine] == [p.cells.tolist() for p in theirs]
                (ta, ba), (tb, bb) = cf.path_costs(mine), new.path_costs(theirs)
                assert same_bits(ta, tb) and np.array_equal(ba, bb)
            assert np.array_equal(cf.grid, np.array(grid, dtype=int)) and same_bits(cf.cost, np.array(c, np.float64))
            assert same_bits(cf.cost_device.download().reshape(g.shape), np.array(c, np.float64))
        finally:
            new.close()
    try:
        _ = cf.parents, cf.owners                                     # derived state that a repair must drop
        g1, _ = rc.seeded_change(g, cost, "u50", 6, 3, keep=src)
        g1 = np.where(g1 == 1, 1, 0).astype(np.uint8)
        e.update_grid(g1)
        assert cf.repair() is cf and cf.work[0] >= 2 and cf.kernel_ms > 0
        same_as_a_fresh_field(g1, cost)
        _, cost2 = rc.seeded_change(g1, cost, "u50", 40, 4, keep=[v for v in range(g.size) if g1.reshape(-1)[v] == 1])
        cf.repair(cost=cost2)
        same_as_a_fresh_field(g1, cost2)
        g3, cost3 = rc.seeded_change(g1, cost2, "u50", 10, 5, keep=src)
        e.update_grid(g3)
        cf.repair(cost=cost3)
        same_as_a_fresh_field(g3, cost3)
        # nothing changed: the fields and everything derived are kept, nothing is launched
        fields, parents, owners = cf.fields, cf.parents, cf.owners
        e.klog = []
        work = cf.work
        assert cf.repair() is cf and cf.repair(cost=cost3.copy()) is cf
        assert e.klog == [] and cf.fields is fields and cf.parents is parents and cf.owners is owners and cf.work == work
        e.klog = None
        bad = cost3.copy()
        bad.reshape(-1)[src[0]] = 0.5
        with pytest.raises(ValueError, match="^CostField: cost"):
            cf.repair(cost=bad)
        assert cf.fields is fields
    finally:
        cf.close()
        e.close()


# ---- 10. argument errors of the raw ABI
def test_argument_errors_leave_the_rows_and_the_info_untouched():
    from pathfit._lib import PathfitError
    from pathfit.engine import _View
    g = wc.seeded(20, 70, 0.2, 3)
    free = np.flatnonzero(g.reshape(-1) != 1)
    s0, s1 = int(free[0]), int(free[-1])
    c = ck.cost_of_kind("u50", g.shape, 1)
    rig = Rig(g, c, [[s0], [s1]])
    e, RC = rig.e, g.size
    ib = between_canaries(e, 8, np.int64)
    iv = _View(e, ib.at(PAD), 8, np.int64)
    try:
        start = rig.start(1, 1).copy()
        work0 = e.cost_field_work()

        def untouched():
            return same_bits(rig.shape(inner(rig.db, "rows")), start) and np.all(inner(ib, "info") == CANARY)

        def raw(cost, n, changed, B, off, src, rows, info, h=True):
            changed, off, src = np.asarray(changed, np.int32), np.asarray(off, np.int32), np.asarray(src, np.int32)
            return e.L.pf_cost_field_repair(e.h if h else None, 1, 1, cost, n, changed.ctypes.data if changed.size else None, B,
                                            off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, rows, info)
        ok = (rig.dcost.ptr, 1, [s0 + 1], 2, [0, 1, 2], [s0, s1], rig.rows.ptr, iv.ptr)

        def but(**kw):
            names = ("cost", "n", "changed", "B", "off", "src", "rows", "info")
            return raw(*[kw.get(k, v) for k, v in zip(names, ok)])
        assert but(n=-1) == -1 and b"must not be negative" in e.L.pf_last_error(e.h)
        assert but(n=2, changed=[]) == -1 and b"must not be null" in e.L.pf_last_error(e.h)
        for n, lst, at in ((1, [RC], 0), (3, [0, 5, -1], 2), (2, [3, 2 ** 31 - 1], 1)):
            assert but(n=n, changed=lst) == -1
            assert f"changed[{at}] = {lst[at]} lies outside the grid".encode() in e.L.pf_last_error(e.h)
        assert but(cost=None) == -1 and but(rows=None) == -1
        assert but(off=[]) == -1 and but(src=[]) == -1 and but(B=0, off=[0]) == -1 and but(B=-1) == -1
        assert but(off=[1, 1, 2]) == -1 and but(off=[0, 2, 1]) == -1 and but(off=[0, 0, 2]) == -1       # the start, the order, an empty set
        assert but(src=[s0, RC]) == -1 and but(src=[-1, s1]) == -1
        assert raw(*ok, h=False) == -2
        assert untouched() and e.cost_field_work() == work0
        where = int(free[len(free) // 2])
        for v in (0.5, 2.0 ** 20 + 1, np.nan, np.inf, 0.0):           # a bad cost on a free cell: refused before anything is written
            bad = c.copy()
            bad.reshape(-1)[where] = v
            rig.dcost.upload(bad.reshape(-1))
            with pytest.raises(PathfitError, match=rf"pf_cost_field_repair: bad arguments \(the cost of the free cell \({where // 70}, {where % 70}\)"):
                e.cost_field_repair(rig.dcost, [where], rig.off, rig.src, rig.rows, 1, 1, iv)
            assert but() == -1 and but(n=0, changed=[]) == -1
            assert untouched(), v
        rig.dcost.upload(c.reshape(-1))
        # nothing listed: the rows stay untouched, no tile kernel runs, the info is still written
        assert but(n=0, changed=[]) == 0 and e.cost_field_work() == (0, 0, 0, 0)
        assert same_bits(rig.shape(inner(rig.db, "rows")), start)
        assert np.array_equal(inner(ib, "info").reshape(2, 4), ck.fields(g, c, rig.sets, 1, 1)[2])
        junk = np.full(2 * RC, 123.0)
        rig.rows.upload(junk)
        assert but(n=0, changed=[], info=None) == 0 and np.all(inner(rig.db, "junk") == 123.0) and e.cost_field_work() == (0, 0, 0, 0)
        # rows out of contract: the call still ends, inside its bounds
        e.cost_field_repair(rig.dcost, list(range(0, RC, 7)), rig.off, rig.src, rig.rows, 1, 1, iv)
        inner(rig.db, "out of contract")
    finally:
        ib.free()
        rig.close()
