"""Turn-field repair on the device (pf_turn_field_repair, Engine.turn_field_repair, TurnField.repair) against a fresh pf_turn_field
call on the same handle afterwards AND the heap Dijkstra of tests/turn_checkers.py on the new map; d_info against the fresh call's;
the state words raised against the model of tests/turn_repair_checkers.py (pinned by tests/test_turn_repair_checkers.py).  Every
comparison is exact equality -- labels as 64-bit words --; every output lies between canary words."""
import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc
import golden_io as gio
import repair_checkers as rc
import thin_maps
import turn_checkers as tk
import turn_repair_checkers as tr
import widest_checkers as wc

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64
TW, TH = tk.TW, tk.TH                                                # the kernels' tile (PF_TF_TW x PF_TF_TH)
BIG = float(2 ** 20)
WTS = (0.0, 0.3, BIG)
_HEAP = {}


def heap(g, cost, sets, wt, ad, rs):
    """turn_checkers.fields on a map, computed once per (map, cost map, sets, weight, policy) and left unchanged."""
    key = (np.asarray(g, np.uint8).tobytes(), np.asarray(g).shape, None if cost is None else np.asarray(cost, np.float64).tobytes(), repr(sets), wt, ad, rs)
    if key not in _HEAP:
        _HEAP[key] = tk.fields(np.asarray(g), cost, sets, wt, ad, rs)
    return _HEAP[key]


def between_canaries(e, n, dtype, canary=CANARY):
    return e.put(np.full(n + 2 * PAD, canary, dtype))


def inner(buf, tag, canary=CANARY):
    a = buf.download()
    assert np.all(a[:PAD] == canary) and np.all(a[len(a) - PAD:] == canary), tag
    return a[PAD:len(a) - PAD]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class Rig:
    """An engine on a map, a cost map in HBM (or none), a turn weight, and the states and best rows of B sets between canaries, which
    every repair updates in place."""

    def __init__(self, g, cost, sets, wt):
        from pathfit.engine import Engine, _View
        self.g = np.array(g, np.uint8)
        self.e = Engine(self.g)
        self.sets, self.B, self.RC, self.wt = sets, len(sets), self.g.size, wt
        self.off, self.src = ck.csr(sets)
        self.cost = None if cost is None else np.array(cost, np.float64)
        self.dcost = None if cost is None else self.e.put(self.cost.reshape(-1))
        self.sb = between_canaries(self.e, 8 * self.B * self.RC, np.float64)
        self.bb = between_canaries(self.e, self.B * self.RC, np.float64)
        self.states = _View(self.e, self.sb.at(PAD), 8 * self.B * self.RC, np.float64)
        self.best = _View(self.e, self.bb.at(PAD), self.B * self.RC, np.float64)
        self.T = self.M = None

    def set_map(self, g, cost):
        g = np.array(g, np.uint8)
        if not np.array_equal(g, self.g):
            self.e.update_grid(g)
        self.g = g
        assert (cost is None) == (self.dcost is None)
        if cost is not None:
            self.cost = np.array(cost, np.float64)
            self.dcost.upload(self.cost.reshape(-1))

    def shape(self, flat, planes=False):
        return flat.reshape(((self.B, 8) if planes else (self.B,)) + self.g.shape)

    def read(self, tag):
        self.T, self.M = self.shape(inner(self.sb, (tag, "states")), True), self.shape(inner(self.bb, (tag, "best")))
        return self.T, self.M

    def start(self, ad, rs):
        """The rows become a fresh field of the present map."""
        self.e.turn_field(self.dcost, self.wt, self.off, self.src, self.states, self.best, ad, rs, None)
        return self.read("start")

    def fresh(self, ad, rs):
        """pf_turn_field from nothing on the same handle, into buffers of its own -> (T, best, info)."""
        from pathfit.engine import _View
        e, n = self.e, self.B * self.RC
        sb, bb, ib = between_canaries(e, 8 * n, np.float64), between_canaries(e, n, np.float64), between_canaries(e, 4 * self.B, np.int64)
        try:
            e.turn_field(self.dcost, self.wt, self.off, self.src, _View(e, sb.at(PAD), 8 * n, np.float64), _View(e, bb.at(PAD), n, np.float64), ad, rs,
                         _View(e, ib.at(PAD), 4 * self.B, np.int64))
            assert e.turn_field_work()[3] == 0
            return self.shape(inner(sb, "fresh T"), True), self.shape(inner(bb, "fresh best")), inner(ib, "fresh info").reshape(self.B, 4)
        finally:
            for b in (sb, bb, ib):
                b.free()

    def repair(self, changed, ad, rs, want_info=True):
        """One raw repair of the rows in place -> (T, best, info or None, work)."""
        from pathfit.engine import _View
        e = self.e
        ib = between_canaries(e, 4 * self.B, np.int64)
        try:
            e.turn_field_repair(self.dcost, self.wt, changed, self.off, self.src, self.states, self.best, ad, rs,
                                _View(e, ib.at(PAD), 4 * self.B, np.int64) if want_info else None)
            assert e.last_kernel_ms() > 0
            work = e.turn_field_work()
            assert work[0] <= work[1] and (work[0] > 0) == (work[1] > 0)
            info = inner(ib, "info").reshape(self.B, 4)
            if not want_info:
                assert np.all(info == CANARY)
            T, M = self.read("repair")
            return T, M, (info if want_info else None), work
        finally:
            ib.free()

    def step(self, g1, c1, ad, rs, changed=None, tag=None, want_info=True):
        """The map becomes (g1, c1) and the rows are repaired: compared with the fresh call afterwards, with the heap, with the fresh
        call's info and with the model's state words raised -> work."""
        old = self.T
        exact = tr.changed_cells(self.g, self.cost, g1, c1)
        if changed is None:
            changed = exact
        want_raised = sum(len(tr.raised_by_worklist(old[b], g1, c1, self.wt, exact, ad, rs)) for b in range(self.B))
        self.set_map(g1, c1)
        T, M, info, work = self.repair(changed, ad, rs, want_info)
        where = (tag, self.g.shape, ad, rs, self.wt)
        print("turn repair", where, "work", work, "model raised", want_raised)
        fT, fM, finfo = self.fresh(ad, rs)
        assert same_bits(T, fT), (where, "fresh states", np.argwhere(T != fT)[:4])
        assert same_bits(M, fM), (where, "fresh best", np.argwhere(M != fM)[:4])
        hT, hM, hinfo = heap(self.g, self.cost, self.sets, self.wt, ad, rs)
        assert same_bits(T, hT), (where, "heap states", np.argwhere(T != hT)[:4])
        assert same_bits(M, hM), (where, "heap best", np.argwhere(M != hM)[:4])
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
    """From (g, c): `cell` closes, opens again, the cost of `other` rises, then falls to 1 (without a cost map: `other` closes and
    opens instead) -> the four maps, each built on the last."""
    g = np.array(g, np.uint8)
    r, k = divmod(int(cell), g.shape[1])
    p, q = divmod(int(other), g.shape[1])
    g1 = g.copy()
    g1[r, k] = 1
    if c is None:
        g2 = g.copy()
        g2[p, q] = 1
        return [(g1, None, "closes"), (g, None, "opens"), (g2, None, "the other closes"), (g, None, "the other opens")]
    c = np.array(c, np.float64)
    c2 = c.copy()
    c2[p, q] = min(2.0 * c[p, q] + 3.3, BIG)
    c3 = c.copy()
    c3[p, q] = 1.0
    return [(g1, c, "closes"), (g, c, "opens"), (g, c2, "cost rises"), (g, c3, "cost falls")]


def run_steps(g, c, sets, wt, steps, policies=tk.POLICIES, tag=None, want_info=True):
    """Per policy: a fresh field on (g, c), then the steps (g1, c1, label) one after the other -> the works, per policy."""
    rig = Rig(g, c, sets, wt)
    works = {}
    try:
        for ad, rs in policies:
            rig.set_map(g, c)
            rig.start(ad, rs)
            works[ad, rs] = [rig.step(g1, c1, ad, rs, tag=(tag, label), want_info=want_info) for g1, c1, label in steps]
    finally:
        rig.close()
    return works


# ---- 1. small and thin maps; the four kinds of change at the three turn weights
@pytest.mark.parametrize("wt", WTS)
@pytest.mark.parametrize("kind", [None, "u50"])
def test_the_golden_20x20_map(kind, wt):
    g, s, t = gio.grid("fig7")
    free = free_cells(g, 6, 1)
    cells = [v for v in free if v not in (s, t)]
    c = tr.cost_of_kind(kind, g.shape, 2)
    works = run_steps(g, c, [[s], [t, s]], wt, four_changes(g, c, cells[0], cells[1]), tag=kind)
    assert all(w[1][3] == 0 for w in works.values())                  # a cell that opens raises nothing


THIN = [(1, 2), (2, 1), (1, 9), (2, 17), (17, 2), (1, 4096), (4096, 1)]


@pytest.mark.parametrize("R, C", THIN)
def test_thin_maps(R, C):
    g, s, t = thin_maps.thin_map(R, C, max(R, C) >= 9)
    c = ck.cost_of_kind("u50", g.shape, R + C)
    L = R * C
    free = [int(v) for v in np.flatnonzero(np.asarray(g).reshape(-1) != 1) if int(v) != s]
    cell = free[len(free) // 5]                                       # near the source: most of a corridor loses its support
    other = free[len(free) // 2] if len(free) > 1 else cell
    works = run_steps(g, c, [[s]] if L < 9 else [[s], [t, s]], 0.3, four_changes(g, c, cell, other), policies=[(1, 1), (0, 0)], tag=(R, C))
    if min(R, C) == 1 and L >= 9:
        assert all(w[0][3] > 0 for w in works.values())               # a closed corridor cell always raises what lies behind it
    if min(R, C) == 1:                                                # two headings only
        T = heap(g, c, [[s]] if L < 9 else [[s], [t, s]], 0.3, 1, 1)[0]
        assert sum(1 for d in range(8) if (np.isfinite(T[:, d]) & (T[:, d] > 0)).any()) <= 2   # (a source holds 0 in all eight)


# ---- 2. tile edges
@pytest.mark.parametrize("C", [TW - 1, TW, TW + 1, 2 * TW])
@pytest.mark.parametrize("R", [TH - 1, TH, TH + 1, 2 * TH])
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
        run_steps(m, c, [src[:1], src], 0.3, steps, policies=[(1, 1)] if j == 0 else [(0, 0)], tag=(R, C, j))


def test_a_changed_cell_on_a_tile_corner_border_and_interior():
    R, C = 2 * TH + 1, 2 * TW + 2
    g = wc.seeded(R, C, 0.15, 9)
    spots = [(TH - 1, TW - 1), (TH, TW), (TH - 1, TW), (TH, TW - 1), (TH - 1, 40), (TH, 40), (20, TW - 1), (20, TW), (24, 50), (0, 0), (R - 1, C - 1)]
    for r, k in spots:
        g[r, k] = 0
    c = ck.cost_of_kind("u50", g.shape, 4)
    src = [v for v in free_cells(g, 3, 5) if divmod(v, C) not in spots]
    steps = []
    for r, k in spots:
        closed = g.copy()
        closed[r, k] = 1
        steps += [(closed, c, ("closes", r, k)), (g, c, ("opens", r, k))]
    run_steps(g, c, [src], 0.3, steps, policies=[(1, 1), (0, 0)], tag="spots")


def test_a_diagonal_gap_across_a_tile_corner():
    r, c = 2 * TH, TW                                                 # the four cells about (r, c) lie in four tiles
    g = wc.corner_gap(4 * TH + 3, 2 * TW + 5, r, c)
    C = g.shape[1]
    shut = g.copy()
    shut[r - 1, c] = 1                                                # one of the two gap cells closed: the sides are apart under every policy
    left, right = (r + 5) * C + 3, 3 * C + c + 9
    rig = Rig(shut, None, [[left], [right]], 0.3)
    try:
        for ad, rs in tk.POLICIES:
            rig.set_map(shut, None)
            _, M = rig.start(ad, rs)
            assert np.isinf(M[0].reshape(-1)[right]) and np.isinf(M[1].reshape(-1)[left])
            w = rig.step(g, None, ad, rs, tag="gap opens")
            through = np.isfinite(rig.M[0].reshape(-1)[right])
            assert through == ((ad, rs) == (1, 0)) and np.isfinite(rig.M[1].reshape(-1)[left]) == through   # the free and the restricted policy disagree
            assert w[3] == 0
            w = rig.step(shut, None, ad, rs, tag="gap closes")
            assert (w[3] > 1000) == through and np.isinf(rig.M[0].reshape(-1)[right])
    finally:
        rig.close()


# ---- 3. the support rule's cases
def test_the_corner_rule_map():
    g0, g1, c, sources, wt, _ = tr.corner_rule_case()
    works = run_steps(g0, c, [sources], wt, [(g1, c, "x closes"), (g0, c, "x opens")])
    assert works[1, 1][0][3] > works[1, 0][0][3] > 0                  # restricted: the states behind the diagonal go too
    big = np.zeros((2 * TH + 2, 2 * TW + 2), np.uint8)                # the same four cells about a tile corner
    big2 = big.copy()
    big2[TH, TW] = 1
    src = [TH * big.shape[1] + TW - 1]
    works = run_steps(big, None, [src], wt, [(big2, None, "x closes"), (big, None, "x opens")])
    assert works[1, 1][0][3] > works[1, 0][0][3] > 0


def test_the_case_on_which_the_two_read_form_differs():
    g0, c0, g1, c1, sources, wt, (ad, rs) = tr.two_read_case()
    works = run_steps(g0, c0, [sources], wt, [(g1, c1, "three cells"), (g0, c0, "back")], policies=[(ad, rs)])
    assert works[ad, rs][0][3] == 18                                  # the literal form's count: the two-read form would raise 19


@pytest.mark.parametrize("shape", [(3, 3), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1)])
def test_best_rises_to_a_finite_value(shape):
    g0, g1, s, v, x, wt, (ad, rs) = tr.finite_rise_case(*shape)
    rig = Rig(g0, None, [[s]], wt)
    try:
        T0, M = (a.copy() for a in rig.start(ad, rs))
        before = M[0].reshape(-1)[v]
        w = rig.step(g1, None, ad, rs, tag="west of v closes")
        after = rig.M[0].reshape(-1)[v]
        assert w[3] > 0 and before < after < np.inf
        at_v = rig.T[0].reshape(8, -1)[:, v]
        assert np.isfinite(at_v).any() and np.isinf(at_v[np.isfinite(T0[0].reshape(8, -1)[:, v])]).any()   # some states of v went, not all
        rig.step(g0, None, ad, rs, tag="and opens")
        assert rig.M[0].reshape(-1)[v] == before
    finally:
        rig.close()


@pytest.mark.parametrize("wt", WTS)
def test_the_pocket_map(wt):
    g0, g1, s, cell, heading = tr.pocket_change()
    works = run_steps(g0, None, [[s]], wt, [(g1, None, "the dead end closes"), (g0, None, "and opens")])
    for w in works.values():
        assert w[0][3] == 2 and w[1][3] == 0 and w[1][2] == 2        # the dead end's state and the state that came back out of it


def test_a_door_that_seals_a_room_and_opens_again():
    g, door, inside, sealed = rc.sealed_room_map()
    C = g.shape[1]
    shut = g.copy()
    shut.reshape(-1)[door] = 1
    for kind in (None, "u50"):
        c = tr.cost_of_kind(kind, g.shape, 8)
        works = run_steps(g, c, [[C + 1]], 0.3, [(shut, c, "door closes"), (g, c, "door opens")], policies=[(1, 1), (0, 0)], tag=kind)
        for w in works.values():
            assert w[0][3] > 500 and w[1][3] == 0 and w[1][2] > 500   # a room's cells lose a state each at least; then nothing raised and a room lowered


def test_a_closing_in_a_sealed_room_raises_nothing():
    g, door, inside, sealed = rc.sealed_room_map()
    C = g.shape[1]
    g1 = g.copy()
    g1.reshape(-1)[sealed] = 1
    c = ck.cost_of_kind("u50", g.shape, 8)
    rig = Rig(g, c, [[C + 1]], 0.3)
    try:
        for ad, rs in tk.POLICIES:
            rig.set_map(g, c)
            T0, M0 = (a.copy() for a in rig.start(ad, rs))
            w = rig.step(g1, c, ad, rs, tag="sealed")
            assert w[3] == 0 and w[2] == 0 and same_bits(rig.T, T0) and same_bits(rig.M, M0)
    finally:
        rig.close()


# ---- 4. the reach of the invalid region
def test_a_long_corridor_needs_a_launch_per_tile():
    g, src, x = rc.long_corridor(200)
    g1 = g.copy()
    g1[0, x] = 1
    old = tr.fresh(g, None, [src], 0.3, 1, 1)
    gone = tr.raised_by_worklist(old, g1, None, 0.3, [x], 1, 1)
    need = tr.min_raise_launches(gone, [x], 1, 200)
    assert need == 7 and len(gone) == 199 + 198
    works = run_steps(g, None, [[src]], 0.3, [(g1, None, "closes"), (g, None, "opens")])
    for w in works.values():
        assert w[0][3] == len(gone) and w[0][0] >= need + 1           # the raise launches any timing needs, and one lower launch
        assert w[1][3] == 0 and w[1][2] == len(gone) and w[1][0] >= 1 + 7   # one raise launch, then the corridor again tile by tile


def test_a_serpentine_loses_its_tail_across_three_tiles():
    g = fc.serpentine(41)                                             # rows 0, 2, .., 40: the corridor crosses three tiles of 16 rows
    c = ck.cost_of_kind("u50", g.shape, 6)
    g1 = g.copy()
    g1[0, 5] = 1
    old = tr.fresh(g, c, [0], 0.3, 1, 1)
    gone = tr.raised_by_worklist(old, g1, c, 0.3, [5], 1, 1)
    need = tr.min_raise_launches(gone, [5], 41, 41)
    assert need >= 3 and len(rc.tiles_of([v for v, _ in gone], 41, tr.TILE)) >= 3
    works = run_steps(g, c, [[0]], 0.3, [(g1, c, "closes"), (g, c, "opens")], policies=[(1, 1), (0, 0)])
    assert works[1, 1][0][0] >= need + 1 and works[1, 1][0][3] == len(gone)


# ---- 5. costs and ties
def test_costs_at_the_bounds():
    g = wc.seeded(30, 70, 0.15, 12)
    rnd = np.random.default_rng(3)
    c = np.where(rnd.random(g.shape) < 0.5, 1.0, BIG)
    cells = free_cells(g, 4, 2)
    src, a, b = cells[0], cells[1], cells[2]
    c.reshape(-1)[a], c.reshape(-1)[b] = 1.0, BIG
    up, down = c.copy(), c.copy()
    up.reshape(-1)[a] = BIG
    down.reshape(-1)[a], down.reshape(-1)[b] = BIG, 1.0
    for wt in (0.3, BIG):
        run_steps(g, c, [[src]], wt, [(g, up, "1 -> 2^20"), (g, down, "2^20 -> 1")] + four_changes(g, down, cells[3], a)[:2], policies=[(1, 1)], tag=wt)


@pytest.mark.parametrize("kind", ["u1e6", "int14", "ones"])
def test_non_dyadic_costs_and_ties(kind):
    g = wc.seeded(30, 70, 0.2, 17)
    c = ck.cost_of_kind(kind, g.shape, 5)
    cells = free_cells(g, 3, 8)
    g1, c1 = rc.seeded_change(g, c, kind, 9, 21, keep=cells[:1])
    g2, c2 = rc.seeded_change(g1, c1, kind, 9, 22, keep=cells[:1])
    wt = 0.0 if kind == "int14" else 3.0 if kind == "ones" else 0.1   # integer costs at weight 0, unit costs at an integer weight: ties everywhere
    run_steps(g, c, [cells[:1], cells], wt, [(g1, c1, "nine"), (g2, c2, "nine more"), (g, c, "back")], policies=[(1, 1), (1, 0)], tag=kind)


# ---- 6. sources and sets
def test_no_cost_map_against_a_buffer_of_ones():
    g = wc.seeded(33, 70, 0.2, 41)
    src = free_cells(g, 2, 1)
    g1, _ = tr.seeded_change(g, None, None, 6, 3, keep=src)
    ones = np.ones(g.shape)
    a, b = Rig(g, None, [src], 0.3), Rig(g, ones, [src], 0.3)
    try:
        for rig, c in ((a, None), (b, ones)):
            rig.start(1, 1)
            rig.work = rig.step(g1, c, 1, 1, tag="ones" if c is not None else "none")
        assert same_bits(a.T, b.T) and same_bits(a.M, b.M) and a.work[3] == b.work[3]
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("B", [1, 3, 70])
def test_many_sets_in_one_call(B):
    g = wc.seeded(20, 45, 0.2, 21)
    rnd = np.random.default_rng(B)
    free = np.flatnonzero(g.reshape(-1) != 1)
    sets = [[int(v) for v in rnd.choice(free, int(rnd.integers(1, 5)))] for _ in range(B)]
    c = ck.cost_of_kind("u50", g.shape, B)
    g1, c1 = rc.seeded_change(g, c, "u50", 5, 30 + B)
    g2, c2 = rc.seeded_change(g1, c1, "u50", 5, 40 + B)
    run_steps(g, c, sets, 0.3, [(g1, c1, "five"), (g2, c2, "five more")], policies=[(1, 1)] if B == 70 else [(1, 1), (0, 0)], tag=B)


def test_awkward_sources():
    g = wc.seeded(30, 60, 0.2, 5)
    wall = [int(v) for v in np.flatnonzero(g.reshape(-1) == 1)[:3]]
    a, b, x, y = free_cells(g, 4, 6)
    sets = [[wall[0], a], [b, b, x, b], [wall[1], wall[2]], [a], [y, wall[0]]]     # listed on an obstacle; twice; no usable source; alone
    c = ck.cost_of_kind("u50", g.shape, 7)
    g1 = g.copy()
    g1.reshape(-1)[wall[0]], g1.reshape(-1)[a] = 0, 1                 # the listed obstacle opens, a source closes
    g2 = g1.copy()
    g2.reshape(-1)[wall[1]] = 0                                       # the set without a source gets one
    rig = Rig(g, c, sets, 0.3)
    try:
        for ad, rs in [(1, 1), (0, 1)]:
            rig.set_map(g, c)
            rig.start(ad, rs)
            assert np.all(np.isinf(rig.M[2]))
            rig.step(g1, c, ad, rs, tag="opens and closes")
            T, M, info, _ = rig.repair([], ad, rs)
            assert np.all(np.isinf(M[3])) and list(info[3]) == [0, 0, -1, 0] and info[0][0] == 1 and info[1][0] == 2 and info[4][0] == 2
            assert M[0].reshape(-1)[wall[0]] == 0.0 and np.all(T[0].reshape(8, -1)[:, wall[0]] == 0.0) and np.all(np.isinf(T[0].reshape(8, -1)[:, a]))
            rig.step(g2, c, ad, rs, tag="a first source")
            assert rig.M[2].reshape(-1)[wall[1]] == 0.0
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
    src = free_cells(g, 3, 1)
    g1, _ = tr.seeded_change(g, None, None, n, 50 + n, keep=src)
    rig = Rig(g, None, [src], 0.3)
    try:
        rig.start(1, 1)
        changed = tr.changed_cells(g, None, g1, None)
        assert len(changed) == n
        if n == 7:                                                    # duplicates, and cells that did not change
            changed = changed + changed[::-1] + free_cells(g1, 20, 4) + [0, g.size - 1]
        rig.step(g1, None, 1, 1, changed=changed, tag=n)
    finally:
        rig.close()


def test_duplicates_and_unchanged_cells_in_the_list():
    g = wc.seeded(40, 100, 0.2, 31)
    c = ck.cost_of_kind("u50", g.shape, 3)
    src = free_cells(g, 2, 1)
    g1, c1 = rc.seeded_change(g, c, "u50", 6, 9, keep=src)
    exact = rc.changed_cells(g, c, g1, c1)
    rig = Rig(g, c, [src], 0.3)
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
    g = wc.seeded(50, 100, 0.22, 13)
    c = ck.cost_of_kind("u50", g.shape, 2)
    src = free_cells(g, 2, 3)
    rig = Rig(g, c, [src], 0.3)
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
    g = wc.seeded(50, 100, 0.15, 4)
    c = ck.cost_of_kind("u1e6", g.shape, 1)
    sets = [free_cells(g, 2, 1), free_cells(g, 1, 2)]
    g1, c1 = rc.seeded_change(g, c, "u1e6", 12, 5, keep=sets[1])
    changed = rc.changed_cells(g, c, g1, c1)
    rig = Rig(g, c, sets, 0.3)
    try:
        T0, M0 = (a.copy() for a in rig.start(1, 1))
        rig.set_map(g1, c1)
        runs = []
        for _ in range(5):
            rig.states.upload(T0.reshape(-1))
            rig.best.upload(M0.reshape(-1))
            T, M, info, work = rig.repair(changed, 1, 1)
            runs.append((T.copy(), M.copy(), info.copy(), work[3]))
        for T, M, info, raised in runs[1:]:
            assert same_bits(T, runs[0][0]) and same_bits(M, runs[0][1]) and np.array_equal(info, runs[0][2]) and raised == runs[0][3]
        fT, fM, finfo = rig.fresh(1, 1)
        assert same_bits(runs[0][0], fT) and same_bits(runs[0][1], fM) and np.array_equal(runs[0][2], finfo)
    finally:
        rig.close()


# ---- 9. next to the other tile-queue calls
def test_weight_zero_against_the_cost_repair_on_the_same_handle():
    g = wc.seeded(40, 100, 0.2, 8)
    c = ck.cost_of_kind("u50", g.shape, 1)
    src = free_cells(g, 3, 2)
    g1, c1 = rc.seeded_change(g, c, "u50", 8, 6, keep=src)
    rig = Rig(g, c, [src[:1], src], 0.0)
    rows = rig.e.buf(2 * g.size, np.float64)
    try:
        rig.start(1, 1)
        rig.e.cost_field(rig.dcost, rig.off, rig.src, rows, 1, 1, None)
        assert same_bits(rows.download(), rig.M.reshape(-1))
        changed = rc.changed_cells(g, c, g1, c1)
        rig.step(g1, c1, 1, 1, tag="turn, weight 0")
        rig.e.cost_field_repair(rig.dcost, changed, rig.off, rig.src, rows, 1, 1, None)
        assert same_bits(rows.download(), rig.M.reshape(-1))          # best at weight 0 is the cost field, repaired or fresh
        rig.step(g, c, 1, 1, tag="turn, back")
        rig.e.cost_field_repair(rig.dcost, changed, rig.off, rig.src, rows, 1, 1, None)
        assert same_bits(rows.download(), rig.M.reshape(-1))
    finally:
        rows.free()
        rig.close()


def test_the_shared_scratch_after_a_repair():
    from pathfit.engine import Engine
    g = wc.seeded(40, 100, 0.2, 8)
    c = ck.cost_of_kind("u50", g.shape, 1)
    src = free_cells(g, 3, 2)
    g1, c1 = rc.seeded_change(g, c, "u50", 8, 6, keep=src)
    off, ids = ck.csr([src[:1], src])
    n = 2 * g.size

    def others(e, dcost):
        d2, wd, rows, st, best = e.buf(g.size, np.int32), e.buf(n, np.int32), e.buf(n, np.float64), e.buf(8 * n, np.float64), e.buf(n, np.float64)
        try:
            e.clearance_field(d2)
            e.clearance_widest(d2, off, ids, wd, 1, 1)
            e.cost_field(dcost, off, ids, rows, 1, 1)
            e.turn_field(dcost, 2.5, off, ids, st, best, 1, 1)
            return wd.download(), rows.download(), st.download(), best.download()
        finally:
            for b in (d2, wd, rows, st, best):
                b.free()
    rig = Rig(g, c, [src[:1], src], 0.3)
    e2 = Engine(g1)
    try:
        rig.start(1, 1)
        rig.step(g1, c1, 1, 1)                                        # (its fresh call is pf_turn_field after the repair)
        got = others(rig.e, rig.dcost)
        want = others(e2, e2.put(c1.reshape(-1)))
        assert np.array_equal(got[0], want[0]) and all(same_bits(a, b) for a, b in zip(got[1:], want[1:]))
        rig.step(g, c, 1, 1)                                          # and a repair after them
    finally:
        rig.close()
        e2.close()


# ---- 10. through the class
def test_the_class_repairs_after_update_grid_and_with_a_new_cost_map():
    import pathfit
    g = wc.seeded(40, 90, 0.2, 31)
    C = g.shape[1]
    cost = ck.cost_of_kind("u50", g.shape, 9)
    src = free_cells(g, 4, 10)
    sets = [src[:1], src[1:]]
    pairs = [[(v // C, v % C) for v in s] for s in sets]
    targets = free_cells(g, 30, 11)
    wt = 0.3
    e = pathfit.Engine(g)
    tf = pathfit.TurnField(g, pairs, wt, engine=e)                    # built without a cost map

    def same_as_a_fresh_field(grid, c):
        new = pathfit.TurnField(grid, pairs, wt, cost=c)
        try:
            want = heap(grid, c, sets, wt, True, True)
            assert same_bits(tf.states, new.states) and same_bits(tf.states, want[0])
            assert same_bits(tf.best, new.best) and same_bits(tf.best, want[1])
            assert np.array_equal(tf.info, new.info) and np.array_equal(tf.info, want[2])
            tp = [(v // C, v % C) for v in targets if np.asarray(grid).reshape(-1)[v] != 1]
            for b in range(2):
                mine, theirs = tf.paths(tp, b=b), new.paths(tp, b=b)
                assert [p.cells.tolist() for p in mine] == [p.cells.tolist() for p in theirs]
                assert [tf.heading(b, t) for t in tp] == [new.heading(b, t) for t in tp]
                (ta, na, ba), (tb, nb, bb) = tf.path_costs(mine), new.path_costs(theirs)
                assert same_bits(ta, tb) and np.array_equal(na, nb) and np.array_equal(ba, bb)
            assert np.array_equal(tf.grid, np.array(grid, dtype=int))
            if c is not None:
                assert same_bits(tf.cost, np.array(c, np.float64)) and same_bits(tf.cost_device.download().reshape(g.shape), np.array(c, np.float64))
        finally:
            new.close()
    try:
        _ = tf.states, tf.best, tf.info                              # downloaded state that a repair must drop
        g1, _ = tr.seeded_change(g, None, None, 6, 3, keep=src)
        g1 = np.where(g1 == 1, 1, 0).astype(np.uint8)
        e.update_grid(g1)
        assert tf.repair() is tf and tf.work[0] >= 2 and tf.kernel_ms > 0 and tf.cost is None and tf.cost_device is None
        same_as_a_fresh_field(g1, None)
        _, cost2 = rc.seeded_change(g1, np.ones(g.shape), "u50", 40, 4, keep=[v for v in range(g.size) if g1.reshape(-1)[v] == 1])
        tf.repair(cost=cost2)                                         # the field takes a cost map here
        same_as_a_fresh_field(g1, cost2)
        g3, cost3 = rc.seeded_change(g1, cost2, "u50", 10, 5, keep=src)
        e.update_grid(g3)
        tf.repair(cost=cost3)
        same_as_a_fresh_field(g3, cost3)
        # nothing changed: what was downloaded is kept, nothing is launched
        states, best, info = tf.states, tf.best, tf.info
        e.klog = []
        work = tf.work
        assert tf.repair() is tf and tf.repair(cost=cost3.copy()) is tf
        assert e.klog == [] and tf.states is states and tf.best is best and tf.info is info and tf.work == work
        e.klog = None
        bad = cost3.copy()
        bad.reshape(-1)[src[0]] = 0.5
        with pytest.raises(ValueError, match="^TurnField: cost"):
            tf.repair(cost=bad)
        assert tf.states is states
    finally:
        tf.close()
        e.close()


# ---- 11. argument errors of the raw ABI
def test_argument_errors_leave_the_rows_and_the_info_untouched():
    from pathfit._lib import PathfitError
    from pathfit.engine import _View
    g = wc.seeded(20, 70, 0.2, 3)
    free = np.flatnonzero(g.reshape(-1) != 1)
    s0, s1 = int(free[0]), int(free[-1])
    c = ck.cost_of_kind("u50", g.shape, 1)
    rig = Rig(g, c, [[s0], [s1]], 0.3)
    e, RC = rig.e, g.size
    ib = between_canaries(e, 8, np.int64)
    iv = _View(e, ib.at(PAD), 8, np.int64)
    try:
        T0, M0 = (a.copy() for a in rig.start(1, 1))
        work0 = e.turn_field_work()

        def untouched():
            T, M = rig.read("rows")
            return same_bits(T, T0) and same_bits(M, M0) and np.all(inner(ib, "info") == CANARY)

        def raw(cost, wt, n, changed, B, off, src, states, best, info, h=True):
            changed, off, src = np.asarray(changed, np.int32), np.asarray(off, np.int32), np.asarray(src, np.int32)
            return e.L.pf_turn_field_repair(e.h if h else None, 1, 1, cost, wt, n, changed.ctypes.data if changed.size else None, B,
                                            off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, states, best, info)
        ok = (rig.dcost.ptr, 0.3, 1, [s0 + 1], 2, [0, 1, 2], [s0, s1], rig.states.ptr, rig.best.ptr, iv.ptr)

        def but(**kw):
            names = ("cost", "wt", "n", "changed", "B", "off", "src", "states", "best", "info")
            return raw(*[kw.get(k, v) for k, v in zip(names, ok)])
        assert but(n=-1) == -1 and b"must not be negative" in e.L.pf_last_error(e.h)
        assert but(n=2, changed=[]) == -1 and b"must not be null" in e.L.pf_last_error(e.h)
        for n, lst, at in ((1, [RC], 0), (3, [0, 5, -1], 2), (2, [3, 2 ** 31 - 1], 1)):
            assert but(n=n, changed=lst) == -1
            assert f"changed[{at}] = {lst[at]} lies outside the grid".encode() in e.L.pf_last_error(e.h)
        assert but(states=None) == -1 and but(best=None) == -1
        for wt in (-0.5, 2.0 ** 20 + 1, float("nan"), float("inf")):
            assert but(wt=wt) == -1 and b"pf_turn_field_repair: bad arguments (the turn weight" in e.L.pf_last_error(e.h), wt
        assert but(off=[]) == -1 and but(src=[]) == -1 and but(B=0, off=[0]) == -1 and but(B=-1) == -1
        assert but(off=[1, 1, 2]) == -1 and but(off=[0, 2, 1]) == -1 and but(off=[0, 0, 2]) == -1       # the start, the order, an empty set
        assert but(src=[s0, RC]) == -1 and but(src=[-1, s1]) == -1
        assert raw(*ok, h=False) == -2
        assert untouched() and e.turn_field_work() == work0
        where = int(free[len(free) // 2])
        for v in (0.5, 2.0 ** 20 + 1, np.nan, np.inf, 0.0):           # a bad cost on a free cell: refused before anything is written
            bad = c.copy()
            bad.reshape(-1)[where] = v
            rig.dcost.upload(bad.reshape(-1))
            with pytest.raises(PathfitError, match=rf"pf_turn_field_repair: bad arguments \(the cost of the free cell \({where // 70}, {where % 70}\)"):
                e.turn_field_repair(rig.dcost, 0.3, [where], rig.off, rig.src, rig.states, rig.best, 1, 1, iv)
            assert but() == -1 and but(n=0, changed=[]) == -1
            assert untouched(), v
        rig.dcost.upload(c.reshape(-1))
        # nothing listed: the rows stay untouched, no tile kernel runs, the info is still written
        assert but(n=0, changed=[]) == 0 and e.turn_field_work() == (0, 0, 0, 0)
        T, M = rig.read("rows")
        assert same_bits(T, T0) and same_bits(M, M0)
        assert np.array_equal(inner(ib, "info").reshape(2, 4), heap(g, c, rig.sets, 0.3, 1, 1)[2])
        rig.states.upload(np.full(16 * RC, 123.0))
        rig.best.upload(np.full(2 * RC, 123.0))
        assert but(n=0, changed=[], info=None) == 0 and np.all(inner(rig.sb, "junk") == 123.0) and np.all(inner(rig.bb, "junk") == 123.0)
        assert e.turn_field_work() == (0, 0, 0, 0)
        # rows out of contract: the call still ends, inside its bounds
        e.turn_field_repair(rig.dcost, 0.3, list(range(0, RC, 7)), rig.off, rig.src, rig.states, rig.best, 1, 1, iv)
        inner(rig.sb, "out of contract")
        inner(rig.bb, "out of contract")
    finally:
        ib.free()
        rig.close()
