"""Pins the CPU model of the turn-field repair (tests/turn_repair_checkers.py) against the heap Dijkstra of tests/turn_checkers.py on
the NEW map, bit for bit; makes it reject three wrong repairs, each on a map built for the purpose; compares the literal form of the
support rule with the relax kernel's two-read form; and asserts the CPU facts that tests/test_gpu_turn_repair.py leans on (runs on a
CPU-only host)."""
import numpy as np
import pytest

import field_checkers as fc
import repair_checkers as rc
import turn_checkers as tk
import turn_repair_checkers as tr

KINDS = tk.KINDS + (None,)                                           # None: no cost map


def seeded_case(seed, kind):
    """A grid of 3..11 cells a side, a cost map of the kind, 1..3 sources, 1..4 mixed changes, a turn weight of turn_checkers.WEIGHTS
    -> (g0, c0, g1, c1, sources, wt)."""
    rnd = np.random.default_rng(seed)
    R, C = (int(v) for v in rnd.integers(3, 12, 2))
    g0 = (rnd.random((R, C)) < 0.25).astype(int)
    c0 = tr.cost_of_kind(kind, (R, C), seed)
    free = np.flatnonzero(g0.reshape(-1) != 1)
    if len(free) == 0:
        g0[0, 0] = 0
        free = np.array([0])
    sources = [int(v) for v in rnd.choice(free, min(int(rnd.integers(1, 4)), len(free)), replace=False)]
    g1, c1 = tr.seeded_change(g0, c0, kind, int(rnd.integers(1, 5)), seed + 5)      # (a source may close, and open again later)
    return g0, c0, g1, c1, sources, tk.WEIGHTS[seed % len(tk.WEIGHTS)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ad, rs", tk.POLICIES)
def test_the_model_is_the_fresh_dijkstra_bit_for_bit(ad, rs, kind):
    raised = states = 0
    for seed in range(60):                                            # 4 policies x 5 kinds x 60 = 1 200 cases, every turn weight twelve times each
        g0, c0, g1, c1, sources, wt = seeded_case(1000 * (2 * ad + rs) + seed, kind)
        mm = fc.move_masks(np.asarray(g1), ad, rs)
        old, want = tr.fresh(g0, c0, sources, wt, ad, rs), tk.dijkstra(np.asarray(g1), mm, c1, sources, wt)
        changed = tr.changed_cells(g0, c0, g1, c1)
        a = tr.repair(old, g1, c1, sources, wt, changed, ad, rs, seed=seed)
        b = tr.repair(old, g1, c1, sources, wt, changed, ad, rs, seed=seed + 100, tile=(2, 3))  # another order, and a queue of many tiles
        where = (seed, kind, ad, rs, wt)
        for got in (a, b):
            assert tr.same_bits(got.T, want), (where, np.argwhere(got.T != want)[:4])
            assert tr.same_bits(got.best, want.min(axis=0))
        assert a.n_raised == b.n_raised and set(a.raised) == set(b.raised), where   # the surviving set is unique
        assert len(set(a.raised)) == a.n_raised                       # inf is never raised twice
        assert all(np.isfinite(old.reshape(8, -1)[d, v]) for v, d in a.raised)
        assert tr.raised_by_label_order(old, g1, c1, wt, ad, rs) == sorted(a.raised), where     # the sweep-free derivations of the same set
        assert tr.raised_by_worklist(old, g1, c1, wt, changed, ad, rs) == sorted(a.raised), where
        assert tr.same_bits(a.best_raised, b.best_raised)
        # a repair with nothing listed on an unchanged map moves nothing
        same = tr.repair(want, g1, c1, sources, wt, [], ad, rs, seed=seed)
        assert same.n_raised == 0 and not same.lowered and not same.first and tr.same_bits(same.T, want)
        # ... and listing cells that did not change, twice, is harmless
        extra = tr.repair(old, g1, c1, sources, wt, changed + changed + [0, g0.size - 1], ad, rs, seed=seed)
        assert tr.same_bits(extra.T, want) and extra.n_raised == a.n_raised
        raised += a.n_raised
        states += old.size
    assert 0 < raised < states


def test_the_two_read_form_against_the_literal_form():
    """The search the design note reports: over the seeded cases, three sweep orders each, does the relax kernel's two-read form
    raise another set than the literal form?  One case does: at a changed cell, where a weight fell, a state keeps
    its label by a supporter d' that is neither d nor the minimum of u -- the literal form keeps it, the two-read form raises it.
    The difference lies inside the 3 x 3 blocks of the changed cells, where the argument for the two forms' agreement fails, and
    nowhere else.  The kernel evaluates the literal form, and the model -- the literal form -- is what must equal Dijkstra."""
    differing = {}
    for kind in KINDS:
        for ad, rs in tk.POLICIES:
            for seed in range(10):
                g0, c0, g1, c1, sources, wt = seeded_case(5000 + 1000 * (2 * ad + rs) + seed, kind)
                old = tr.fresh(g0, c0, sources, wt, ad, rs)
                changed = tr.changed_cells(g0, c0, g1, c1)
                lit = set(tr.raised_by_label_order(old, g1, c1, wt, ad, rs))
                R, C = g0.shape
                blocks = {rr * C + kk for x in changed for rr in range(max(x // C - 1, 0), min(x // C + 1, R - 1) + 1)
                          for kk in range(max(x % C - 1, 0), min(x % C + 1, C - 1) + 1)}
                for order in range(3):
                    two = set(tr.repair(old, g1, c1, sources, wt, changed, ad, rs, seed=order, form="two_read").raised)
                    if two != lit:
                        assert all(v in blocks for v, _ in two ^ lit), (kind, ad, rs, seed)
                        differing.setdefault((kind, ad, rs, seed), []).append((sorted(lit - two), sorted(two - lit)))
    assert differing == {("int14", 1, 0, 5): [([], [(6, 6)])] * 3}    # whatever the order: one state more
    # the case the model must get right: 18 states raised, not 19, and Dijkstra's states
    g0, c0, g1, c1, sources, wt = seeded_case(5000 + 1000 * 2 + 5, "int14")
    k0, d0, k1, d1, s, w, (ad, rs) = tr.two_read_case()
    assert np.array_equal(g0, k0) and np.array_equal(g1, k1) and np.array_equal(c0, d0) and np.array_equal(c1, d1) and (sources, wt) == (s, w)
    old, want = tr.fresh(g0, c0, sources, wt, ad, rs), tr.fresh(g1, c1, sources, wt, ad, rs)
    changed = tr.changed_cells(g0, c0, g1, c1)
    assert (ad, rs) == (1, 0) and changed == [4, 6, 14]
    rep = tr.repair(old, g1, c1, sources, wt, changed, ad, rs)
    assert rep.n_raised == 18 and (6, 6) not in rep.raised and tr.same_bits(rep.T, want)
    assert tr.raised_by_worklist(old, g1, c1, wt, changed, ad, rs) == sorted(rep.raised)


def test_changed_cells_without_a_cost_map():
    g0 = np.array([[0, 1, 0, 1], [0, 0, 2, 3]])
    g1 = np.array([[0, 0, 1, 1], [0, 0, 0, 0]])
    c1 = np.array([[1.0, 3.0, np.nan, np.nan], [1.5, 1.0, 1.0, 1.0]])
    assert tr.changed_cells(g0, None, g1, None) == [1, 2]
    assert tr.changed_cells(g0, None, g1, c1) == [1, 2, 4] and tr.changed_cells(g1, c1, g0, None) == [1, 2, 4]
    assert tr.changed_cells(g0, None, g0, np.ones(g0.shape)) == []


# ---- the three wrong repairs
def test_a_repair_without_a_raise_phase_is_rejected():
    g0, g1, c, sources, wt, (ad, rs) = tr.closed_corridor_case()
    old, want = tr.fresh(g0, c, sources, wt, ad, rs), tr.fresh(g1, c, sources, wt, ad, rs)
    changed = tr.changed_cells(g0, c, g1, c)
    assert changed == [3] and np.all(np.isinf(want[:, 2, 0])) and np.isfinite(old[:, 2, 0]).any()
    good = tr.repair(old, g1, c, sources, wt, changed, ad, rs)
    assert tr.same_bits(good.T, want) and good.n_raised == int(np.isfinite(old).sum() - np.isfinite(want).sum()) > 10
    bad = tr.repair(old, g1, c, sources, wt, changed, ad, rs, variant="no_raise")
    assert bad.n_raised == 0 and not tr.same_bits(bad.T, want)
    assert bad.best[2, 0] == old.min(axis=0)[2, 0] < want.min(axis=0)[2, 0]   # a label below the answer, which no lowering sweep repairs


def test_raising_only_along_legal_moves_from_a_changed_cell_is_rejected():
    g0, g1, c, sources, wt, (ad, rs) = tr.corner_rule_case()
    assert (ad, rs) == (1, 1)
    old, want = tr.fresh(g0, c, sources, wt, ad, rs), tr.fresh(g1, c, sources, wt, ad, rs)
    changed = tr.changed_cells(g0, c, g1, c)
    assert changed == [4] and old[6, 0, 1] == fc.SQRT2 and np.isinf(want[6, 0, 1]) and want.min(axis=0)[0, 1] == 1.0 + (1.0 + wt)
    good = tr.repair(old, g1, c, sources, wt, changed, ad, rs)
    assert tr.same_bits(good.T, want) and (1, 6) in good.raised
    bad = tr.repair(old, g1, c, sources, wt, changed, ad, rs, variant="legal_from_changed")
    assert not tr.same_bits(bad.T, want) and bad.T[6, 0, 1] == fc.SQRT2 and bad.best[0, 1] < want.min(axis=0)[0, 1]
    # under the free policy the diagonal stays legal and the state stays
    old_f, want_f = tr.fresh(g0, c, sources, wt, 1, 0), tr.fresh(g1, c, sources, wt, 1, 0)
    keep = tr.repair(old_f, g1, c, sources, wt, changed, 1, 0)
    assert tr.same_bits(keep.T, want_f) and (1, 6) not in keep.raised and want_f[6, 0, 1] == fc.SQRT2


def test_lowering_only_the_tiles_with_a_raised_word_is_rejected():
    g, c0, c1, sources, wt, (ad, rs) = tr.falling_cost_case()
    old, want = tr.fresh(g, c0, sources, wt, ad, rs), tr.fresh(g, c1, sources, wt, ad, rs)
    assert old.min(axis=0).tolist() == [[0.0, 2.0, 0.0]] and want.min(axis=0).tolist() == [[0.0, 1.0, 0.0]]
    assert sorted(old[:, 0, 1][np.isfinite(old[:, 0, 1])].tolist()) == [2.0, 2.0]      # x's two states, one from either source
    changed = tr.changed_cells(g, c0, g, c1)
    assert changed == [1]
    good = tr.repair(old, g, c1, sources, wt, changed, ad, rs)
    assert good.n_raised == 0 and good.first == {(0, 0)} and {v for v, _ in good.lowered} == {1} and tr.same_bits(good.T, want)
    bad = tr.repair(old, g, c1, sources, wt, changed, ad, rs, variant="lower_touched_only")
    assert bad.n_raised == 0 and not bad.first and tr.same_bits(bad.T, old) and not tr.same_bits(bad.T, want)


# ---- the CPU facts the GPU file leans on
def test_best_rises_to_a_finite_value():
    g0, g1, s, v, x, wt, (ad, rs) = tr.finite_rise_case()
    C = g0.shape[1]
    old, want = tr.fresh(g0, None, [s], wt, ad, rs), tr.fresh(g1, None, [s], wt, ad, rs)
    rep = tr.repair(old, g1, None, [s], wt, [x], ad, rs)
    gone = {d for cell, d in rep.raised if cell == v}
    stay = {d for d in range(8) if np.isfinite(rep.T[d, v // C, v % C])} - gone
    assert gone and stay and tr.same_bits(rep.T, want)               # some states of v raised, not all
    before, between = old.min(axis=0)[v // C, v % C], rep.best_raised[v // C, v % C]
    assert before == 2.0 and before < between < np.inf and between == want.min(axis=0)[v // C, v % C] == 4.0 + 2 * wt
    for shape in ((33, 65), (17, 33)):                                # the same on the maps of the GPU test: v in another tile than the source
        h0, h1, s, v, x, wt, (ad, rs) = tr.finite_rise_case(*shape)
        old = tr.fresh(h0, None, [s], wt, ad, rs)
        gone = tr.raised_by_worklist(old, h1, None, wt, [x], ad, rs)
        at_v = {d for cell, d in gone if cell == v}
        assert at_v and np.isfinite(tr.fresh(h1, None, [s], wt, ad, rs).min(axis=0).reshape(-1)[v])
        assert tr.same_bits(tr.repair(old, h1, None, [s], wt, [x], ad, rs).T, tr.fresh(h1, None, [s], wt, ad, rs))


def test_facts_of_the_pocket():
    g0, g1, s, cell, heading = tr.pocket_change()
    for wt in (0.0, 0.3):
        old = tr.fresh(g0, None, [s], wt, 1, 1)
        assert old[heading, 0, cell] == 1.0 + ((1.0 + wt) + 1.0) or old[heading, 0, cell] == (1.0 + 1.0) + (1.0 + wt)   # past the cell, into the dead end, back
        assert len(tk.route(old, None, cell, wt, heading)) == 4       # the walk passes the cell twice
        rep = tr.repair(old, g1, None, [s], wt, [2], 1, 1)
        assert (cell, heading) in rep.raised and rep.n_raised == 2 and tr.same_bits(rep.T, tr.fresh(g1, None, [s], wt, 1, 1))
        assert rep.best[0, cell] == old.min(axis=0)[0, cell] == 1.0   # best stands: the state that came straight is still supported
        back = tr.repair(rep.T, g0, None, [s], wt, [2], 1, 1)
        assert back.n_raised == 0 and tr.same_bits(back.T, old)


def test_facts_of_the_door_maps():
    g, door, inside, sealed = rc.sealed_room_map()
    C = g.shape[1]
    src, wt = [1 * C + 1], 0.3
    old = tr.fresh(g, None, src, wt, 1, 1)
    ob = old.min(axis=0).reshape(-1)
    assert np.isfinite(ob[inside]) and np.isfinite(ob[door]) and np.isinf(ob[sealed])
    g1 = g.copy()
    g1.reshape(-1)[door] = 1
    want = tr.fresh(g1, None, src, wt, 1, 1)
    gone = tr.raised_by_worklist(old, g1, None, wt, [door], 1, 1)
    assert len(gone) >= int((np.isfinite(old) & np.isinf(want)).sum()) > 4000 and len(rc.tiles_of([v for v, _ in gone], C, tr.TILE)) >= 2
    assert gone == tr.raised_by_label_order(old, g1, None, wt, 1, 1)
    g2 = g.copy()
    g2.reshape(-1)[sealed] = 1                                        # a closing where no source reaches: nothing raised
    assert tr.raised_by_worklist(old, g2, None, wt, [sealed], 1, 1) == [] and tr.same_bits(tr.fresh(g2, None, src, wt, 1, 1), old)


def test_facts_of_the_long_corridor():
    g, src, x = rc.long_corridor(200)
    old = tr.fresh(g, None, [src], 0.3, 1, 1)
    g1 = g.copy()
    g1[0, x] = 1
    gone = tr.raised_by_worklist(old, g1, None, 0.3, [x], 1, 1)
    assert {v for v, _ in gone} == set(range(1, 200)) and len(gone) == 199 + 198        # the east states of 1 .. 199 and the west states of 1 .. 198 (walks that turn back at the far end)
    tiles = rc.tiles_of([v for v, _ in gone], 200, tr.TILE)
    assert tiles == {(0, k) for k in range(7)} and tr.min_raise_launches(gone, [x], 1, 200) == 7
    assert tr.min_raise_launches([], [x], 1, 200) == 0


def test_facts_of_the_sources_that_close_and_open():
    g = np.zeros((5, 9), int)
    g[2, 4] = 1
    sets = [0, 2 * 9 + 4, 44]                                         # the middle one is listed ON an obstacle
    old = tr.fresh(g, None, sets, 0.3, 1, 1)
    assert np.all(np.isinf(old[:, 2, 4])) and np.all(old[:, 0, 0] == 0.0)
    g1 = g.copy()
    g1[2, 4], g1[0, 0] = 0, 1                                         # the listed obstacle opens; a source closes
    rep = tr.repair(old, g1, None, sets, 0.3, tr.changed_cells(g, None, g1, None), 1, 1)
    assert rep.reseeded == [2 * 9 + 4] and {(0, d) for d in range(8)} <= set(rep.raised)
    assert tr.same_bits(rep.T, tr.fresh(g1, None, sets, 0.3, 1, 1)) and np.all(rep.T[:, 2, 4] == 0.0) and np.all(np.isinf(rep.T[:, 0, 0]))
