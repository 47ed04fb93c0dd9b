"""Pins the CPU model of the cost-field repair (tests/repair_checkers.py) against the heap Dijkstra of tests/cost_checkers.py on the
NEW map, bit for bit; makes it reject three wrong repairs, each on a map built for the purpose; and asserts the CPU facts that
tests/test_gpu_cost_repair.py leans on (runs on a CPU-only host)."""
import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc
import repair_checkers as rc

KINDS = ("ones", "int14", "u50", "u1e6")


def seeded_case(seed, kind):
    """A grid of 3..11 cells a side, a cost map of the kind, 1..3 sources, 1..4 mixed changes -> (g0, c0, g1, c1, sources)."""
    rnd = np.random.default_rng(seed)
    R, C = (int(v) for v in rnd.integers(3, 12, 2))
    g0 = (rnd.random((R, C)) < 0.25).astype(int)
    c0 = ck.cost_of_kind(kind, (R, C), seed)
    free = np.flatnonzero(g0.reshape(-1) != 1)
    if len(free) == 0:
        g0[0, 0] = 0
        free = np.array([0])
    sources = [int(v) for v in rnd.choice(free, min(int(rnd.integers(1, 4)), len(free)), replace=False)]
    g1, c1 = rc.seeded_change(g0, c0, kind, int(rnd.integers(1, 5)), seed + 5)      # (a source may close, and open again later)
    return g0, c0, g1, c1, sources


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ad, rs", ck.POLICIES)
def test_the_model_is_the_fresh_dijkstra_bit_for_bit(ad, rs, kind):
    raised = labels = 0
    for seed in range(90):                                            # 4 policies x 4 kinds x 90 = 1 440 cases
        g0, c0, g1, c1, sources = seeded_case(1000 * (2 * ad + rs) + seed, kind)
        old, want = rc.fresh(g0, c0, sources, ad, rs), rc.fresh(g1, c1, sources, ad, rs)
        changed = rc.changed_cells(g0, c0, g1, c1)
        a = rc.repair(old, g1, c1, sources, changed, ad, rs, seed=seed)
        b = rc.repair(old, g1, c1, sources, changed, ad, rs, seed=seed + 100, tile=(2, 3))     # another order, and a queue of many tiles
        for got in (a, b):
            assert rc.same_bits(got.D, want), (seed, kind, ad, rs, np.argwhere(got.D != want)[:4])
        assert a.n_raised == b.n_raised and set(a.raised) == set(b.raised), (seed, kind, ad, rs)   # the surviving set is unique
        assert len(set(a.raised)) == a.n_raised                                                   # inf is never raised twice
        assert all(np.isfinite(old.reshape(-1)[v]) for v in a.raised)
        assert rc.raised_by_label_order(old, g1, c1, sources, ad, rs) == sorted(a.raised)          # the sweep-free derivation of the same set
        # a repair with nothing listed on an unchanged map moves nothing
        same = rc.repair(want, g1, c1, sources, [], ad, rs, seed=seed)
        assert same.n_raised == 0 and not same.lowered and not same.first and rc.same_bits(same.D, want)
        # ... and listing cells that did not change, twice, is harmless
        extra = rc.repair(old, g1, c1, sources, changed + changed + [0, g0.size - 1], ad, rs, seed=seed)
        assert rc.same_bits(extra.D, want) and extra.n_raised == a.n_raised
        raised += a.n_raised
        labels += old.size
    assert 0 < raised < labels


def test_changed_cells():
    g0 = np.array([[0, 1, 0, 1], [0, 0, 2, 3]])
    g1 = np.array([[0, 0, 1, 1], [0, 0, 0, 0]])
    c0 = np.array([[1.0, np.nan, 2.0, -5.0], [1.0, 4.0, 1.0, 1.0]])
    c1 = np.array([[1.0, 3.0, np.nan, np.nan], [1.5, 4.0, 1.0, 1.0]])
    assert rc.changed_cells(g0, c0, g1, c1) == [1, 2, 4]              # opened, closed, another cost; start / target marks are free cells
    assert rc.changed_cells(g0, c0, g0, c0) == [] and rc.changed_cells(g1, c1, g0, c0) == [1, 2, 4]
    from pathfit.cost_field import changed_cells
    got = changed_cells(g0, c0, g1, c1)
    assert got.dtype == np.int32 and got.tolist() == [1, 2, 4] and changed_cells(g0, c0, g0, c0).size == 0
    for seed in range(20):
        a0, k0, a1, k1, _ = seeded_case(seed, "int14")
        assert changed_cells(a0, k0, a1, k1).tolist() == rc.changed_cells(a0, k0, a1, k1)
    with pytest.raises(ValueError, match="^changed_cells: the shapes differ"):
        changed_cells(g0, c0, g1, np.ones((2, 5)))


# ---- the three wrong repairs
def test_a_repair_without_a_raise_phase_is_rejected():
    g0, g1, c, sources, (ad, rs) = rc.closed_corridor_case()
    old, want = rc.fresh(g0, c, sources, ad, rs), rc.fresh(g1, c, sources, ad, rs)
    changed = rc.changed_cells(g0, c, g1, c)
    assert changed == [3] and np.isinf(want[2, 0]) and np.isfinite(old[2, 0])
    good = rc.repair(old, g1, c, sources, changed, ad, rs)
    assert rc.same_bits(good.D, want) and good.n_raised == int(np.isfinite(old).sum() - np.isfinite(want).sum()) > 10
    bad = rc.repair(old, g1, c, sources, changed, ad, rs, variant="no_raise")
    assert bad.n_raised == 0 and not rc.same_bits(bad.D, want)
    assert bad.D[2, 0] == old[2, 0] < want[2, 0]                      # a label below the answer, which no lowering sweep repairs


def test_raising_only_along_legal_moves_from_a_changed_cell_is_rejected():
    g0, g1, c, sources, (ad, rs) = rc.corner_rule_case()
    assert (ad, rs) == (1, 1)
    old, want = rc.fresh(g0, c, sources, ad, rs), rc.fresh(g1, c, sources, ad, rs)
    changed = rc.changed_cells(g0, c, g1, c)
    assert changed == [4] and old[0, 1] == fc.SQRT2 and want[0, 1] == 2.0
    m0, m1 = fc.move_masks(g0, ad, rs), fc.move_masks(g1, ad, rs)
    assert (m0[1, 0] >> 6) & 1 and not (m1[1, 0] >> 6) & 1            # move 6 = (-1, +1): the diagonal (1, 0) -> (0, 1) past x
    assert m1[1, 1] == 0                                              # no legal move from x, and (0, 1), (1, 0) are orthogonal neighbours of x
    good = rc.repair(old, g1, c, sources, changed, ad, rs)
    assert rc.same_bits(good.D, want) and 1 in good.raised and 4 in good.raised
    bad = rc.repair(old, g1, c, sources, changed, ad, rs, variant="legal_from_changed")
    assert not rc.same_bits(bad.D, want) and bad.D[0, 1] == fc.SQRT2 < want[0, 1]
    # under the free policy the diagonal stays legal and the label stays
    old_f, want_f = rc.fresh(g0, c, sources, 1, 0), rc.fresh(g1, c, sources, 1, 0)
    keep = rc.repair(old_f, g1, c, sources, changed, 1, 0)
    assert rc.same_bits(keep.D, want_f) and 1 not in keep.raised and want_f[0, 1] == fc.SQRT2


def test_lowering_only_the_tiles_with_a_raised_word_is_rejected():
    g, c0, c1, sources, (ad, rs) = rc.falling_cost_case()
    old, want = rc.fresh(g, c0, sources, ad, rs), rc.fresh(g, c1, sources, ad, rs)
    assert old.tolist() == [[0.0, 2.0, 1.0, 0.0]] and want.tolist() == [[0.0, 1.0, 1.0, 0.0]]
    changed = rc.changed_cells(g, c0, g, c1)
    assert changed == [1]
    good = rc.repair(old, g, c1, sources, changed, ad, rs)
    assert good.n_raised == 0 and good.first == {(0, 0)} and good.lowered == {1} and rc.same_bits(good.D, want)
    bad = rc.repair(old, g, c1, sources, changed, ad, rs, variant="lower_touched_only")
    assert bad.n_raised == 0 and not bad.first and bad.D.tolist() == old.tolist() and not rc.same_bits(bad.D, want)


# ---- the CPU facts the GPU file leans on
def test_facts_of_the_door_maps():
    g, door, inside, sealed = rc.sealed_room_map()
    R, C = g.shape
    c, src = np.ones(g.shape), [1 * C + 1]
    old = rc.fresh(g, c, src, 1, 1)
    assert np.isfinite(old.reshape(-1)[inside]) and np.isfinite(old.reshape(-1)[door]) and np.isinf(old.reshape(-1)[sealed])
    g1 = g.copy()
    g1.reshape(-1)[door] = 1
    want = rc.fresh(g1, c, src, 1, 1)
    room = np.isfinite(old) & np.isinf(want)
    assert np.isinf(want.reshape(-1)[inside]) and room.sum() > 500    # the whole room goes, and the door
    rep = rc.repair(old, g1, c, src, [door], 1, 1)
    assert rc.same_bits(rep.D, want) and rep.n_raised >= room.sum() and len(rc.tiles_of(rep.raised, C)) >= 2
    back = rc.repair(want, g, c, src, [door], 1, 1)                   # the door opens again: nothing to raise, a room to lower
    assert back.n_raised == 0 and rc.same_bits(back.D, old) and len(back.lowered) == room.sum()
    g2 = g.copy()
    g2.reshape(-1)[sealed] = 1                                        # a closing where no source reaches: nothing raised, nothing lowered
    quiet = rc.repair(old, g2, c, src, [sealed], 1, 1)
    assert quiet.n_raised == 0 and not quiet.lowered and rc.same_bits(quiet.D, old) and rc.same_bits(rc.fresh(g2, c, src, 1, 1), old)


def test_facts_of_the_long_corridor():
    g, src, x = rc.long_corridor(200)
    c = np.ones(g.shape)
    old = rc.fresh(g, c, [src], 1, 1)
    g1 = g.copy()
    g1[0, x] = 1
    rep = rc.repair(old, g1, c, [src], [x], 1, 1)
    assert rep.n_raised == 199 and rc.tiles_of(rep.raised, 200) == {(0, 0), (0, 1), (0, 2), (0, 3)}
    assert rc.min_raise_launches(rep.raised, [x], 1, 200) == 4        # at least three tiles beyond the first: four raise launches under any timing
    assert rc.min_raise_launches([], [x], 1, 200) == 0
    s = fc.serpentine(41)                                             # one corridor down 21 free rows: three tiles of 16 rows
    c = ck.cost_of_kind("u50", s.shape, 6)
    s1 = s.copy()
    s1[0, 5] = 1
    gone = rc.raised_by_label_order(rc.fresh(s, c, [0], 1, 1), s1, c, [0], 1, 1)
    assert len(gone) > 400 and rc.tiles_of(gone, 41) == {(0, 0), (1, 0), (2, 0)} and rc.min_raise_launches(gone, [5], 41, 41) == 3


def test_facts_of_the_sources_that_close_and_open():
    g = np.zeros((5, 9), int)
    g[2, 4] = 1
    c = ck.cost_of_kind("u50", g.shape, 3)
    sets = [0, 2 * 9 + 4, 44]                                         # the middle one is listed ON an obstacle
    old = rc.fresh(g, c, sets, 1, 1)
    assert old[2, 4] == INF_ and old[0, 0] == 0.0 and old[4, 8] == 0.0
    g1 = g.copy()
    g1[2, 4], g1[0, 0] = 0, 1                                         # the listed obstacle opens; a source closes
    rep = rc.repair(old, g1, c, sets, rc.changed_cells(g, c, g1, c), 1, 1)
    assert rep.reseeded == [2 * 9 + 4] and 0 in rep.raised
    assert rc.same_bits(rep.D, rc.fresh(g1, c, sets, 1, 1)) and rep.D[2, 4] == 0.0 and rep.D[0, 0] == INF_
    assert ck.info_of(g1, rep.D, sets)[0] == 2 and ck.info_of(g, old, sets)[0] == 2


INF_ = float("inf")
