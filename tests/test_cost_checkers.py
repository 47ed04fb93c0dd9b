"""The cost-field checkers pinned against each other on any host (tests/cost_checkers.py): the heap Dijkstra, random-order sweeps run
to a fixed point, the field-only parent rule and the left-to-right path cost agree bit for bit on seeded maps up to 18 x 23 under the
four move policies; at cost == 1 they are field_checkers.reference_dijkstra; and a deliberately wrong rounding order is rejected."""
import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc

SHAPES = [(18, 23), (7, 11), (1, 9), (12, 2)]


def case(shape, seed):
    g = fc.seeded_map(shape[0], shape[1], 0.25, seed)
    free = np.flatnonzero(g.reshape(-1) != 1)
    rnd = np.random.default_rng(seed + 1)
    sets = [[int(v) for v in rnd.choice(free, min(n, len(free)), replace=False)] for n in (1, 2, 3)]
    return g, sets


@pytest.mark.parametrize("kind", ck.KINDS)
@pytest.mark.parametrize("ad, rs", ck.POLICIES)
def test_heap_sweeps_rule_and_path_cost_agree(kind, ad, rs):
    for i, shape in enumerate(SHAPES):
        g, sets = case(shape, 40 + i)
        cost = ck.cost_of_kind(kind, g.shape, 7 * i + len(kind))
        mm = fc.move_masks(g, ad, rs)
        for j, s in enumerate(sets):
            d, p = ck.dijkstra(g, mm, cost, s)
            sw = ck.sweeps(g, mm, cost, s, seed=100 * i + j)
            assert np.array_equal(d, sw), (shape, kind, ad, rs, j)              # bit for bit: inf == inf, no NaN anywhere
            assert np.array_equal(ck.rule_parents(d, mm, cost), p), (shape, kind, ad, rs, j)
            assert np.all((d == 0.0) == (p == ck.SOURCE)) and np.all(np.isinf(d) == (p == ck.NONE))
            for t in np.flatnonzero(np.isfinite(d).reshape(-1))[::5]:
                cells = fc.trace(p, int(t))
                assert ck.path_cost(cost, cells, g.shape[1]) == d.reshape(-1)[t], (shape, kind, ad, rs, j, int(t))
            info = ck.info_of(g, d, s)
            assert info[0] == len(set(s)) and info[1] == int(np.isfinite(d).sum()) and info[3] == 0
            assert d.reshape(-1)[info[2]] == d[np.isfinite(d)].max()


@pytest.mark.parametrize("ad, rs", ck.POLICIES)
def test_unit_cost_is_the_reference_dijkstra(ad, rs):
    for i, shape in enumerate(SHAPES):
        g, sets = case(shape, 60 + i)
        mm = fc.move_masks(g, ad, rs)
        cost = np.ones(g.shape)
        for k in range(8):
            assert np.all(ck.weights_into(cost, k) == fc.W[k])
        d0, p0 = fc.reference_dijkstra(g, mm, sets[0][0])
        d, p = ck.dijkstra(g, mm, cost, sets[0])
        assert np.array_equal(d, d0) and np.array_equal(p, p0)
        assert np.array_equal(ck.rule_parents(d, mm, cost), fc.rule_parents(d0, mm))
        # a set: the elementwise minimum of its sources' reference fields
        d3, _ = ck.dijkstra(g, mm, cost, sets[2])
        assert np.array_equal(d3, np.minimum.reduce([fc.reference_dijkstra(g, mm, s)[0] for s in sets[2]]))


def test_weight_is_symmetric_and_rounded_once():
    c = np.array([1.0, 3.7, 2.0 ** 20, 1.0 + 2.0 ** -52])
    for u in range(4):
        for v in range(4):
            for k in (0, 5):
                assert ck.weight(c, u, v, k) == ck.weight(c, v, u, k)
    assert ck.weight(c, 0, 0, 0) == 1.0 and ck.weight(c, 0, 0, 4) == ck.SQRT2
    assert ck.weight(c, 2, 2, 7) == ck.SQRT2 * 2.0 ** 20


def test_sources_on_obstacles_duplicates_and_empty_sets():
    g = np.zeros((5, 6), np.uint8)
    g[2, :5] = 1
    cost = ck.cost_of_kind("u50", g.shape, 3)
    mm = fc.move_masks(g, 1, 1)
    d, p = ck.dijkstra(g, mm, cost, [12, 13])                                     # both on the wall
    assert np.all(np.isinf(d)) and np.all(p == ck.NONE) and ck.info_of(g, d, [12, 13]) == [0, 0, -1, 0]
    d1, p1 = ck.dijkstra(g, mm, cost, [0, 12, 0])
    d2, p2 = ck.dijkstra(g, mm, cost, [0])
    assert np.array_equal(d1, d2) and np.array_equal(p1, p2) and ck.info_of(g, d1, [0, 12, 0])[0] == 1
    assert np.array_equal(ck.owners(p1, [0, 12, 0]), np.where(np.isfinite(d1), 0, -1))


@pytest.mark.parametrize("variant", ["split_diag", "presum"])
def test_a_wrong_rounding_order_is_rejected(variant):
    """The checker sees the ORDER of the rounded additions: a solver that forms a label another way -- the diagonal in two steps,
    or two moves summed ahead -- differs from the heap on at least one seeded case."""
    rejected = 0
    for i in range(6):
        g, sets = case((18, 23), 80 + i)
        cost = ck.cost_of_kind("u50", g.shape, i)
        mm = fc.move_masks(g, 1, 1)
        d, _ = ck.dijkstra(g, mm, cost, sets[0])
        assert np.array_equal(ck.sweeps(g, mm, cost, sets[0], seed=i), d)
        rejected += not np.array_equal(ck.sweeps(g, mm, cost, sets[0], seed=i, variant=variant), d)
    assert rejected >= 1
