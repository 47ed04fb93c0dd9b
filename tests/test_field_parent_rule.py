"""The checker of the routing-tree tests checks itself (any host, no GPU): the field-only parent rule of tests/field_checkers.py
gives the parents -- hence the paths -- of a reference-shaped Dijkstra (heap entries (g, cell), closed set, strict-< parent), and
a wrong tie-break does not."""
import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio


def maps():
    return {"open9x11": np.zeros((9, 11), np.uint8), "fig7": (gio.grid("fig7")[0] == 1).astype(np.uint8), "seeded18x23": fc.seeded_map()}


def sources_of(g, n=4, seed=3):
    free = np.flatnonzero(g.reshape(-1) != 1)
    picks = np.random.default_rng(seed).choice(free, n - 2, replace=False)
    return [int(free[0]), int(free[len(free) // 2])] + [int(v) for v in picks]


@pytest.mark.parametrize("name", ["open9x11", "fig7", "seeded18x23"])
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_rule_gives_the_reference_shaped_parents(name, ad, rs):
    g = maps()[name]
    mm = fc.move_masks(g, ad, rs)
    C = g.shape[1]
    for s in sources_of(g):
        dist, code = fc.reference_dijkstra(g, mm, s)
        assert dist.reshape(-1)[s] == 0.0 and code.reshape(-1)[s] == fc.SOURCE
        rule = fc.rule_parents(dist, mm)
        assert np.array_equal(rule, code), (name, ad, rs, s)
        assert np.array_equal(rule == fc.NONE, np.isinf(dist))
        for t in range(g.size):                                       # every cell as a target: the traced paths agree too
            p = fc.trace(rule, t)
            assert p == fc.trace(code, t)
            if np.isinf(dist.reshape(-1)[t]):
                assert p == []
                continue
            assert p[0] == s and p[-1] == t and len(set(p)) == len(p)
            length = 0.0
            for a, b in zip(p[:-1], p[1:]):                           # the path's left-to-right fp64 length is the label
                k = [i for i in range(8) if fc.DR[i] * C + fc.DC[i] == b - a and abs(b % C - a % C) <= 1]
                assert len(k) == 1 and (mm.reshape(-1)[a] >> k[0]) & 1
                length += fc.W[k[0]]
            assert length == dist.reshape(-1)[t]


def test_source_on_an_obstacle_reaches_nothing():
    g = maps()["fig7"]
    s = int(np.flatnonzero(g.reshape(-1) == 1)[0])
    dist, code = fc.reference_dijkstra(g, fc.move_masks(g, 1, 1), s)
    assert np.all(np.isinf(dist)) and np.all(code == fc.NONE)
    assert np.all(fc.rule_parents(dist, fc.move_masks(g, 1, 1)) == fc.NONE)


@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_wrong_tie_break_is_rejected(ad, rs):
    """On the open map ties are everywhere: taking the LARGEST u among the cells that offer the final label gives other parents."""
    g = maps()["open9x11"]
    mm = fc.move_masks(g, ad, rs)
    s = 4 * 11 + 5
    dist, code = fc.reference_dijkstra(g, mm, s)
    wrong = fc.rule_parents(dist, mm, largest_u=True)
    assert not np.array_equal(wrong, code)
    assert any(fc.trace(wrong, t) != fc.trace(code, t) for t in range(g.size))
    assert np.array_equal(fc.rule_parents(dist, mm), code)


def test_serpentine_is_one_corridor():
    g = fc.serpentine(8)
    dist, code = fc.reference_dijkstra(g, fc.move_masks(g, 1, 1), 0)
    assert np.isfinite(dist).sum() == (g != 1).sum()
    assert len(fc.trace(code, int(np.argmax(np.where(np.isfinite(dist), dist, -1))))) > (g != 1).sum() // 2
