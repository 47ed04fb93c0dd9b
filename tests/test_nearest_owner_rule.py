"""The checkers of the nearest-source tests check themselves (any host, no GPU).  Three identities, all bit for bit:
the table of a Dijkstra seeded with a whole set is the elementwise minimum of the single-source tables; the field-only parent rule
applied to it gives the seeded search's came_from codes; and the field of the source that owns a cell equals the merged label
there.  The owner is the root of the tree, which is NOT always the lowest index among the tied sources."""
import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import nearest_checkers as nc

SIZES = (1, 2, 5, 17)


def maps():
    return {"open9x11": np.zeros((9, 11), np.uint8), "fig7": (gio.grid("fig7")[0] == 1).astype(np.uint8), "seeded18x23": fc.seeded_map(),
            "serpentine12": fc.serpentine(12)}


def case(g, ad, rs, sources):
    """-> (merged table, codes, owners, counts, the single-source tables)"""
    mm = fc.move_masks(g, ad, rs)
    merged, code = nc.multi_dijkstra(g, mm, sources)
    own, count = nc.owners_of(code, sources)
    single = np.stack([fc.reference_dijkstra(g, mm, s)[0] for s in sources])
    return mm, merged, code, own, count, single


@pytest.mark.parametrize("name", ["open9x11", "fig7", "seeded18x23", "serpentine12"])
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_three_identities(name, ad, rs):
    g = maps()[name]
    for S, sources in zip(SIZES, nc.seeded_sets(g, SIZES, seed=11)):
        mm, merged, code, own, count, single = case(g, ad, rs, sources)
        assert np.array_equal(merged, single.min(axis=0)), (name, ad, rs, S)
        assert np.array_equal(fc.rule_parents(merged, mm), code), (name, ad, rs, S)
        reach = np.isfinite(merged)
        assert np.array_equal(own >= 0, reach) and np.array_equal(code == fc.NONE, ~reach)
        assert (code == fc.SOURCE).sum() == len(sources) and count.sum() == reach.sum()
        flat_own, flat = own.reshape(-1), merged.reshape(-1)
        for v in np.flatnonzero(reach):
            assert single[flat_own[v]].reshape(-1)[v] == flat[v], (name, ad, rs, S, v)
            p = fc.trace(code, int(v))                                # the trace stops at the first code 8: the owner's cell
            assert p[0] == sources[flat_own[v]] and p[-1] == v


def test_the_owner_is_not_always_argmin():
    """The tie rule is really exercised: on these maps some cells are owned by another source than the lowest tied index."""
    differ = 0
    for name, g in maps().items():
        for ad, rs in fc.POLICIES:
            for sources in nc.seeded_sets(g, SIZES, seed=11):
                _, merged, _, own, _, single = case(g, ad, rs, sources)
                reach = np.isfinite(merged)
                differ += int((own[reach] != np.argmin(single, axis=0)[reach]).sum())
    assert differ > 0
    print("cells whose owner is not argmin:", differ)


def test_duplicates_and_obstacles_in_a_set():
    g = maps()["fig7"]
    wall = int(np.flatnonzero(g.reshape(-1) == 1)[0])
    a, b = nc.seeded_sets(g, [2], seed=5)[0]
    mm, merged, code, own, count, _ = case(g, 1, 1, [a, wall, b, a])
    assert np.array_equal(merged, nc.multi_dijkstra(g, mm, [a, b])[0])
    assert own.reshape(-1)[a] == 0 and own.reshape(-1)[b] == 2 and count[1] == 0 and count[3] == 0 and count.sum() == np.isfinite(merged).sum()
    merged, code = nc.multi_dijkstra(g, mm, [wall])
    assert np.all(np.isinf(merged)) and np.all(code == fc.NONE) and np.all(nc.owners_of(code, [wall])[0] == -1)


@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_wrong_tie_break_gives_other_owners(ad, rs):
    """On the open map ties are everywhere: the LARGEST u among the cells that offer the label hangs cells under other roots."""
    g = maps()["open9x11"]
    sources = nc.seeded_sets(g, [5], seed=11)[0]
    mm, merged, code, own, _, _ = case(g, ad, rs, sources)
    wrong = fc.rule_parents(merged, mm, largest_u=True)
    assert not np.array_equal(nc.owners_of(wrong, sources)[0], own)
    assert np.array_equal(nc.owners_of(fc.rule_parents(merged, mm), sources)[0], own)
