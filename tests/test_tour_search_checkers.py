"""The tour-search checkers pinned on a CPU-only host: the literal 2-opt loop against the numpy form word for word, what every
result must satisfy, brute force and Held-Karp below it, the cap, the four wrong solvers told from the rule, and the map fact the GPU
file leans on."""
import itertools

import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import tour_checkers as tc
import tour_search_checkers as ts

KINDS = ("ints", "uniform", "euclid", "asym", "tenths")
SIZES = (1, 2, 3, 4, 5, 6, 9, 17, 33, 70)


def words(r):
    order, value, status, info = r
    return [int(v) for v in order], tuple(tc.bits(x) for x in value), int(status), tuple(int(v) for v in info)


def start(d, mode):
    return tc.nearest_neighbour(ts.mirror(d), mode)[:len(d)]          # (n = 1 in mode 2: node 0 is the start and the end)


def cases(sizes=SIZES, kinds=KINDS):
    for kind, n, mode in itertools.product(kinds, sizes, ts.MODES):
        yield kind, n, mode, ts.matrix(kind, n, 3)


def test_the_literal_form_and_the_numpy_form_agree_word_for_word():
    for kind, n, mode, d in cases():
        for o in (start(d, mode), [0] + list(range(ts.hi_of(n, mode), 0, -1)) + ([n - 1] if mode == 2 and n > 1 else [])):
            assert words(ts.two_opt(d, o, mode, 16 * n)) == words(ts.two_opt_numpy(d, o, mode, 16 * n)), (kind, n, mode)


def test_every_result_is_a_permutation_with_its_ends_and_its_own_sum():
    for kind, n, mode, d in cases():
        o, value, status, info = ts.two_opt_numpy(d, start(d, mode), mode, 16 * n)
        assert status == 0 and tc.admissible(o, n, mode, None), (kind, n, mode)
        w = ts.mirror(d)
        t = w[o[0]][o[1]] if n > 1 else 0.0                           # the left-to-right sum, written out once more
        for a, b in zip(o[1:], o[2:] + ([o[0]] if mode == 1 and n > 1 else [])):
            t = t + w[a][b]
        assert float(t) == value[0] and value[0] == tc.route_cost(w, o, mode) and value[0] <= value[1]
        assert value[1] == tc.route_cost(w, start(d, mode), mode)
        assert info[1] == info[0] + 1 and info[2:] == (0, 0)
        assert ts.improving_pairs(d, o, mode) == [], (kind, n, mode)   # a local optimum, looked at independently


def test_only_the_upper_triangle_is_read():
    for kind, n, mode, d in cases(sizes=(5, 9, 17)):
        junk = d.copy()
        junk[np.tril_indices(n)] = np.nan
        assert words(ts.two_opt(junk, start(d, mode), mode, 16 * n)) == words(ts.two_opt(d, start(d, mode), mode, 16 * n))


def test_never_below_brute_force_or_held_karp():
    for kind, n, mode, d in cases(sizes=(2, 3, 4, 5, 6, 7, 8)):
        got = ts.two_opt_numpy(d, start(d, mode), mode, 16 * n)[1][0]
        assert got >= tc.brute_force(ts.mirror(d), mode)[0], (kind, n, mode)
    for kind, n, mode, d in cases(sizes=(9, 12)):
        got = ts.two_opt_numpy(d, start(d, mode), mode, 16 * n)[1][0]
        assert got >= tc.held_karp(ts.mirror(d), mode)[0], (kind, n, mode)


def test_the_cap():
    d = ts.matrix("euclid", 30, 4)
    for mode in ts.MODES:
        o = list(range(30))                                           # (seeded points in index order: a long way from any optimum)
        full = ts.two_opt(d, o, mode, 16 * 30)
        assert full[2] == 0 and full[3][0] >= 3
        for cap in (0, 1, full[3][0] - 1):
            got = ts.two_opt(d, o, mode, cap)
            assert got[2] == 2 and got[3][:2] == (cap, cap + 1) and words(got) == words(ts.two_opt_numpy(d, o, mode, cap))
            assert tc.admissible(got[0], 30, mode, None) and full[1][0] < got[1][0] <= got[1][1]
        assert ts.two_opt(d, o, mode, 0)[0] == o
        assert words(ts.two_opt(d, o, mode, full[3][0])) == words(full)      # exactly enough moves: status 0
        again = ts.two_opt(d, full[0], mode, 0)                       # a local optimum under a cap of 0: status 0, one sweep
        assert again[2] == 0 and again[3][:2] == (0, 1) and again[0] == full[0]


def test_a_problem_with_an_infinite_weight_is_not_searched():
    d = ts.matrix("uniform", 6, 1)
    d[4, 2] = ts.INF                                                  # (the lower triangle: ignored)
    assert ts.two_opt(d, start(d, 0), 0, 96)[2] == 0
    d[2, 4] = ts.INF
    for solve in (ts.two_opt, ts.two_opt_numpy):
        assert solve(d, list(range(6)), 0, 96) == ([-1] * 6, (ts.INF, ts.INF), 1, (0, 0, 0, 0))
    assert ts.search(d, 0)["feasible"] is False


@pytest.mark.parametrize("case,flag", [(ts.WRONG_LARGEST_ON_TIE, "largest_on_tie"), (ts.WRONG_FIRST_IMPROVEMENT, "first_improvement"),
                                       (ts.WRONG_OTHER_SUM, "other_sum"), (ts.WRONG_SKIP_LAST, "skip_last")])
def test_the_wrong_solvers_are_told_from_the_rule(case, flag):
    kind, n, mode, seed = case
    d = ts.matrix(kind, n, seed)
    o = start(d, mode)
    right = ts.two_opt(d, o, mode, 16 * n)
    assert words(right) == words(ts.two_opt_numpy(d, o, mode, 16 * n))
    assert words(ts.two_opt(d, o, mode, 16 * n, **{flag: True})) != words(right)


def test_the_validators():
    good = np.array([ts.matrix("uniform", 4, b) for b in range(3)])
    assert ts.first_bad_entry(good) is None
    bad = good.copy()
    bad[2, 0, 1], bad[1, 2, 3], bad[0, 3, 1], bad[0, 2, 2] = -1.0, np.nan, np.nan, -5.0      # (the last two: never read)
    assert ts.first_bad_entry(bad) == (1, 2, 3)
    bad[1, 2, 3] = 2.0 ** 1000
    assert ts.first_bad_entry(bad) == (2, 0, 1)
    bad[2, 0, 1] = 2.0 ** 1001
    assert ts.first_bad_entry(bad) == (2, 0, 1)
    bad[2, 0, 1] = ts.INF
    assert ts.first_bad_entry(bad) is None
    assert ts.first_bad_start([[0, 2, 1, 3], [0, 1, 2, 3]], 4, 2) is None
    assert ts.first_bad_start([[0, 2, 1, 3], [0, 3, 2, 1]], 4, 2) == (1, 3) and ts.first_bad_start([[0, 3, 2, 1]], 4, 0) is None
    assert ts.first_bad_start([[0, 2, 2, 3]], 4, 0) == (0, 2) and ts.first_bad_start([[1, 0, 2, 3]], 4, 0) == (0, 0)
    assert ts.first_bad_start([[0, 4, 2, 3]], 4, 0) == (0, 1) and ts.first_bad_start([[0, -1, 2, 3]], 4, 1) == (0, 1)


def test_the_rounds():
    d = ts.matrix("euclid", 40, 2)
    a = ts.search(d, 1, starts=6, rounds=4, seed=3)
    assert a == ts.search(d, 1, starts=6, rounds=4, seed=3, improve=ts.two_opt) and a != ts.search(d, 1, starts=6, rounds=4, seed=4)
    assert len(a["history"]) == 5 and all(x >= y for x, y in zip(a["history"], a["history"][1:])) and a["history"][-1] == a["total"]
    assert a["history"][-1] < a["history"][0] < a["start_total"]
    assert tc.admissible(a["order"], 40, 1, None) and tc.route_cost(ts.mirror(d), a["order"], 1) == a["total"]
    for n, mode in ((3, 0), (4, 2), (1, 1)):                         # hi < 3: no rounds
        assert len(ts.search(ts.matrix("uniform", n, 1), mode)["history"]) == 1
    assert len(ts.search(ts.matrix("uniform", 4, 1), 0, rounds=2)["history"]) == 3
    o = list(range(9))
    assert ts.double_bridge(o, (2, 4, 7)) == [0, 1, 4, 5, 6, 2, 3, 7, 8] and ts.double_bridge(o, (1, 2, 9)) == [0, 2, 3, 4, 5, 6, 7, 8, 1]


def test_the_map_fact():
    """On ts.MAP_STOPS the nearest-neighbour total, its 2-opt optimum and the total after the rounds are three different numbers."""
    g = np.asarray(gio.grid(ts.MAP)[0], np.uint8)
    assert ts.MAP_STOPS == tc.free_cells(g, 24, 2)
    mm = fc.move_masks(g, True, True)
    ids = [r * g.shape[1] + c for r, c in ts.MAP_STOPS]
    fields = np.array([fc.reference_dijkstra(g, mm, s)[0] for s in ids]).reshape(len(ids), -1)
    m = np.ascontiguousarray(fields[:, ids])
    assert (m != m.T).any()                                           # the gathered matrix is not symmetric as words: the rule mirrors it
    got = ts.search(m, 0, **ts.MAP_SEARCH)
    assert (got["start_total"], got["history"][0], got["total"]) == (ts.MAP_NN_TOTAL, ts.MAP_TWO_OPT_TOTAL, ts.MAP_ROUNDS_TOTAL)
    assert ts.MAP_NN_TOTAL > ts.MAP_TWO_OPT_TOTAL > ts.MAP_ROUNDS_TOTAL
