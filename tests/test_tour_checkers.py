"""The tour checkers against each other (any host): the literal Held-Karp rule equals brute force over permutations bit for bit, the
numpy layer form equals the literal form, the returned order's left-to-right sum is the total, infeasible problems give the all -1
row -- and the checker tells four wrong solvers from the rule, each on a seeded case kept in tour_checkers.py.  Also the map fact
tests/test_gpu_tour.py leans on: a set of stops on the golden 20 x 20 map on which the greedy order is strictly dearer."""
import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import tour_checkers as tc


def needs_for(n, mode, which):
    """None, two precedence pairs, or a cycle among the first two middle nodes (None where the problem has too few)."""
    mid = tc.middle(n, mode)
    if which == "none":
        return None
    if len(mid) < 2:
        return False
    need = [0] * n
    if which == "pairs":
        need[mid[0]] |= 1 << mid[-1]
        if len(mid) >= 3:
            need[mid[1]] |= 1 << mid[2]
    else:
        need[mid[0]] |= 1 << mid[1]
        need[mid[1]] |= 1 << mid[0]
    return need


def same(a, b):
    return (tc.bits(a[0]), list(a[1]), a[2], a[3]) == (tc.bits(b[0]), list(b[1]), b[2], b[3])


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("kind", tc.KINDS)
def test_the_rule_equals_brute_force_bit_for_bit(kind, mode):
    cases = 0
    for n in range(1, 9):
        if mode == 2 and n < 2:
            continue
        for seed in range(2 if n < 8 else 1):
            d = tc.matrix(kind, n, seed)
            for which in ("none", "pairs", "cycle"):
                need = needs_for(n, mode, which)
                if need is False:
                    continue
                total, order, finite, last = tc.held_karp(d, mode, need)
                best, _ = tc.brute_force(d, mode, need)
                assert tc.bits(total) == tc.bits(best), (kind, n, mode, seed, which)
                if which == "cycle":
                    assert total == tc.INF
                if total < tc.INF:
                    assert tc.admissible(order, n, mode, need), (order, need)
                    assert tc.bits(tc.route_cost(d, order, mode)) == tc.bits(total)
                    assert last == (order[-2] if mode == 2 else order[-1]) or tc.middle(n, mode) == []
                else:
                    assert order == [-1] * n and last == -1
                cases += 1
    assert cases >= 30


@pytest.mark.parametrize("mode", tc.MODES)
def test_the_numpy_layers_equal_the_literal_form_up_to_m_10(mode):
    for m in range(0, 11):
        n = m + (2 if mode == 2 else 1)
        for kind in (tc.KINDS if m <= 8 else ("ints", "holes")):
            d = tc.matrix(kind, n, 3)
            for which in ("none", "pairs", "cycle"):
                need = needs_for(n, mode, which)
                if need is False:
                    continue
                assert same(tc.held_karp_layers(d, mode, need), tc.held_karp(d, mode, need)), (m, kind, which)


def test_a_chain_of_needs_leaves_one_order():
    for mode in tc.MODES:
        n = 7
        perm = [3, 1, 5, 2, 4] + ([6] if mode != 2 else [])
        d = tc.matrix("asym", n, 4)
        total, order, finite, last = tc.held_karp(d, mode, tc.chain_need(n, mode, perm))
        assert order == [0] + perm + ([6] if mode == 2 else [])
        assert tc.bits(total) == tc.bits(tc.route_cost(d, order, mode))
        assert finite == len(perm)                                    # one finite state per prefix


def test_a_middle_node_that_needs_the_end_is_infeasible():
    d = tc.matrix("asym", 5, 0)
    need = [0, 0, 1 << 4, 0, 0]
    assert tc.held_karp(d, 2, need)[:2] == (tc.INF, [-1] * 5)
    assert tc.brute_force(d, 2, need)[0] == tc.INF
    need = [0, 0, 0, 0, 1 << 2]                                       # the end's own needs are always met
    assert same(tc.held_karp(d, 2, need), tc.held_karp(d, 2, None))


def test_an_unreachable_stop_is_infeasible():
    d = tc.matrix("uniform", 6, 0)
    d[:, 3] = tc.INF
    for mode in tc.MODES:
        assert tc.held_karp(d, mode)[:2] == (tc.INF, [-1] * 6)
        assert tc.held_karp_layers(d, mode)[:2] == (tc.INF, [-1] * 6)


def test_m_0():
    assert tc.held_karp(np.zeros((1, 1)), 0) == (0.0, [0], 0, -1)
    assert tc.held_karp(np.zeros((1, 1)), 1) == (0.0, [0], 0, -1)
    assert tc.held_karp(np.array([[0.0, 2.5], [7.0, 0.0]]), 2) == (2.5, [0, 1], 0, -1)
    assert tc.held_karp(np.array([[0.0, tc.INF], [7.0, 0.0]]), 2) == (tc.INF, [-1, -1], 0, -1)


# ---- the checker rejects four wrong solvers
def test_rejects_a_solver_that_sums_right_to_left():
    kind, n, mode, seed = tc.WRONG_RIGHT_TO_LEFT
    d = tc.matrix(kind, n, seed)
    right, wrong = tc.held_karp(d, mode), tc.held_karp(d, mode, right_to_left=True)
    assert tc.bits(right[0]) == tc.bits(tc.brute_force(d, mode)[0])
    assert tc.bits(wrong[0]) != tc.bits(right[0])
    assert abs(wrong[0] - right[0]) < 1e-12                           # (the same optimum in exact arithmetic)


def test_rejects_a_solver_that_takes_the_largest_index_on_a_tie():
    kind, n, mode, seed = tc.WRONG_LARGEST_ON_TIE
    d = tc.matrix(kind, n, seed)
    right, wrong = tc.held_karp(d, mode), tc.held_karp(d, mode, largest_on_tie=True)
    assert tc.bits(wrong[0]) == tc.bits(right[0]) and wrong[1] != right[1]


def test_rejects_a_solver_that_ignores_need_and_one_that_applies_it_to_the_final_set_only():
    kind, n, mode, seed, need = tc.WRONG_NEED
    d = tc.matrix(kind, n, seed)
    right = tc.held_karp(d, mode, need)
    assert tc.bits(right[0]) == tc.bits(tc.brute_force(d, mode, need)[0]) and tc.admissible(right[1], n, mode, need)
    ignores = tc.held_karp(d, mode, None)
    assert ignores[0] < right[0] and not tc.admissible(ignores[1], n, mode, need)
    final_only = tc.held_karp(d, mode, need, need_final_only=True)
    assert final_only[0] < right[0] and not tc.admissible(final_only[1], n, mode, need)


# ---- the map fact of the GPU file
def test_the_greedy_order_is_dearer_on_the_golden_map():
    g = gio.grid(tc.NN_MAP)[0]
    C = g.shape[1]
    mm = fc.move_masks(g, 1, 1)
    ids = [r * C + c for r, c in tc.NN_STOPS]
    assert all(g.reshape(-1)[v] != 1 for v in ids)
    d = np.array([fc.reference_dijkstra(g, mm, s)[0].reshape(-1)[ids] for s in ids])
    best = tc.held_karp(d, 0)
    greedy = tc.nearest_neighbour(d, 0)
    assert best[0] == 49.62741699796952 and tc.route_cost(d, greedy, 0) == 61.45584412271571
    assert tc.route_cost(d, greedy, 0) > best[0] == tc.brute_force(d, 0)[0]
