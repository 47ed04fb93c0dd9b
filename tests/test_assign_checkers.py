"""The assignment checkers against themselves (any host): the rule's literal form against brute force over all injections, the numpy
form against the literal form word for word, the duals on integer matrices, the step count of the product matrix, five wrong solvers
each rejected on a seeded case kept in assign_checkers.py, and the map fact tests/test_gpu_assign.py leans on."""
from fractions import Fraction

import numpy as np
import pytest

import assign_checkers as ac
import field_checkers as fc
import golden_io as gio

SHAPES = [(1, 1), (1, 3), (2, 2), (3, 3), (3, 5), (4, 4), (4, 7), (5, 5), (5, 6), (6, 6), (6, 7)]
SEEDS = (0, 1, 2)


@pytest.mark.parametrize("kind", ac.INT_KINDS)
def test_the_literal_form_equals_brute_force_on_integer_kinds(kind):
    infeasible = cases = 0
    for n, m in SHAPES:
        for seed in SEEDS:
            a = ac.matrix(kind, n, m, seed)
            best_sum, best_max, best_max_sum = ac.brute(a)
            r0, r1, r2 = (ac.solve(a, mode) for mode in ac.MODES)
            cases += 1
            if best_sum == ac.INF:
                infeasible += 1
                for r in (r0, r1, r2):
                    assert r.status == 1 and r.col == [-1] * n and r.sum == r.max == ac.INF and not r.dual.any() and 0 <= r.info[2] < n
                continue
            for r in (r0, r1, r2):
                assert r.status == 0 and sorted(set(r.col)) == sorted(r.col) and min(r.col) >= 0 and r.info[2] == -1
                s, mx = ac.assignment_cost(a, r.col)
                assert (ac.bits(r.sum), r.max) == (ac.bits(s), mx)
            assert ac.bits(r0.sum) == ac.bits(best_sum), (kind, n, m, seed)
            assert r1.max == best_max, (kind, n, m, seed)
            assert (r2.max, ac.bits(r2.sum)) == (best_max, ac.bits(best_max_sum)), (kind, n, m, seed)
            assert r0.info[1] == 0 and r1.info[0] == 0 and r2.info[0] > 0 and r2.info[1] == r1.info[1] and not r1.dual.any()
    if kind in ("inf30", "inf55"):
        assert infeasible > 0
    if kind == "inf55":
        assert 5 * infeasible >= cases, (infeasible, cases)           # at least a fifth


@pytest.mark.parametrize("kind", ac.REAL_KINDS)
def test_real_valued_kinds_the_makespan_is_exact_and_the_sum_is_never_below_brute_force(kind):
    worst_gap, worst_cert = 0.0, Fraction(0)
    for n, m in SHAPES:
        for seed in SEEDS:
            a = ac.matrix(kind, n, m, seed)
            best_sum, best_max, best_max_sum = ac.brute(a)
            r0, r1, r2 = (ac.solve(a, mode) for mode in ac.MODES)
            assert r1.max == best_max and r2.max == best_max
            assert r0.sum >= best_sum and r2.sum >= best_max_sum
            worst_gap = max(worst_gap, r0.sum - best_sum, r2.sum - best_max_sum)
            worst_cert = max(worst_cert, ac.certificate(a, r0))
    print(kind, "worst gap", worst_gap, "worst certificate", float(worst_cert))
    # the rule is held to its model and not to a tolerance: the gap measured on this seeded set is 0, and stays 0
    assert worst_gap == ac.WORST_GAP == 0.0
    assert float(worst_cert) <= 4 * ac.WORST_CERTIFICATE


@pytest.mark.parametrize("mode", ac.MODES)
def test_the_numpy_form_equals_the_literal_form_word_for_word(mode):
    shapes = SHAPES + [(17, 17), (30, 33), (1, 64), (63, 64), (64, 64), (65, 65), (40, 70), (70, 70)]
    for n, m in shapes:
        for kind in ac.KINDS:
            if n > 40 and kind not in ("ties", "inf30", "sqrt2"):
                continue
            a = ac.matrix(kind, n, m, 4)
            assert ac.words(ac.solve_np(a, mode)) == ac.words(ac.solve(a, mode)), (kind, n, m, mode)
    a = ac.product(24)
    assert ac.words(ac.solve_np(a, mode)) == ac.words(ac.solve(a, mode))


def test_the_duals_on_integer_matrices():
    for kind in ac.INT_KINDS:
        for n, m in SHAPES + [(20, 31)]:
            for mode in (0, 2):
                a = ac.matrix(kind, n, m, 6)
                r = ac.solve(a, mode)
                if r.status:
                    continue
                u, v = r.dual[:n], r.dual[n:]
                lim = ac.INF if mode == 0 else r.max                  # mode 2 reads an entry above t as +inf
                al = np.where(a > lim, ac.INF, a)
                assert np.all(u[:, None] + v[None, :] <= al)
                assert all(u[i] + v[c] == a[i, c] for i, c in enumerate(r.col))
                assert np.all(v <= 0) and all(v[j] == 0 for j in range(m) if j not in r.col)
                assert u.sum() + v.sum() == r.sum
                assert ac.certificate(al, r) == 0


@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_the_product_matrix_takes_the_most_steps(n):
    r = ac.solve_np(ac.product(n), 0)
    assert r.info == [n * (n + 1) // 2, 0, -1, 0] and r.col == list(range(n - 1, -1, -1))
    assert ac.solve_np(ac.product(n), 2).info[:2] == [n * (n + 1) // 2, ac.solve_np(ac.product(n), 1).info[1]]


def case(spec):
    kind, n, m, mode, seed = spec
    return ac.matrix(kind, n, m, seed), mode


def test_wrong_largest_column_on_a_tie_is_rejected():
    a, mode = case(ac.WRONG_LARGEST_ON_TIE)
    good, bad = ac.solve(a, mode), ac.solve(a, mode, largest_on_tie=True)
    assert ac.words(good) != ac.words(bad) and ac.words(good) == ac.words(ac.solve_np(a, mode))
    assert good.sum == bad.sum == ac.brute(a)[0]                      # (both optimal: only the rule tells them apart)


def test_wrong_fused_potentials_are_rejected():
    a, mode = case(ac.WRONG_FUSED)
    good, bad = ac.solve(a, mode), ac.solve(a, mode, fused_potentials=True)
    assert ac.words(good) != ac.words(bad) and ac.words(good) == ac.words(ac.solve_np(a, mode))


def test_wrong_right_to_left_sum_is_rejected():
    a, mode = case(ac.WRONG_RIGHT_TO_LEFT)
    good, bad = ac.solve(a, mode), ac.solve(a, mode, right_to_left=True)
    assert good.col == bad.col and ac.bits(good.sum) != ac.bits(bad.sum)


def test_wrong_mode_2_without_the_limit_is_rejected():
    a, mode = case(ac.WRONG_IGNORES_LIMIT)
    assert mode == 2
    good, bad = ac.solve(a, 2), ac.solve(a, 2, ignore_limit=True)
    assert bad.col == ac.solve(a, 0).col and good.col != bad.col
    assert good.max == ac.solve(a, 1).max < bad.max and good.sum > bad.sum


def test_wrong_greedy_pairing_is_rejected():
    a, mode = case(ac.WRONG_GREEDY)
    good, bad = ac.solve(a, mode), ac.wrong_greedy(a, mode)
    assert bad.status == 0 and bad.sum > good.sum == ac.brute(a)[0]


def test_greedy_nearest_and_assignment_cost():
    a = np.array([[1.0, 2.0, 9.0], [1.0, ac.INF, ac.INF], [ac.INF, ac.INF, ac.INF]])
    assert ac.greedy_nearest(a) == [0, -1, -1] and ac.greedy_nearest(a[:2, :]) == [0, -1]
    assert ac.assignment_cost(a, [1, 0, -1]) == (3.0, 2.0) and ac.assignment_cost(a, [-1, -1, -1]) == (0.0, -ac.INF)
    assert ac.solve(a[:2], 0).col == [1, 0] and ac.solve(a, 0).status == 1 and ac.solve(a, 0).info[2] == 2


def test_the_map_fact():
    """Eight robots and eight tasks on the golden 20 x 20 map: the nearest-task greedy pairing costs more than the optimum."""
    g = gio.grid(ac.GREEDY_MAP)[0]
    C = g.shape[1]
    mm = fc.move_masks(g, 1, 1)
    rows = [fc.reference_dijkstra(g, mm, r * C + c)[0].reshape(-1) for r, c in ac.GREEDY_ROBOTS]
    a = np.array([[row[r * C + c] for r, c in ac.GREEDY_TASKS] for row in rows])
    assert len(ac.GREEDY_ROBOTS) == len(ac.GREEDY_TASKS) == 8 and np.all(a < ac.INF)
    opt = ac.solve(a, 0)
    greedy = ac.assignment_cost(a, ac.greedy_nearest(a))[0]
    assert opt.sum == ac.GREEDY_OPTIMUM == 50.071067811865476 and greedy == ac.GREEDY_COST == 73.97056274847715 > opt.sum
    assert ac.solve(a, 1).max == ac.solve(a, 2).max <= opt.max
