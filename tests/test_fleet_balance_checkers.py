"""The min-max fleet checkers pinned on a CPU-only host: the literal loop against the numpy form word for word, what the exact
(integer) case guarantees move by move, brute force below the result, one robot against the sum rule, the capped runs of the
seeded set, the six wrong solvers told from the rule, and the map facts the GPU file, DESIGN.md 4.32 and the README lean on."""
import itertools

import numpy as np

import fleet_balance_checkers as fb
import fleet_checkers as fl
import tour_checkers as tc
from test_fleet_checkers import map_matrix

KINDS = ("euclid", "ints", "tenths", "holes")
SHAPES = ((1, 1), (1, 2), (2, 1), (1, 5), (2, 2), (2, 5), (3, 1), (3, 6), (4, 9), (5, 3), (5, 12), (3, 22), (5, 35))


def words(r):
    route, lens, value, status, info = r
    return [int(v) for v in route], tuple(tc.bits(x) for x in lens), tuple(tc.bits(x) for x in value), int(status), tuple(int(v) for v in info)


def ceil_caps(k, n, slack=0):
    return [-(-n // k) + slack] * k


def starts_of(k, n, cap, seed=3):
    """A seeded start (routes may be empty) and, without caps, all tasks on the last robot."""
    rows = [fl.random_row(k, n, seed, cap)]
    if cap is None:
        rows.append(fl.row_of([[] for _ in range(k - 1)] + [list(range(k, k + n))]))
    return rows


def cases(shapes=SHAPES, kinds=KINDS):
    for kind, (k, n), mode in itertools.product(kinds, shapes, fl.MODES):
        for cap in (None, ceil_caps(k, n, 1)):
            yield kind, k, n, mode, cap, fl.matrix(kind, k + n, 3)


def test_the_literal_form_and_the_numpy_form_agree_word_for_word():
    seen, two, relocations, lowered = set(), 0, 0, 0
    for kind, k, n, mode, cap, d in cases():
        for o in starts_of(k, n, cap):
            if k + n > 20 and (kind != "euclid" or cap is not None or mode == 1):
                continue                                              # (the literal loop is slow: the large shapes once per kind)
            a = fb.balance(d, o, k, mode, cap, 16 * (k + n))
            assert words(a) == words(fb.balance_numpy(d, o, k, mode, cap, 16 * (k + n))), (kind, k, n, mode, cap)
            seen.add(a[3])
            two, relocations, lowered = two + a[4][2], relocations + a[4][3], lowered + a[4][4]
    assert two > 20 and relocations > 100 and lowered > 100 and {0, 1} <= seen
    d, o = fl.matrix("euclid", 40, 3), fl.random_row(5, 35, 3)        # the form that was not chosen, once
    assert words(fb.balance(d, o, 5, 0, None, 30, carry="recomputed")) == words(fb.balance_numpy(d, o, 5, 0, None, 30, carry="recomputed"))


def test_the_robot_a_tie_names_changes_nothing():
    for kind, k, n, mode, cap, d in cases(shapes=((2, 2), (3, 6), (4, 9), (5, 3)), kinds=("ints", "tenths")):
        for o in starts_of(k, n, cap):                                # (balance asserts the pick among three against the plain maximum)
            assert words(fb.balance(d, o, k, mode, cap, 16 * (k + n))) == words(fb.balance(d, o, k, mode, cap, 16 * (k + n), last_robot_on_tie=True))
    assert fb.top_three([2.0, 5.0, 5.0, 1.0]) == [(5.0, 1), (5.0, 2), (2.0, 0)] and fb.top_three([2.0, 5.0, 5.0], True)[0] == (5.0, 2)
    assert fb.top_three([4.0]) == [(4.0, 0), (-fb.INF, -1), (-fb.INF, -1)] and fb.pick(fb.top_three([4.0]), (0,)) == -fb.INF
    assert fb.pick(fb.top_three([3.0, 9.0, 7.0, 8.0]), (1, 3)) == 7.0 and fb.pick(fb.top_three([3.0, 9.0]), (0, 1)) == -fb.INF


def test_on_integers_every_move_lowers_the_key_no_row_recurs_and_a_status_0_row_is_a_local_optimum():
    moves = optima = 0
    for kind, k, n, mode, cap, d in cases(kinds=("ints",)):
        if k + n > 20:
            continue
        w = fl.mirror(d)
        for o in starts_of(k, n, cap):
            trace = []
            route, lens, value, status, info = fb.balance(d, o, k, mode, cap, 16 * (k + n), trace=trace)
            rows = {tuple(o)}
            for sp, delta, code, i, j, was, now in trace:
                a, b = fb.key_of(w, was, k, mode), fb.key_of(w, now, k, mode)
                assert b < a and b[0] == sp and b[1] - a[1] == delta, (k, n, mode, cap, code, i, j)      # (span, total) as summed from the rows
                assert tuple(now) not in rows and fl.valid_row(now, k, k + n, cap)
                rows.add(tuple(now))
            moves += len(trace)
            assert status == 0 and info[0] == len(trace) == info[2] + info[3] and info[1] == info[0] + 1 and info[4] <= info[0]
            assert value == (max(lens), sum(lens), *fb.key_of(w, o, k, mode)) and (value[0], value[1]) <= (value[2], value[3])
            assert fb.improving_candidates(d, route, k, mode, cap) == [], (k, n, mode, cap)
            optima += 1
    assert moves > 100 and optima > 30


def test_every_result_is_a_valid_row_with_its_own_sums():
    for kind, k, n, mode, cap, d in cases(kinds=("euclid", "tenths")):
        for o in starts_of(k, n, cap):
            N = k + n
            route, lens, value, status, info = fb.balance_numpy(d, o, k, mode, cap, 16 * N)
            w = fl.mirror(d)
            assert status in (0, 2) and fl.valid_row(route, k, N, cap) and (status == 2) == (info[0] == 16 * N)
            assert [tc.bits(x) for x in lens] == [tc.bits(x) for x in fl.lengths(w, route, k, mode)[0]]
            assert value == (*fb.key_of(w, route, k, mode), *fb.key_of(w, o, k, mode)) and value[0] <= value[2] + 1e-9
            # (no claim of a local optimum here: two spans that tie as real numbers need not tie as rounded sums, so a status-0 row of
            # these kinds may have a neighbour with the same makespan to a rounding and a smaller total; the integers are exact)


def test_never_below_brute_force():
    hits = runs = 0
    for kind in ("euclid", "ints", "tenths"):
        for (k, n), mode, seed in itertools.product(((1, 4), (2, 3), (2, 5), (3, 4), (3, 6), (2, 6)), fl.MODES, range(2)):
            d = fl.matrix(kind, k + n, seed)
            for cap in (None, ceil_caps(k, n, 1)):
                low = fb.brute_force(d, k, mode, cap)
                got = fb.balance_numpy(d, fl.random_row(k, n, seed, cap), k, mode, cap, 16 * (k + n))
                assert got[2][0] >= low > 0, (kind, k, n, mode, seed, cap)
                hits += got[2][0] == low
                runs += 1
    assert hits > runs // 3                                           # (and many reach it)
    assert fb.brute_force(fl.matrix("ints", 6, 0), 2, 1) <= fl.brute_force(fl.matrix("ints", 6, 0), 2, 1)


def test_one_robot_is_the_sum_rule():
    count = 0
    for kind, n, mode, seed in itertools.product(("euclid", "ints", "tenths"), (1, 2, 5, 9, 14), fl.MODES, range(3)):
        d, o = fl.matrix(kind, 1 + n, seed), fl.random_row(1, n, seed)
        summed = fl.improve_numpy(d, o, 1, mode, None, 16 * (1 + n))
        if summed[3] != 0:
            continue
        got = fb.balance_numpy(d, o, 1, mode, None, 16 * (1 + n))
        assert got[0] == summed[0] and got[3] == 0 and got[4][:4] == summed[4] and (got[4][4] == got[4][0] if kind == "ints" else got[4][4] <= got[4][0])
        assert [tc.bits(x) for x in got[2]] == [tc.bits(x) for x in (summed[2][0], summed[2][0], summed[2][1], summed[2][1])]
        again = fb.balance_numpy(d, summed[0], 1, mode, None, 16 * (1 + n))
        assert again[4] == (0, 1, 0, 0, 0) and again[0] == summed[0]
        count += 1
    assert count > 60


def test_the_capped_runs_of_the_seeded_set():
    assert fb.capped_runs("incremental") == fb.CAPPED_INCREMENTAL and fb.CAPPED_INCREMENTAL["ints"] == 0
    assert fb.capped_runs("recomputed") == fb.CAPPED_RECOMPUTED and fb.CAPPED_RECOMPUTED["ints"] == 0


def test_the_cap_on_the_moves_and_the_caps_on_the_tasks():
    d = fl.matrix("euclid", 14, 5)
    for mode in fl.MODES:
        o = fl.random_row(3, 11, 5)
        full = fb.balance_numpy(d, o, 3, mode, None, 16 * 14)
        moves = full[4][0]
        assert full[3] == 0 and moves >= 4
        for limit in (0, 1, moves - 1, moves):
            r = fb.balance_numpy(d, o, 3, mode, None, limit)
            assert words(r) == words(fb.balance(d, o, 3, mode, None, limit))
            assert r[3] == (0 if limit == moves else 2) and r[4][:2] == (limit, limit + 1)
            assert limit or (r[0] == o and r[2][:2] == r[2][2:])
        held = fl.structure(o, 3)[1]
        tight = fb.balance_numpy(d, o, 3, mode, held, 16 * 14)        # caps equal to the start's counts: no task changes hands
        assert [sorted(t) for t in fl.split(tight[0], 3)] == [sorted(t) for t in fl.split(o, 3)] and tight[2][0] >= full[2][0]


def test_garbage_in_the_unread_entries_and_an_infinite_entry():
    for kind, k, n, mode, cap, d in cases(shapes=((2, 5), (3, 6)), kinds=("euclid", "ints")):
        N = k + n
        junk = d.copy()
        junk[np.tril_indices(N)] = np.resize([np.nan, -1.0, -fl.INF, 2.0 ** 1010, fl.INF], N * (N + 1) // 2)
        junk[:k, :k] = np.resize([fl.INF, np.nan, -3.0], (k, k))
        o = fl.random_row(k, n, 3, cap)
        want = words(fb.balance(d, o, k, mode, cap, 16 * N))
        assert words(fb.balance(junk, o, k, mode, cap, 16 * N)) == want and words(fb.balance_numpy(junk, o, k, mode, cap, 16 * N)) == want
    d = fl.matrix("euclid", 7, 1)
    d[1, 4] = fl.INF
    r = fb.balance(d, fl.random_row(2, 5, 1), 2, 1, None, 50)
    assert words(r) == words(fb.balance_numpy(d, fl.random_row(2, 5, 1), 2, 1, None, 50)) == words(([-1] * 7, [fl.INF] * 2, (fl.INF,) * 4, 1, (0,) * 5))
    got = fb.search(d, 2, 1)
    assert not got["feasible"] and got["history"] == got["total_history"] == [fl.INF] and got["routes"] == [[], []] and got["moves"] == 0


def wrong_case(case, flag):
    kind, k, n, mode, seed = case
    d, o = fl.matrix(kind, k + n, seed), fl.random_row(k, n, seed)
    right = fb.balance(d, o, k, mode, None, 16 * (k + n))
    assert right[3] == 0 and words(right) == words(fb.balance_numpy(d, o, k, mode, None, 16 * (k + n)))
    return right, fb.balance(d, o, k, mode, None, 16 * (k + n), **{flag: True})


def test_the_wrong_solvers_are_told_from_the_rule():
    for case, flag in ((fb.WRONG_DELTA_FIRST, "delta_first"), (fb.WRONG_ACCEPT_EQUAL, "accept_equal"), (fb.WRONG_OLD_MAX, "old_max"),
                       (fb.WRONG_LARGEST_ON_TIE, "largest_on_tie"), (fb.WRONG_ADD_AS_DELTA, "add_as_delta")):
        right, wrong = wrong_case(case, flag)
        assert right[0] != wrong[0] and right[2][:2] != wrong[2][:2], flag
    right, wrong = wrong_case(fb.WRONG_DELTA_FIRST, "delta_first")
    assert right[2][0] < wrong[2][0]                                  # the sum's best move first: the span is never lowered
    right, wrong = wrong_case(fb.WRONG_ACCEPT_EQUAL, "accept_equal")
    assert wrong[3] == 2 and wrong[4][0] == 16 * 4                    # equal spans accepted with any delta: a walk in a circle
    kind, k, n, mode, seed = fb.WRONG_NO_INNER                        # the segment's inner legs left behind: a move that lowers nothing
    d, trace = fl.matrix(kind, k + n, seed), []
    wrong = fb.balance(d, fl.random_row(k, n, seed), k, mode, None, 16 * (k + n), no_inner=True, trace=trace)
    keys = [(fb.key_of(fl.mirror(d), was, k, mode), fb.key_of(fl.mirror(d), now, k, mode)) for *_, was, now in trace]
    assert any(not b < a for a, b in keys) and words(wrong) != words(fb.balance(d, fl.random_row(k, n, seed), k, mode, None, 16 * (k + n)))


def test_the_map_facts():
    g, m = map_matrix()
    for mode in fl.MODES:
        summed = fl.search(m, 3, mode, **fl.MAP_SEARCH)
        assert (summed["makespan"], summed["total"]) == fb.MAP_SUM[mode]
        for improver, solver in ((fl.improve_numpy, fb.balance_numpy), (fl.improve, fb.balance)):
            got = fb.search(m, 3, mode, improver=improver, solver=solver, **fl.MAP_SEARCH)
            assert (got["makespan"], got["total"]) == fb.MAP_BALANCED[mode] and got["routes"] == fb.MAP_BALANCED_ROUTES[mode]
            assert got["feasible"] and len(got["history"]) == len(got["total_history"]) == 4 and got["makespan"] == max(got["lengths"])
            assert got["history"] == sorted(got["history"], reverse=True) and got["start_total"] == summed["start_total"]
        assert fb.MAP_BALANCED[mode][0] < fb.MAP_SUM[mode][0] and fb.MAP_BALANCED[mode][1] > fb.MAP_SUM[mode][1]
    assert fb.MAP_SUM[1][0] == fb.MAP_SUM[1][1]                       # end="return" under the sum: one robot does everything
