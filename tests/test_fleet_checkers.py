"""The fleet checkers pinned on a CPU-only host: the literal loop against the numpy form word for word, what every result must
satisfy, every move's delta against the recomputed totals, brute force below it, the unread entries, the caps, the six wrong
solvers told from the rule, and the map fact the GPU file and the README lean on."""
import itertools

import numpy as np

import field_checkers as fc
import fleet_checkers as fl
import golden_io as gio
import tour_checkers as tc

KINDS = ("euclid", "ints", "tenths", "holes")
SHAPES = ((1, 1), (1, 2), (2, 1), (1, 5), (2, 2), (2, 5), (3, 1), (3, 6), (4, 9), (5, 3), (5, 12), (3, 22), (5, 35))


def words(r):
    route, lens, value, status, info = r
    return [int(v) for v in route], tuple(tc.bits(x) for x in lens), tuple(tc.bits(x) for x in value), int(status), tuple(int(v) for v in info)


def ceil_caps(k, n, slack=0):
    return [-(-n // k) + slack] * k


def starts_of(k, n, cap, seed=3):
    """A seeded start (routes may be empty), all tasks on the last robot with room for them (the others empty), the greedy start."""
    rows = [fl.random_row(k, n, seed, cap)]
    if cap is None:
        rows.append(fl.row_of([[] for _ in range(k - 1)] + [list(range(k, k + n))]))
    return rows


def cases(shapes=SHAPES, kinds=KINDS):
    for kind, (k, n), mode in itertools.product(kinds, shapes, fl.MODES):
        for cap in (None, ceil_caps(k, n, 1)):
            yield kind, k, n, mode, cap, fl.matrix(kind, k + n, 3)


def test_the_literal_form_and_the_numpy_form_agree_word_for_word():
    seen, two, relocations = set(), 0, 0
    for kind, k, n, mode, cap, d in cases():
        for o in starts_of(k, n, cap):
            if k + n > 20 and (kind != "euclid" or cap is not None or mode == 1):
                continue                                              # (the literal loop is slow: the large shapes once per kind)
            a = fl.improve(d, o, k, mode, cap, 16 * (k + n))
            assert words(a) == words(fl.improve_numpy(d, o, k, mode, cap, 16 * (k + n))), (kind, k, n, mode, cap)
            seen.add(a[3])
            two, relocations = two + a[4][2], relocations + a[4][3]
    assert two > 50 and relocations > 50 and {0, 1} <= seen                                             # (2 too: a search may walk in a circle until the cap)


def test_every_move_changes_the_total_by_its_delta():
    count = 0
    for kind, k, n, mode, cap, d in cases(kinds=("euclid", "ints", "tenths")):
        if k + n > 20:
            continue
        for o in starts_of(k, n, cap):
            trace = []
            fl.improve(d, o, k, mode, cap, 16 * (k + n), trace=trace)
            for delta, code, i, j, was, now in trace:
                assert delta < 0 and abs((now - was) - delta) <= 1e-9, (kind, k, n, mode, cap, code, i, j)
            count += len(trace)
    assert count > 200


def test_every_result_is_a_valid_row_within_its_caps_with_its_own_sums():
    for kind, k, n, mode, cap, d in cases(kinds=("euclid", "ints", "tenths")):
        for o in starts_of(k, n, cap):
            N = k + n
            route, lens, value, status, info = fl.improve_numpy(d, o, k, mode, cap, 16 * N)
            assert status in (0, 2) and fl.valid_row(route, k, N, cap), (kind, k, n, mode, cap)
            w = fl.mirror(d)
            want = []
            for r, tasks in enumerate(fl.split(route, k)):            # the left-to-right sums, written out once more
                t, at = 0.0, r
                for x, v in enumerate(tasks):
                    t = w[at][v] if x == 0 else t + w[at][v]
                    at = v
                if tasks and mode == 1:
                    t = t + w[at][r]
                want.append(float(t))
            assert [tc.bits(x) for x in want] == [tc.bits(x) for x in lens]
            assert value[0] == sum_left(lens) and value[2] == max(lens) and value[1] == fl.lengths(w, o, k, mode)[1]
            assert info[0] == info[2] + info[3] and info[1] == info[0] + 1 and (status == 2) == (info[0] == 16 * N)
            if status == 0:
                assert fl.improving_candidates(d, route, k, mode, cap) == [], (kind, k, n, mode, cap)   # looked at independently


def sum_left(xs):
    t = xs[0]
    for x in xs[1:]:
        t = t + x
    return t


def test_never_below_brute_force():
    hits = runs = 0
    for kind in ("euclid", "ints", "tenths"):
        for (k, n), mode, seed in itertools.product(((1, 4), (2, 3), (2, 5), (3, 4), (3, 6), (2, 6)), fl.MODES, range(2)):
            d = fl.matrix(kind, k + n, seed)
            for cap in (None, ceil_caps(k, n, 1)):
                low = fl.brute_force(d, k, mode, cap)
                got = fl.improve_numpy(d, fl.random_row(k, n, seed, cap), k, mode, cap, 16 * (k + n))
                assert got[2][0] >= low > 0, (kind, k, n, mode, seed, cap)
                hits += got[2][0] == low
                runs += 1
    assert hits > runs // 2                                           # (and most reach it)


def test_garbage_in_the_unread_entries_is_ignored():
    for kind, k, n, mode, cap, d in cases(shapes=((2, 5), (3, 6), (5, 3)), kinds=("euclid", "ints", "tenths")):
        N = k + n
        junk = d.copy()
        junk[np.tril_indices(N)] = np.resize([np.nan, -1.0, -fl.INF, 2.0 ** 1010, fl.INF], N * (N + 1) // 2)
        junk[:k, :k] = np.resize([fl.INF, np.nan, -3.0], (k, k))
        assert fl.first_bad_entry(junk, k) is None
        o = fl.random_row(k, n, 3, cap)
        want = words(fl.improve(d, o, k, mode, cap, 16 * N))
        assert words(fl.improve(junk, o, k, mode, cap, 16 * N)) == want and words(fl.improve_numpy(junk, o, k, mode, cap, 16 * N)) == want


def test_the_cap_on_the_moves():
    d = fl.matrix("euclid", 14, 5)
    for mode in fl.MODES:
        o = fl.random_row(3, 11, 5)
        full = fl.improve_numpy(d, o, 3, mode, None, 16 * 14)
        moves = full[4][0]
        assert full[3] == 0 and moves >= 4
        for limit in (0, 1, moves - 1, moves):
            r = fl.improve_numpy(d, o, 3, mode, None, limit)
            assert words(r) == words(fl.improve(d, o, 3, mode, None, limit))
            assert r[3] == (0 if limit == moves else 2) and r[4][:2] == (limit, limit + 1)
            assert limit or (r[0] == o and r[2][0] == r[2][1])
        assert words(fl.improve_numpy(d, o, 3, mode, None, moves)) == words(full)
        again = fl.improve_numpy(d, full[0], 3, mode, None, 0)       # a local optimum needs no move
        assert again[3] == 0 and again[4] == (0, 1, 0, 0) and again[0] == full[0]


def test_capacities_bind():
    d = fl.matrix("euclid", 11, 2)
    k, n = 3, 8
    o = fl.random_row(k, n, 2, [3, 3, 3])
    held = fl.structure(o, k)[1]
    for mode in fl.MODES:
        free = fl.improve_numpy(d, o, k, mode, None, 16 * 11)
        tight = fl.improve_numpy(d, o, k, mode, held, 16 * 11)        # caps equal to the start's counts: no task changes hands
        assert fl.structure(tight[0], k)[1] == held and [sorted(t) for t in fl.split(tight[0], k)] == [sorted(t) for t in fl.split(o, k)]
        assert tight[2][0] >= free[2][0] and fl.valid_row(tight[0], k, 11, held)
        some = fl.improve_numpy(d, o, k, mode, [3, 3, 3], 16 * 11)
        assert fl.valid_row(some[0], k, 11, [3, 3, 3]) and fl.valid_row(free[0], k, 11)
    shut = fl.improve_numpy(d, fl.row_of([[3, 4, 5, 6, 7, 8, 9, 10], [], []]), k, 0, [8, 0, 0], 16 * 11)   # a cap of 0: nobody else may take one
    assert fl.structure(shut[0], k)[1] == [8, 0, 0]
    few = fl.row_of([[3, 4], [5], []])
    assert fl.first_over_cap([few, few], 3, 6, [2, 0, 1]) == (0, 1) and fl.first_over_cap([few], 3, 6, [1, 0, 0]) == (0, 0)
    assert fl.first_over_cap([few], 3, 6, [2, 1, 0]) is None and fl.first_over_cap([few], 3, 6, None) is None


def test_the_row_checks_name_the_first_position():
    k, N = 3, 7
    good = [0, 3, 4, 1, 5, 2, 6]
    assert fl.first_bad_row([good], k, N) is None and fl.valid_row(good, k, N)
    for row, at in (([0, 3, 4, 2, 5, 1, 6], 3), ([1, 3, 4, 0, 5, 2, 6], 0), ([0, 3, 3, 1, 5, 2, 6], 2), ([0, 3, 7, 1, 5, 2, 6], 2), ([0, 3, -1, 1, 5, 2, 6], 2),
                    ([3, 0, 4, 1, 5, 2, 6], 0), ([0, 3, 4, 1, 5, 1, 6], 5)):
        assert fl.first_bad_row([good, row], k, N) == (1, at), row
    bad = np.array([fl.matrix("uniform", N, b) for b in range(2)])
    bad[1, 0, 1], bad[1, 2, 1], bad[1, 4, 4], bad[1, 5, 3] = -1.0, np.nan, -1.0, np.nan        # robot-robot, the diagonal, below it: unread
    assert fl.first_bad_entry(bad, k) is None
    bad[1, 2, 3], bad[1, 1, 5] = 2.0 ** 1001, np.nan
    assert fl.first_bad_entry(bad, k) == (1, 1, 5)


def wrong_case(case, **flag):
    kind, k, n, mode, seed = case
    d = fl.matrix(kind, k + n, seed)
    cap = ceil_caps(k, n) if "ignore_caps" in flag else None
    o = fl.row_of([list(range(k, k + n))] + [[] for _ in range(k - 1)]) if "no_markers" in flag else fl.random_row(k, n, seed, cap)
    right = fl.improve(d, o, k, mode, cap, 16 * (k + n))
    assert words(right) == words(fl.improve_numpy(d, o, k, mode, cap, 16 * (k + n)))
    return right, fl.improve(d, o, k, mode, cap, 16 * (k + n), **flag), cap


def test_the_wrong_solvers_are_told_from_the_rule():
    for case, flag in ((fl.WRONG_LARGEST_ON_TIE, "largest_on_tie"), (fl.WRONG_RELOCATE_FIRST, "relocate_first"), (fl.WRONG_FIRST_IMPROVEMENT, "first_improvement"),
                       (fl.WRONG_OTHER_SUM, "other_sum")):
        right, wrong, _ = wrong_case(case, **{flag: True})
        assert words(right) != words(wrong) and right[0] != wrong[0], flag
    right, wrong, cap = wrong_case(fl.WRONG_IGNORE_CAPS, ignore_caps=True)
    k, n = fl.WRONG_IGNORE_CAPS[1:3]
    assert fl.valid_row(right[0], k, k + n, cap) and not fl.valid_row(wrong[0], k, k + n, cap)
    right, wrong, _ = wrong_case(fl.WRONG_NO_MARKERS, no_markers=True)
    k = fl.WRONG_NO_MARKERS[1]
    assert [] in fl.split(wrong[0], k) and [] not in fl.split(right[0], k) and right[2][0] < wrong[2][0]   # the empty route must be filled


def test_the_start_rule_and_the_perturbations():
    d = fl.matrix("euclid", 12, 4)
    w = fl.mirror(d)
    o = fl.start_row(w, 3, None)
    lists = fl.split(o, 3)
    assert fl.valid_row(o, 3, 12) and all(min(range(3), key=lambda r: (w[r][t], r)) == r for r, ts_ in enumerate(lists) for t in ts_)
    for r, tasks in enumerate(lists):
        at, left = r, list(tasks)
        for t in tasks:                                               # nearest neighbour, the smallest task on a tie
            assert t == min(left, key=lambda v: (w[at][v], v))
            left.remove(t)
            at = t
    capped = fl.start_row(w, 3, [3, 3, 3])
    assert fl.structure(capped, 3)[1] == [3, 3, 3] and capped != o
    ties = fl.start_row(np.ones((7, 7)), 2, [2, 9])
    assert ties == [0, 2, 3, 1, 4, 5, 6]
    rng = np.random.default_rng(5)
    got = fl.perturbations(rng, capped, 3, [3, 3, 3], 16) + fl.perturbations(rng, o, 3, [9, 9, 9], 16)
    assert all(fl.valid_row(p, 3, 12, [3, 3, 3]) for p in got[:16]) and all(fl.valid_row(p, 3, 12) for p in got[16:])
    assert any(p != o for p in got[16:]) and any(sorted(a) != sorted(b) for p in got[16:] for a, b in zip(fl.split(p, 3), lists))
    assert fl.perturbed(o, 3, None, [(0, 0, 5), (1, 11, 0), (0, 2, 1), (0, 2, 2)]) == o       # a marker, past the end, j = i - 1, j = i: dropped


def map_matrix():
    g = gio.grid(fl.MAP)[0]
    mm = fc.move_masks(np.asarray(g, np.uint8), True, True)
    ids = [r * g.shape[1] + c for r, c in fl.MAP_ROBOTS + fl.MAP_TASKS]
    fields = np.array([fc.reference_dijkstra(np.asarray(g, np.uint8), mm, s)[0] for s in ids]).reshape(len(ids), -1)
    return g, np.ascontiguousarray(fields[:, ids])


def test_the_map_fact():
    g, m = map_matrix()
    assert fl.MAP_ROBOTS + fl.MAP_TASKS == tc.free_cells(g, 15, 6) and np.isfinite(m).all()
    for solver in (fl.improve_numpy, fl.improve):
        got = fl.search(m, 3, 0, solver=solver, **fl.MAP_SEARCH)
        assert (got["start_total"], got["history"][0], got["total"]) == (fl.MAP_START_TOTAL, fl.MAP_ROUND0_TOTAL, fl.MAP_ROUNDS_TOTAL)
        assert got["routes"] == fl.MAP_ROUTES and got["feasible"] and len(got["history"]) == 4 and got["total"] == sum_left(got["lengths"])
    assert fl.MAP_START_TOTAL > fl.MAP_ROUND0_TOTAL > fl.MAP_ROUNDS_TOTAL > 0


def test_an_infinite_entry_is_not_searched():
    d = fl.matrix("euclid", 7, 1)
    d[1, 4] = fl.INF
    r = fl.improve(d, fl.random_row(2, 5, 1), 2, 1, None, 50)
    assert words(r) == words(fl.improve_numpy(d, fl.random_row(2, 5, 1), 2, 1, None, 50)) == words(([-1] * 7, [fl.INF] * 2, (fl.INF,) * 3, 1, (0, 0, 0, 0)))
    got = fl.search(d, 2, 1)
    assert not got["feasible"] and got["history"] == [fl.INF] and got["routes"] == [[], []] and got["moves"] == 0
    d[1, 4], d[0, 1], d[4, 1] = 1.0, fl.INF, fl.INF                   # a robot-robot entry and one below the diagonal: never read
    assert fl.improve_numpy(d, fl.random_row(2, 5, 1), 2, 1, None, 50)[3] == 0
