"""The placement checkers pinned (any host): the rule's literal loop against the numpy form word for word, every applied move and
every stop looked at independently, brute force over all p-subsets, the cap, `fixed`, the two-room matrix, six wrong solvers
rejected, and the map fact tests/test_gpu_place.py leans on."""
import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import place_checkers as pc
from tour_checkers import bits


def words(got):
    row, owner, value, status, info = got
    return [int(v) for v in row], [int(v) for v in owner], tuple(bits(float(x)) for x in value), int(status), tuple(int(v) for v in info)


SMALL = [(kind, m, n, p, seed) for kind in pc.KINDS for (m, n, p) in ((1, 1, 1), (2, 3, 2), (5, 7, 2), (6, 8, 3), (9, 12, 4), (7, 5, 1)) for seed in range(3)]


@pytest.mark.parametrize("mode", pc.MODES)
def test_literal_against_numpy_on_small_matrices(mode):
    for kind, m, n, p, seed in SMALL:
        a = pc.matrix(kind, m, n, seed)
        for start in ([-1] * p, list(np.random.default_rng(seed).permutation(m)[:p])):
            assert words(pc.improve(a, start, mode, 0, 16 * p)) == words(pc.improve_numpy(a, start, mode, 0, 16 * p)), (kind, m, n, p, seed)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_literal_against_numpy_at_40_by_70(kind, mode):
    a = pc.matrix(kind, 40, 70, 5)
    full = list(np.random.default_rng(1).permutation(40)[:8])
    half = full[:4] + [-1] * 4
    for start, fixed, limit in ((half, 2, 3), (full, 0, 2), ([-1] * 8, 0, 2)):
        assert words(pc.improve(a, start, mode, fixed, limit)) == words(pc.improve_numpy(a, start, mode, fixed, limit))


@pytest.mark.parametrize("mode", pc.MODES)
def test_every_move_lowers_the_key_and_every_stop_is_a_local_optimum(mode):
    swapped = 0
    for kind, m, n, p, seed in SMALL:
        a = pc.matrix(kind, m, n, seed)
        trace = []
        row, owner, value, status, info = pc.improve(a, [-1] * p, mode, 0, 16 * p, trace=trace)
        assert status == 0 and info[0] == len(trace) and info[1] == info[0] + 1
        for before, o, i, key in trace:
            after = list(before)
            after[o] = i
            assert key == pc.key_of(pc.cost(a, after), mode) and key < pc.key_of(pc.cost(a, before), mode)
            swapped += before[o] >= 0
        assert pc.better_candidates(a, row, mode, 0) == [] and pc.valid_row(row, m, p, 0)
        last = pc.cost(a, row)
        assert (last[1], last[2], last[0]) == (value[0], value[1], info[2]) and owner == pc.owners(a, row)
        assert pc.key_of(last, mode) >= pc.brute_force(a, p, mode)
        if p == 1:
            assert pc.key_of(last, mode) == pc.brute_force(a, 1, mode)
    assert swapped > 0                                               # swaps follow the additions somewhere


@pytest.mark.parametrize("mode", pc.MODES)
def test_the_cap(mode):
    a = pc.matrix("euclid", 9, 12, 1)
    full = pc.improve(a, [-1] * 4, mode, 0, 64)
    moves = full[4][0]
    assert full[3] == 0 and moves >= 4
    for limit, status in ((0, 2), (moves - 1, 2), (moves, 0), (moves + 1, 0)):
        got = pc.improve(a, [-1] * 4, mode, 0, limit)
        assert got[3] == status and got[4][:2] == (min(limit, moves), min(limit, moves) + 1)
        assert (got[3] == 2) == (pc.better_candidates(a, got[0], mode, 0) != [])
        assert words(got) == words(pc.improve_numpy(a, [-1] * 4, mode, 0, limit))
    assert pc.improve(a, [-1] * 4, mode, 0, 0)[0] == [-1] * 4


@pytest.mark.parametrize("mode", pc.MODES)
def test_fixed_slots_a_full_row_and_m_equal_p(mode):
    a = pc.matrix("euclid", 9, 12, 2)
    for fixed in (0, 1, 4):
        start = [8, 3, 5, 0]
        got = pc.improve(a, start, mode, fixed, 64)
        assert got[0][:fixed] == start[:fixed] and got[3] == 0 and pc.better_candidates(a, got[0], mode, fixed) == []
        assert words(got) == words(pc.improve_numpy(a, start, mode, fixed, 64))
        if fixed == 4:
            assert got[0] == start and got[4][:2] == (0, 1) and bits(got[2][0]) == bits(got[2][2])
    b = pc.matrix("tenths", 4, 6, 2)
    got = pc.improve(b, [2, 0, 3, 1], mode, 0, 64)                    # every site is in the row: no candidate at all
    assert got[0] == [2, 0, 3, 1] and got[3] == 0 and got[4][:2] == (0, 1)
    got = pc.improve(b, [-1] * 4, mode, 0, 64)
    assert words(got) == words(pc.improve_numpy(b, [-1] * 4, mode, 0, 64)) and got[3] == 0


@pytest.mark.parametrize("mode", pc.MODES)
def test_the_two_rooms_and_a_demand_no_site_reaches(mode):
    a = pc.two_rooms()
    got = pc.improve(a, [-1, -1], mode, 0, 32)
    assert got[3] == 0 and got[4][2:] == (0, 6) and min(got[0]) < 2 <= max(got[0])
    assert words(got) == words(pc.improve_numpy(a, [-1, -1], mode, 0, 32))
    one = pc.improve(a, [-1], mode, 0, 32)
    assert one[3] == 0 and one[4][2] == 3 and one[1].count(-1) == 3
    a[:, 4] = pc.INF                                                 # nobody reaches demand 4
    got = pc.improve(a, [-1, -1], mode, 0, 32)
    assert got[3] == 0 and got[4][2] == 1 and got[1][4] == -1 and words(got) == words(pc.improve_numpy(a, [-1, -1], mode, 0, 32))
    dark = np.full((3, 4), pc.INF)
    got = pc.improve(dark, [-1, -1], mode, 0, 32)                     # no addition changes the key: the slots stay empty
    assert got[0] == [-1, -1] and got[4] == (0, 1, 4, 4) and got[2] == (0.0, 0.0, 0.0, 0.0) and got[1] == [-1] * 4


@pytest.mark.parametrize("wrong", pc.WRONG)
def test_wrong_solvers_are_rejected(wrong):
    kind, m, n, p, seed, mode = pc.WRONG_CASES[wrong]
    a = pc.matrix(kind, m, n, seed)
    want = pc.improve(a, [-1] * p, mode, 0, 16 * p)
    assert words(want) == words(pc.improve_numpy(a, [-1] * p, mode, 0, 16 * p))
    assert words(pc.improve(a, [-1] * p, mode, 0, 16 * p, wrong=wrong)) != words(want)


def test_a_key_without_the_unserved_count_leaves_a_room_empty():
    got = pc.improve(pc.two_rooms(), [-1, -1], 0, 0, 32, wrong="no_unserved_count")
    assert got[4][2] > 0


def test_validators():
    a = np.array([pc.matrix("euclid", 3, 4, b) for b in range(3)])
    assert pc.first_bad_entry(a) is None
    for x in (np.nan, -1.0, -0.0, 2.0 ** 1010, -pc.INF):
        bad = a.copy()
        bad[2, 0, 1], bad[1, 2, 3] = x, x
        assert pc.first_bad_entry(bad) == (1, 2, 3)
    a[0, 0, 0], a[0, 0, 1], a[0, 0, 2] = 0.0, pc.BIG, pc.INF
    assert pc.first_bad_entry(a) is None
    assert pc.first_bad_row([[0, -1, 2], [1, 2, -1]], 3, 3, 1) is None
    assert pc.first_bad_row([[0, -1, 2], [1, 2, 1]], 3, 3, 1) == (1, 2)
    assert pc.first_bad_row([[0, -1, 2], [1, 2, 3]], 3, 3, 1) == (1, 2)
    assert pc.first_bad_row([[0, -2, 2], [1, 2, 3]], 3, 3, 1) == (0, 1)
    assert pc.first_bad_row([[0, -1, 2], [-1, 2, 0]], 3, 3, 1) == (1, 0)
    assert pc.first_bad_row([[0, -1, 2]], 3, 3, 2) == (0, 1)


def test_the_rounds():
    a = pc.matrix("euclid", 9, 12, 4)
    for mode in pc.MODES:
        got = pc.search(a, 4, mode, keep=(5,), starts=3, rounds=3, seed=2, solver=pc.improve)
        assert got == pc.search(a, 4, mode, keep=(5,), starts=3, rounds=3, seed=2)
        assert got["row"][0] == 5 and len(got["history"]) == 4 and all(x >= y for x, y in zip(got["history"], got["history"][1:]))
        assert got["history"][-1] == pc.key_of((got["unserved"], got["total"], got["radius"]), mode) >= pc.brute_force(a, 4, mode, keep=(5,))
    rng = np.random.default_rng(7)
    draws = np.random.default_rng(7).integers(0, [3, 9], (5, 1, 2))
    rows = pc.perturbations(rng, [5, 1, 2, -1], 1, 9, 5)
    for s in range(5):
        slot, site = (int(v) for v in draws[s, 0])
        want = [5, 1, 2, -1]
        if site not in want:                                         # a site already in the row: the draw is dropped
            want[1 + slot] = site
        assert rows[s] == want and pc.valid_row(rows[s], 9, 4, 1)
    assert len(pc.search(a, 2, 0, keep=(1, 2), rounds=3)["history"]) == 1      # every slot kept: no later rounds


def map_matrix():
    g = gio.grid(pc.MAP_NAME)[0]
    cells = pc.map_cells(g)
    ids = [r * g.shape[1] + c for r, c in cells]
    mm = fc.move_masks(np.asarray(g, np.uint8), True, True)
    fields = np.array([fc.reference_dijkstra(np.asarray(g, np.uint8), mm, s)[0] for s in ids]).reshape(len(ids), -1)
    return np.ascontiguousarray(fields[:, ids])


def test_the_map_fact_swaps_follow_the_additions():
    a = map_matrix()
    assert a.shape == (290, 290)
    for mode in pc.MODES:
        row, owner, value, status, info = pc.improve_numpy(a, [-1] * pc.MAP_COUNT, mode, 0, 16 * pc.MAP_COUNT)
        assert status == 0 and info[2] == 0 and min(row) >= 0 and info[0] > pc.MAP_COUNT        # the moves exceed the additions
