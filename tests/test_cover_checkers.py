"""The coverage checkers pinned on any host (tests/cover_checkers.py): the rule's literal loop form over Python sets
against the numpy form on packed words, word for word; every applied move's key; every status-0 row; brute force; the cap; the
fixed slots; and the seven WRONG solvers each told from the rule on a seeded case kept in the checkers.  It also derives the map
fact tests/test_gpu_cover.py leans on."""
import numpy as np
import pytest

import cover_checkers as cc
import golden_io as gio

SHAPES = [(1, 1, 1), (2, 1, 1), (3, 2, 3), (5, 7, 2), (9, 64, 3), (12, 65, 4), (20, 130, 5), (40, 200, 8)]


def both(b, n, start, fixed, limit, trace=None):
    lit = cc.improve(cc.sets_of(b), n, start, fixed, limit, trace=trace)
    num = cc.improve_numpy(cc.pack(b), n, start, fixed, limit)
    assert cc.same(lit, num), (b.shape, start, fixed, limit, lit, num)
    return lit


def starts_of(m, p, seed):
    return [[-1] * p, cc.full_row(m, p, seed), cc.half_row(m, p, seed)]


@pytest.mark.parametrize("density", cc.DENSITIES)
def test_the_literal_form_equals_the_numpy_form_word_for_word(density):
    for m, n, p in SHAPES:
        for seed in range(2 if m > 12 else 4):
            b = cc.bits(density, m, n, seed)
            S = cc.sets_of(b)
            for start in starts_of(m, p, seed):
                trace = []
                row, covered, value, status, info = both(b, n, start, 0, 16 * p, trace)
                assert status == 0 and cc.valid_row(row, m, p, 0) and info[0] == len(trace) and info[1] == info[0] + 1
                # every applied move's key is the recomputed key of the new row and lies strictly below the one before
                for before, o, i, k in trace:
                    after = list(before)
                    after[o] = i if i < m else -1
                    assert k == cc.key(S, n, after) and k < cc.key(S, n, before)
                assert info[3] == sum(1 for t in trace if t[2] == m)
                # a status-0 row has no better candidate, looked at independently
                assert cc.better_candidates(S, n, row, 0) == []
                assert (n - value[0], value[1]) == cc.key(S, n, row) and (n - value[2], value[3]) == cc.key(S, n, start)
                assert np.array_equal(cc.unpack(covered, n), cc.unpack(cc.pack(b), n)[[s for s in row if s >= 0]].any(0) if value[1] else np.zeros(n, bool))
                assert info[2] == int((b[[s for s in row if s >= 0]].sum(0) == 1).sum())


def test_pack_unpack_and_popcount():
    b = cc.bits(0.5, 7, 131, 1)
    M = cc.pack(b)
    assert M.shape == (7, 3) and M.dtype == np.uint64 and np.array_equal(cc.unpack(M, 131), b) and cc.first_bad_tail(M, 131) is None
    assert [int(v) for v in cc.popcount(M).sum(1)] == [int(v) for v in b.sum(1)]
    assert [int(v) for v in M[2]] == cc.words_of_set(cc.sets_of(b)[2], 131)
    assert int(cc.popcount(np.array([0, 1, 2 ** 64 - 1, 2 ** 63], np.uint64)).sum()) == 66


@pytest.mark.parametrize("density", cc.DENSITIES)
def test_keys_against_brute_force(density):
    for m, n, p in [(4, 9, 1), (6, 20, 2), (8, 30, 3), (10, 40, 4), (10, 70, 1)]:
        for seed in range(3):
            b = cc.bits(density, m, n, seed)
            S = cc.sets_of(b)
            for keep in ((), (m - 1,)):
                want = cc.brute_force(S, n, p, keep)
                got = both(b, n, list(keep) + [-1] * (p - len(keep)), len(keep), 16 * p)
                assert cc.key_of_result(got, n) >= want
                if p == 1 and not keep:
                    assert cc.key_of_result(got, n) == want


def test_the_cap_on_the_moves():
    m, n, p = 20, 130, 5
    b = cc.bits(0.2, m, n, 3)
    S = cc.sets_of(b)
    full = both(b, n, [-1] * p, 0, 16 * p)
    moves = full[4][0]
    assert full[3] == 0 and moves >= p
    for limit in (0, 1, moves - 1, moves):
        row, covered, value, status, info = both(b, n, [-1] * p, 0, limit)
        # status 2 exactly when a better candidate exists at moves == max_moves
        assert info[0] == limit and (status == 2) == bool(cc.better_candidates(S, n, row, 0)) and status == (0 if limit == moves else 2)
        assert info[1] == limit + 1 and (limit or row == [-1] * p)
    assert both(b, n, full[0], 0, 0)[3] == 0                         # a local optimum under a cap of 0


def test_fixed_slots_and_m_equal_p():
    m, n, p = 12, 100, 4
    b = cc.bits(0.2, m, n, 5)
    for fixed in (0, 1, p):
        for seed in range(3):
            start = cc.full_row(m, p, seed)
            row, covered, value, status, info = both(b, n, start, fixed, 16 * p)
            assert row[:fixed] == start[:fixed] and status == 0
            if fixed == p:
                assert row == start and info[:2] == (0, 1) and info[3] == 0 and value[:2] == value[2:]
        both(b, n, cc.full_row(m, p, 3)[:max(fixed, 1)] + [-1] * (p - max(fixed, 1)), fixed, 16 * p)
    b = cc.bits(0.2, 5, 40, 2)
    for start in ([-1] * 5, [4, 3, 2, 1, 0], [2, -1, -1, 0, -1]):
        row, covered, value, status, info = both(b, 40, start, 0, 80)
        assert status == 0
    row, covered, value, status, info = both(np.eye(5, 40, dtype=bool), 40, [4, 3, 2, 1, 0], 0, 80)
    assert row == [4, 3, 2, 1, 0] and info[:2] == (0, 1)              # every site is in the row and none is redundant: only drops, none better


def test_all_zero_masks_leave_the_slots_empty():
    b = np.zeros((6, 70), bool)
    row, covered, value, status, info = both(b, 70, [-1] * 3, 0, 48)
    assert row == [-1] * 3 and value == (0, 0, 0, 0) and info == (0, 1, 0, 0) and status == 0 and not covered.any()
    row, covered, value, status, info = both(b, 70, [2, -1, 4], 0, 48)   # two sites that cover nothing: both are dropped
    assert row == [-1] * 3 and info == (2, 3, 0, 2) and value == (0, 0, 0, 2)
    row, covered, value, status, info = both(b, 70, [2, -1, 4], 1, 48)   # the kept one stays
    assert row == [2, -1, -1] and info[3] == 1


def test_duplicate_masks():
    b = cc.bits(0.2, 4, 90, 7)
    b = np.concatenate([b, b, b[:2]])                                 # every mask two or three times
    for start in ([-1] * 4, [0, 4, 8, 1], [5, 1, -1, 9]):
        row, covered, value, status, info = both(b, 90, start, 0, 64)
        sites = [s for s in row if s >= 0]
        assert status == 0 and len({s % 4 for s in sites}) == len(sites)   # no two copies of one mask stay: the second is redundant
    two = np.concatenate([b[:2], b[:2], b[:2]])                       # two masks three times each, four slots: two copies must go
    row, covered, value, status, info = both(two, 90, [0, 2, 4, 1], 0, 64)
    assert info[3] == 2 and value[1] == 2 and value[0] == value[2]


@pytest.mark.parametrize("name", cc.WRONG)
def test_each_wrong_solver_is_rejected(name):
    S, n, start = cc.wrong_case(name)
    p = len(start)
    right = cc.improve(S, n, start, 0, 16 * p)
    wrong = cc.improve(S, n, start, 0, 16 * p, wrong=name)
    assert not cc.same(right, wrong), name
    if name == "counts_tail_bits":
        width = cc.words_of(n) * 64
        raw = cc.pack(np.array([[j in s for j in range(width)] for s in S]))
        assert cc.first_bad_tail(raw, n) is not None                  # the validator names such a mask; the rule never sees it
        clean = cc.pack(np.array([[j in s for j in range(n)] for s in S]))
        assert cc.first_bad_tail(clean, n) is None and cc.same(right, cc.improve_numpy(clean, n, start, 0, 16 * p))
    else:
        M = cc.pack(np.array([[j in s for j in range(n)] for s in S]))
        assert cc.same(right, cc.improve_numpy(M, n, start, 0, 16 * p))
    if name == "no_drops":
        assert right[4][3] >= 1 and wrong[4][3] == 0 and -1 not in start   # a full start row with a redundant site


def test_the_validators():
    M = cc.pack(cc.bits(0.5, 5, 70, 1))[None].repeat(3, 0)
    assert cc.first_bad_tail(M, 70) is None and cc.first_bad_tail(M, 128) is None
    M[2, 1, 1] |= np.uint64(1) << np.uint64(6)
    M[1, 3, 1] |= np.uint64(1) << np.uint64(63)
    assert cc.first_bad_tail(M, 70) == (1, 3) and cc.first_bad_tail(M[2:], 70) == (0, 1) and cc.first_bad_tail(M, 71) == (1, 3)
    assert cc.first_bad_row([[0, -1, 3], [4, 2, 4]], 5, 3, 1) == (1, 2) and cc.first_bad_row([[0, -1, 3]], 5, 3, 2) == (0, 1)


def test_the_rounds_keep_the_first_smallest_key():
    b = cc.bits(0.2, 30, 150, 4)
    M = cc.pack(b)
    got = cc.search(M, 150, 5, keep=(3,), starts=5, rounds=3, seed=2)
    assert got["row"][0] == 3 and len(got["history"]) == 4 and got["history"] == sorted(got["history"], reverse=True)
    assert got["count"] == int(cc.unpack(got["covered"], 150).sum()) == 150 - got["history"][-1][0]
    assert cc.search(M, 150, 5, keep=(3,), starts=5, rounds=3, seed=2)["row"] == got["row"]
    assert len(cc.search(M, 150, 2, keep=(3, 4), rounds=3)["history"]) == 1      # every slot kept: no later rounds


def test_the_map_fact():
    """Every free cell of the golden 20 x 20 map (290) a site and a target, the strict rule, no range limit: three additions alone
    see 199 cells, the rule's four moves 206; with 24 slots additions alone need 13 sites to see all 290, the rule 12."""
    g = gio.grid(cc.MAP_NAME)[0]
    cells = cc.map_cells(g)
    assert len(cells) == cc.MAP_FREE
    M = cc.pack(cc.sight_bits(g, cells, cells))
    n = len(cells)
    greedy, rule = cc.improve_numpy(M, n, [-1] * 3, 0, 48, additions_only=True), cc.improve_numpy(M, n, [-1] * 3, 0, 48)
    assert (greedy[2][0], rule[2][0], rule[4][0]) == (cc.MAP_THREE["additions"], cc.MAP_THREE["rule"], cc.MAP_THREE["moves"])
    assert rule[2][0] > greedy[2][0] and greedy[4][0] == 3 and rule[3] == 0
    p = cc.MAP_ALL["slots"]
    greedy, rule = cc.improve_numpy(M, n, [-1] * p, 0, 16 * p, additions_only=True), cc.improve_numpy(M, n, [-1] * p, 0, 16 * p)
    assert greedy[2][:2] == (n, cc.MAP_ALL["additions"]) and rule[2][:2] == (n, cc.MAP_ALL["rule"]) and rule[2][1] < greedy[2][1]
    # the literal form agrees on the three-slot case
    assert cc.same(cc.improve(cc.sets_of(cc.unpack(M, n)), n, [-1] * 3, 0, 48), cc.improve_numpy(M, n, [-1] * 3, 0, 48))
