"""The widest-path model (tests/widest_checkers.py) pinned against the equivalent form of the rule: for every t >= 1, w[v] >= t iff v
and a source lie in one component, under the same policy, of the map whose obstacles are the cells with d2 < t
(clearance_checkers.inflated, component_checkers.flood_fill); and the definition of widest_path pinned against the field.  Runs on
any host."""
import os
import re

import numpy as np
import pytest

import clearance_checkers as ck
import component_checkers as cc
import field_checkers as fc
import widest_checkers as wc


def by_thresholds(grid, d2, sets, ad, rs):
    """w [B, R, C] from threshold-then-flood-fill: the largest t whose inflated map joins the cell to a usable source of the set."""
    R, C = d2.shape
    flat = d2.reshape(-1)
    out = np.zeros((len(sets), R * C), np.int32)
    for t in sorted(set(int(x) for x in flat if x >= 1)):
        lab = cc.flood_fill(ck.inflated(grid, d2, t), ad, rs)[0].reshape(-1)
        for b, s in enumerate(sets):
            ls = set(int(lab[v]) for v in s if lab[v] >= 0)
            if ls:
                out[b][np.isin(lab, list(ls))] = t                     # (thresholds in rising order: the largest one stays)
    return out.reshape(len(sets), R, C)


def every_single_source_by_thresholds(grid, d2, ad, rs, seen):
    """by_thresholds for the sets [[0]], [[1]], ... at once: row s holds the largest t whose inflated map joins the cell to s.  seen keeps
    the labels per (inflated map, policy): the inflated maps of the 3 x 4 grids are 3 x 4 grids again."""
    R, C = d2.shape
    out = np.zeros((R * C, R * C), np.int32)
    for t in sorted(set(int(x) for x in d2.reshape(-1) if x >= 1)):
        fat = ck.inflated(grid, d2, t)
        key = ((fat == 1).tobytes(), ad, rs)
        if key not in seen:
            seen[key] = cc.flood_fill(fat, ad, rs)[0].reshape(-1)
        lab = seen[key]
        out[(lab[:, None] == lab[None, :]) & (lab[:, None] >= 0)] = t
    return out.reshape(R * C, R, C)


@pytest.mark.parametrize("border", [False, True])
def test_every_3x4_grid_and_every_single_source(border):
    R, C = 3, 4
    sets = [[s] for s in range(R * C)]
    seen = {}
    for bits in range(1 << (R * C)):
        g = np.array([(bits >> i) & 1 for i in range(R * C)], np.uint8).reshape(R, C)
        d2 = ck.brute_force(g, border)[0]
        for ad, rs in wc.POLICIES:
            want = every_single_source_by_thresholds(g, d2, ad, rs, seen)
            got, info = wc.widest(d2, sets, ad, rs)
            assert np.array_equal(got, want), (bits, border, ad, rs)
            for s in range(R * C):
                assert info[s][0] == (d2.reshape(-1)[s] >= 1) and info[s][1] == (want[s] >= 1).sum(), (bits, border, ad, rs, s)


def test_a_map_without_obstacles():
    g = np.zeros((3, 4), np.uint8)
    d2 = ck.brute_force(g, False)[0]
    assert np.all(d2 == wc.NONE)
    w, info = wc.widest(d2, [[5]], 1, 1)
    assert np.all(w == wc.NONE) and list(info[0]) == [1, 12, wc.NONE, 0]
    d2 = ck.brute_force(g, True)[0]
    w, info = wc.widest(d2, [[5]], 1, 1)
    assert np.array_equal(w[0], np.minimum(d2, d2.reshape(-1)[5])) and np.array_equal(w, by_thresholds(g, d2, [[5]], 1, 1))


@pytest.mark.parametrize("seed", range(24))
def test_seeded_maps_up_to_12x13(seed):
    rnd = np.random.default_rng(900 + seed)
    R, C = int(rnd.integers(2, 13)), int(rnd.integers(2, 14))
    g = wc.seeded(R, C, float(rnd.choice([0.05, 0.15, 0.3])), 1000 + seed)
    sets = [list(rnd.integers(0, R * C, int(rnd.integers(1, 4)))) for _ in range(3)]
    sets.append([sets[0][0], sets[0][0]])                             # a source listed twice
    for border in (False, True):
        d2 = ck.brute_force(g, border)[0]
        for ad, rs in wc.POLICIES:
            got, info = wc.widest(d2, sets, ad, rs)
            want = by_thresholds(g, d2, sets, ad, rs)
            assert np.array_equal(got, want), (seed, border, ad, rs)
            for b, s in enumerate(sets):
                usable = len(set(int(v) for v in s if d2.reshape(-1)[v] >= 1))
                assert info[b][0] == usable and info[b][1] == (want[b] >= 1).sum()
                if info[b][1]:
                    low = want[b][want[b] >= 1].min()
                    assert info[b][2] == low and info[b][3] == np.flatnonzero(want[b].reshape(-1) == low)[0]
                else:
                    assert list(info[b][2:]) == [-1, -1]


def test_info_of_a_set_without_a_usable_source():
    g = np.zeros((4, 5), np.uint8)
    g[1, 1] = g[2, 3] = 1
    d2 = ck.brute_force(g)[0]
    w, info = wc.widest(d2, [[6], [6, 13]], 1, 1)
    assert not w.any() and list(info[0]) == [0, 0, -1, -1] and list(info[1]) == [0, 0, -1, -1]


@pytest.mark.parametrize("seed", range(12))
def test_widest_path_is_the_dijkstra_path_at_its_own_threshold(seed):
    """The traced path on inflated(w[target]) has smallest d2 equal to w[target]; at w[target] + 1 no path exists."""
    rnd = np.random.default_rng(40 + seed)
    R, C = int(rnd.integers(6, 13)), int(rnd.integers(6, 14))
    g = wc.seeded(R, C, 0.18, 70 + seed)
    d2 = ck.brute_force(g, bool(seed & 1))[0]
    flat = d2.reshape(-1)
    free = np.flatnonzero(flat >= 1)
    for ad, rs in wc.POLICIES:
        s = int(rnd.choice(free))
        w = wc.widest_one(d2, [s], ad, rs)[0]
        for t in [int(x) for x in rnd.choice(R * C, 6)] + [s]:
            path, wt = wc.widest_path(g, d2, s, t, ad, rs, w)
            assert wt == w.reshape(-1)[t]
            if wt == 0:
                assert path == []
                continue
            assert path[0] == s and path[-1] == t and min(int(flat[v]) for v in path) == wt
            if t == s:
                assert path == [s]
            # the field-only parent rule names the same tree
            gi = wc.inflated_with_markers(g, d2, wt, s, t)
            mm = fc.move_masks(gi, ad, rs)
            dist, code = fc.reference_dijkstra(gi, mm, s)
            assert np.array_equal(fc.rule_parents(dist, mm), code) and fc.trace(code, t) == path
            if wt < wc.NONE:
                gj = ck.inflated(g, d2, wt + 1)                         # (no markers: an end with d2 == wt is an obstacle now)
                assert fc.trace(fc.reference_dijkstra(gj, fc.move_masks(gj, ad, rs), s)[1], t) == []


def test_door_ladder_steps_down_room_by_room():
    g, centres = wc.door_ladder(5)
    d2 = ck.brute_force(g)[0]
    w = wc.widest_one(d2, [centres[-1]], 1, 1)[0].reshape(-1)
    # door k (1 .. 4, k cells wide) stands between room k - 1 and room k; the middle of a door k wide is ceil(k / 2) cells from its jambs
    assert [int(w[c]) for c in centres] == [((j + 2) // 2) ** 2 for j in range(4)] + [int(d2.reshape(-1)[centres[-1]])] == [1, 1, 4, 4, 25]


def test_the_entry_points_and_the_tile_the_gpu_tests_assume():
    """pf_clearance_widest and pf_clearance_widest_work are declared in the header and bound; the tile sizes tests/test_gpu_widest.py
    builds its maps about are the kernel's."""
    from pathfit import _lib
    import test_gpu_widest as tg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pathfit.h")).read()
    for name, nargs in (("pf_clearance_widest", 9), ("pf_clearance_widest_work", 2)):
        assert re.search(r"\bint %s\(pf_handle\* h," % name, header) and len(_lib.SYMBOLS[name][1]) == nargs
    kernels = open(os.path.join(root, "maaco-path-planing_amd", "csrc", "pf_widest.h")).read()
    tile = tuple(int(re.search(r"#define %s (\d+)" % n, kernels).group(1)) for n in ("PF_WD_TW", "PF_WD_TH"))
    assert tile == (tg.TW, tg.TH) == (64, 16)
