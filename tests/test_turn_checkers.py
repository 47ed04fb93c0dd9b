"""The CPU checkers of the turn fields (tests/turn_checkers.py) pinned against each other: the literal heap Dijkstra over states, the
kernel's form of it, random-order sweeps, the route rule and the path cost -- and against cost_checkers.dijkstra at turn weight 0 and
the minimum over all simple paths on small grids.  Also the CPU facts tests/test_gpu_turn_field.py leans on, and the declarations.
Runs on a CPU-only host."""
import os
import re

import numpy as np
import pytest

import cost_checkers as ck
import field_checkers as fc
import turn_checkers as tk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def case(seed, kind, R=11, C=13):
    g = fc.seeded_map(R, C, 0.25, seed)
    free = [int(v) for v in np.flatnonzero(g.reshape(-1) != 1)]
    cost = None if kind == "none" else ck.cost_of_kind(kind, g.shape, seed)
    return g, cost, [free[0], free[len(free) // 2], free[0]]


@pytest.mark.parametrize("ad, rs", tk.POLICIES)
@pytest.mark.parametrize("kind", tk.KINDS)
def test_the_solvers_agree_bit_for_bit(kind, ad, rs):
    for seed in (1, 2):
        g, cost, src = case(seed, kind)
        mm = fc.move_masks(g, ad, rs)
        for wt in tk.WEIGHTS:
            T = tk.dijkstra(g, mm, cost, src, wt)
            assert same_bits(T, tk.dijkstra_fast(g, mm, cost, src, wt)), (seed, wt)
            assert same_bits(T, tk.sweeps(g, mm, cost, src, wt, seed)), (seed, wt)
            legal = np.array([(mm >> fc.OPP[d]) & 1 == 1 for d in range(8)])
            seeds = np.zeros(g.size, bool)
            seeds[src] = True
            assert np.all(np.isinf(T[~(legal | seeds.reshape(g.shape)[None])])) and np.all(T[:, seeds.reshape(g.shape)] == 0.0)
            if wt == 0.0:
                assert same_bits(T.min(axis=0), ck.dijkstra(g, mm, np.ones(g.shape) if cost is None else cost, src)[0]), seed


def test_no_cost_map_is_a_map_of_ones():
    g, _, src = case(3, "none")
    for ad, rs in tk.POLICIES:
        mm = fc.move_masks(g, ad, rs)
        assert same_bits(tk.dijkstra(g, mm, None, src, 0.3), tk.dijkstra(g, mm, np.ones(g.shape), src, 0.3))


@pytest.mark.parametrize("variant, wt", [("two_roundings", 0.1), ("two_roundings", 0.3), ("first_turn", 0.3), ("first_turn", 3.0)])
def test_wrong_solvers_are_rejected(variant, wt):
    hits = 0
    for seed in (1, 2, 3):
        g, cost, src = case(seed, "u50")
        mm = fc.move_masks(g, 1, 1)
        right = tk.dijkstra(g, mm, cost, src, wt)
        assert same_bits(right, tk.sweeps(g, mm, cost, src, wt, seed + 10))
        hits += not same_bits(right, tk.sweeps(g, mm, cost, src, wt, seed + 10, variant))
    assert hits == 3, (variant, hits)


def test_routes_cost_exactly_the_label_and_are_simple():
    for seed, kind, wt in ((1, "u50", 0.3), (2, "ones", 3.0), (3, "int14", 0.1), (4, "u1e6", float(2 ** 20)), (5, "none", 0.0)):
        g, cost, src = case(seed, kind, 14, 17)
        for ad, rs in tk.POLICIES:
            T, best, _ = tk.fields(g, cost, [src], wt, ad, rs)
            for t in range(g.size):
                cells = tk.route(T[0], cost, t, wt)
                if not np.isfinite(best[0].reshape(-1)[t]):
                    assert cells == []
                    continue
                total, turns = tk.path_cost(cost, cells, 17, wt)
                assert cells[-1] == t and cells[0] in src and len(set(cells)) == len(cells)
                assert total == best[0].reshape(-1)[t] and turns == tk.count_turns(cells, 17), (seed, t)
                assert (len(cells) == 1) == (t in src)


def test_the_minimum_over_all_simple_paths_on_3x4_grids():
    n = 0
    for seed in range(48):
        g = fc.seeded_map(3, 4, 0.25, seed)
        if g[0, 0] == 1:
            continue
        ad, rs = tk.POLICIES[seed % 4]
        cost = ck.cost_of_kind(("ones", "u50", "int14")[seed % 3], g.shape, seed)
        wt = tk.WEIGHTS[(seed // 4) % len(tk.WEIGHTS)]
        mm = fc.move_masks(g, ad, rs)
        best = tk.dijkstra(g, mm, cost, [0], wt).min(axis=0)
        assert same_bits(best, tk.simple_path_minimum(g, mm, cost, 0, wt)), (seed, ad, rs, wt)
        n += 1
    assert n >= 30


def test_a_state_whose_optimal_walk_revisits_a_cell():
    g, s, v, d = tk.pocket_map()
    for wt in (0.0, 0.3):
        T, best, _ = tk.fields(g, None, [[s]], wt, 1, 1)
        walk = tk.route(T[0], None, v, wt, heading=d)
        assert walk == [0, 1, 2, 1] and T[0].reshape(8, -1)[d, v] == tk.path_cost(None, walk, 3, wt)[0] == (1.0 + 1.0) + (1.0 + wt)
        assert tk.route(T[0], None, v, wt) == [0, 1] and best[0, 0, v] == 1.0          # the best state's walk does not


def test_the_turn_optimal_route_beats_dijkstras_on_the_zigzag_map():
    g, s, t = tk.zigzag_map()
    mm = fc.move_masks(g, 1, 1)
    short = fc.trace(fc.reference_dijkstra(g, mm, s)[1], t)
    T, best, _ = tk.fields(g, None, [[s]], 3.0, 1, 1)
    mine = tk.route(T[0], None, t, 3.0)
    assert tk.count_turns(short, 23) == 16 and mine != short
    assert tk.path_cost(None, mine, 23, 3.0)[0] == best[0].reshape(-1)[t] < tk.path_cost(None, short, 23, 3.0)[0]
    assert abs(best[0].reshape(-1)[t] - 63.66) < 0.005 and abs(tk.path_cost(None, short, 23, 3.0)[0] - 81.73) < 0.005


@pytest.mark.parametrize("stacked", [False, True])
def test_the_detour_maps_need_three_launches(stacked):
    cost, s, probe, far = tk.detour_map(stacked)
    for ad, rs in ((1, 1), (0, 1)):
        assert tk.needs_the_far_tile(cost, s, probe, far, 0.3, ad, rs), (stacked, ad, rs)


def test_the_four_entry_points_are_declared_and_bound():
    """The header declares them, the binding table holds them with the header's argument counts, and the tile the GPU tests size
    their maps by is the kernel's."""
    from pathfit import _lib
    hdr = open(os.path.join(ROOT, "include", "pathfit.h")).read()
    for name, nargs in (("pf_turn_field", 11), ("pf_turn_field_work", 2), ("pf_turn_field_paths", 13), ("pf_turn_paths", 10)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m and m.group(1).count(",") + 1 == nargs, name
        assert len(_lib.SYMBOLS[name][1]) == nargs and hasattr(_lib.lib(), name)
    src = open(os.path.join(ROOT, "maaco-path-planing_amd", "csrc", "pf_turn_field.h")).read()
    assert re.search(r"#define PF_TF_TW (\d+)", src).group(1) == str(tk.TW) and re.search(r"#define PF_TF_TH (\d+)", src).group(1) == str(tk.TH)
