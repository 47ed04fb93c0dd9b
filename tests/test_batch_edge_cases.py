"""The case table of tests/batch_edge_cases.py and the CPU facts its GPU run (tests/test_gpu_batch_edges.py) rests on, checked on
any host with the oracle alone: the policies show in the results, the MPA runs accept candidates in every phase and take a FADs
detour, walks fail on the obstacle maps, a thin-map school falls back to [start, target], decodes outgrow the 2 x 2 grid, and the
exact-fit length is reached after the first iteration.  Nothing here touches a device."""
import collections

import numpy as np
import pytest

import batch_edge_cases as bc


def total(events):
    ev = collections.Counter()
    for e in events:
        ev += e
    return ev


# ---- 1. move policies -----------------------------------------------------------------------------------------------------------
def test_mpa_policy_table_shares_start_and_target_cells():
    c = bc.MPA_POLICY
    g = bc.fig7()
    assert len(c["pairs"]) == len(c["seeds"]) == 4 and c["N"] == 24 and c["iters"] == 9
    assert all(g[s] != 1 and g[t] != 1 and s != t for s, t in c["pairs"])
    starts, targets = [p[0] for p in c["pairs"]], [p[1] for p in c["pairs"]]
    assert starts[0] == starts[1] and targets[1] == targets[2]          # shared bound tables
    assert len(set(starts)) == 3 and len(set(targets)) == 3


@pytest.mark.parametrize("ad,rs", bc.POLICIES)
def test_mpa_policy_runs_show_the_policy_and_every_branch(ad, rs):
    ref, base = bc.mpa_policy_reference(ad, rs), bc.mpa_policy_reference(1, 1)
    ev = total(ref["events"])
    assert ev["phase1"] > 0 and ev["phase2"] > 0 and ev["phase3"] > 0 and ev["detour_taken"] > 0, ev
    assert any(ref["log"][-1][k][2] != base["log"][-1][k][2] for k in range(4)), "no school's best path differs from the default policy's"
    if not ad:
        for it_log in ref["log"]:
            for paths, _, best, _ in it_log:
                assert all(bc.four_connected(p, 20) for p in paths) and bc.four_connected(best, 20)
    else:                                                                # corner cutting allowed: some path does cut one
        assert any(not bc.four_connected(p, 20) for it_log in ref["log"] for paths, _, _, _ in it_log for p in paths)


@pytest.mark.parametrize("ad,rs", bc.POLICIES)
def test_ga_policy_runs_show_the_policy(ad, rs):
    c = bc.GA_POLICY
    assert len(c["pairs"]) == 3 and c["kw"]["population_size"] == 24 and c["kw"]["num_generations"] == 4
    ref, base = bc.ga_policy_reference(ad, rs), bc.ga_policy_reference(1, 1)
    assert all(r is not None for r in ref)
    assert any(a[1][0] != b[1][0] for a, b in zip(ref, base)), "no population's best path differs from the default policy's"
    for ga, res in ref:
        assert len(ga.convergence_curve) == 5 and res[0][0] == ga.start_node and res[0][-1] == ga.target_node
        if not ad:
            assert bc.four_connected([r * 20 + c_ for r, c_ in res[0]], 20)


# ---- 2. thin maps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", bc.THIN_KEYS + [bc.THIN_LONG] + ["2x17e"])
def test_thin_units(key):
    g, pairs, seeds = bc.thin_units(key)
    R, C_ = g.shape
    _, s, t = bc.thin_grid(key)
    assert len(pairs) == len(seeds) == (2 if key == bc.THIN_LONG else 3) and len(set(seeds)) == len(seeds)
    assert pairs[0] == ((s // C_, s % C_), (t // C_, t % C_))
    assert all(g[a] != 1 and g[b] != 1 and a != b for a, b in pairs)
    assert min(R, C_) <= 3 and (R * C_ < 64 or max(R, C_) >= 200)
    far = bc.far_target(key, g)
    if key.endswith("o"):
        assert far is not None and pairs[1] == (pairs[0][0], (far // C_, far % C_))
    if key == bc.THIN_LONG:
        assert pairs[0][1] == (0, 4095)


@pytest.mark.parametrize("key", bc.THIN_KEYS + [bc.THIN_LONG])
def test_thin_maaco_walks(key):
    """On the obstacle maps walks of the far-target colony fail and colony 0's do not all fail; on the empty maps none fails."""
    for n_ants, beta in bc.thin_maaco_runs(key):
        ref = bc.thin_maaco_reference(key, n_ants, beta)
        iters = 2 if key == bc.THIN_LONG else 3
        assert all(walks == n_ants * iters for _, walks, _ in ref)
        if key.endswith("o"):
            assert ref[1][2] > 0 and ref[0][2] < ref[0][1], (key, n_ants, beta, [r[1:] for r in ref])
        else:
            assert all(failed == 0 for _, _, failed in ref)
        assert ref[0][0]["length"] < bc.INF and len(ref[0][0]["path"]) >= 2


def test_thin_mpa_fallback_school_beside_live_schools():
    fallback = 0
    for key in bc.THIN_KEYS:
        g, pairs, _ = bc.thin_units(key)
        cols = g.shape[1]
        ref = bc.thin_mpa_reference(key)
        assert len(ref["log"]) == bc.THIN_MPA["iters"] and all(len(s[0]) == bc.THIN_MPA["N"] for s in ref["log"][-1])
        for k, (s, t) in enumerate(pairs):
            ends = [bc.cell_of(s, cols), bc.cell_of(t, cols)]
            assert ref["first"][k][0] == ends[0] and ref["first"][k][-1] == ends[1]
        if key.endswith("o"):
            import pf_oracle as po
            orc = po.Oracle(g)
            dead = [k for k, (s, t) in enumerate(pairs) if not len(orc.astar(bc.cell_of(s, cols), bc.cell_of(t, cols), None, 1)[0])]
            live = [k for k in range(len(pairs)) if k not in dead]
            for k in dead:                                               # MPA.py:235-236: [start, target], through the whole run
                want = [bc.cell_of(pairs[k][0], cols), bc.cell_of(pairs[k][1], cols)]
                assert all(p == want for it_log in ref["log"] for p in it_log[k][0])
            fallback += bool(dead) and bool(live) and all(len(ref["first"][k]) > 2 for k in live)
    assert fallback >= 1
    assert [len(p) for p in bc.thin_mpa_reference("1x2e")["first"]] == [2, 2, 2]     # rows of 2 cells: path_cap = min(RC, ...) = 2


@pytest.mark.parametrize("key", bc.THIN_WP_KEYS)
def test_thin_ga_and_pso_references(key):
    g, pairs, _ = bc.thin_units(key)
    ga = bc.thin_ga_reference(key)
    pso = {sync: bc.thin_pso_reference(key, sync) for sync in (False, True)}
    live = [k for k in range(3) if ga[k] is not None]
    assert 0 in live and len(live) >= 2 and all((pso[sync][k] is not None) == (k in live) for sync in pso for k in range(3))
    if key.endswith("e"):
        assert live == [0, 1, 2]
    for k in live:
        assert len(ga[k][0].convergence_curve) == bc.THIN_GA_KW["num_generations"] + 1
        assert all(len(pso[sync][k]["curve"]) == bc.THIN_PSO_KW["num_iterations"] + 1 for sync in pso)
    if key == "2x2e":                                                    # the decodes are longer than the grid
        assert all(ga[k][0].longest > g.size for k in live) and all(pso[sync][k]["longest"] > g.size for sync in pso for k in live)


# ---- 3. slot wipes ----------------------------------------------------------------------------------------------------------------
def test_wipe_cases():
    g = bc.wrap_grid()
    assert g.shape == (48, 48)
    pairs = bc.wipe_mpa_pairs()
    assert len(pairs) == len(bc.WIPE_MPA["seeds"]) == 3 and all(g[s] != 1 and g[t] != 1 for s, t in pairs)
    ev = total(bc.wipe_mpa_reference()["events"])                       # the sweeps do search: rebuilt paths and detours, every iteration
    assert ev["phase1"] + ev["phase2"] + ev["phase3"] > 0 and ev["detour_tried"] > 0, ev
    assert len(bc.wipe_ga_pairs()) == len(bc.WIPE_GA["seeds"]) == 2
    ref = bc.wipe_maaco_reference()
    assert len(ref) == 3 and all(r[0]["length"] < bc.INF for r in ref)


# ---- 4. exact fit -------------------------------------------------------------------------------------------------------------------
def test_exact_fit_length_is_reached_after_the_first_iteration():
    """Lmax is longer than every initial path (so path_cap = Lmax - 1 still holds the initial populations) and is first built in an
    iteration after the first (so 'raises at the predicted iteration, and not earlier' says something)."""
    ref = bc.fit_mpa_reference()
    Lmax, at = bc.fit_lengths(ref)
    assert Lmax - 1 > max(len(p) for p in ref["first"]) and 2 <= at <= bc.FIT_MPA["iters"], (Lmax, at)
    assert Lmax < 400
