"""CPU oracle (oracle/pf_oracle.c) == the unmodified reference under the three non-default move policies
(allow_diag, restrict) = (1, 0), (0, 1), (0, 0): tests/golden/policy_cases.npz, captured by
`oracle/capture_golden.py policies`.  Runs anywhere (no GPU, no reference tree)."""
import numpy as np

import golden_io as gio
import pf_oracle as po
from pathfit import rng as pfrng

_orc = {}


def orc(name, ad, rs):
    key = (name, int(ad), int(rs))
    if key not in _orc:
        g, s, t = score_grid(name)
        _orc[key] = (po.Oracle(g, ad, rs), s, t)
    return _orc[key]


def score_grid(name):
    """The fixture grids, plus the obstacle-free map the score cases use."""
    if name == "open":
        R, C = (int(v) for v in gio.load("policy_cases")["open_map_shape"])
        g = np.zeros((R, C), np.uint8)
        g[0, 0], g[-1, -1] = 2, 3
        return g, 0, R * C - 1
    return gio.grid(name)


def test_connectors_all_variants():
    """AStarSolver.solve / MPA._a_star / DijkstraSolver.solve: paths and the reference's heap pops / pushes."""
    z = gio.load("policy_cases")
    names = [str(s) for s in z["grid_names"]]
    n = len(z["as_start"])
    assert n > 400
    seen = set()
    for i in range(n):
        ad, rs = (int(v) for v in z["policies"][int(z["as_policy"][i])])
        o, _, _ = orc(names[int(z["as_grid"][i])], ad, rs)
        avoid = gio.csr_get(z["as_avoid_off"], z["as_avoid"], i) if z["as_has_avoid"][i] else None
        variant = int(z["as_variant"][i])
        path, st = o.astar(int(z["as_start"][i]), int(z["as_target"][i]), avoid, variant)
        want = gio.csr_get(z["as_path_off"], z["as_path"], i)
        assert np.array_equal(path, want), (i, ad, rs, variant)
        pops, pushes = (int(v) for v in z["as_counts"][i])
        if len(want) != 1 and not (len(want) == 0 and pops == 0):
            assert st[0] == pops and st[1] == pushes, (i, ad, rs, variant, st[:2], pops, pushes)
        if len(want) > 1:
            seen.add((ad, rs, variant))
            steps = np.abs(np.diff(want // o.C)) + np.abs(np.diff(want % o.C))
            assert ad or (steps == 1).all(), i                       # 4-connected paths take unit steps only
    assert len(seen) == 9                                            # every policy and variant found paths


def test_decodes_and_stats():
    """GA chromosome and PSO position decodes with _calculate_stats_for_path, under main.py's and the default weights."""
    z = gio.load("policy_cases")
    names = [str(s) for s in z["grid_names"]]
    feasible = 0
    for i in range(len(z["dec_kind"])):
        ad, rs = (int(v) for v in z["policies"][int(z["dec_policy"][i])])
        o, s, t = orc(names[int(z["dec_grid"][i])], ad, rs)
        w = z["main_w"] if z["dec_w"][i] == 0 else z["def_w"]
        wp = gio.csr_get(z["dec_wp_off"], z["dec_wp"], i)
        cells = wp.astype(np.int32) if z["dec_kind"][i] == 0 else o.pso_round(wp)
        path, _ = o.decode(s, t, cells)
        want = gio.csr_get(z["dec_path_off"], z["dec_path"], i)
        assert np.array_equal(path, want), (i, ad, rs)
        assert np.array_equal(o.score(path, 0, w[0], w[1], w[2], rs, w[3]), z["dec_stats"][i]), (i, ad, rs)
        feasible += len(want) > 0
    assert feasible >= 30


def test_mpa_rebuilds():
    """MPA._reconstruct_path_segment: rebuilt path, number of draws from the agent's stream, MPA._calculate_path_stats."""
    z = gio.load("policy_cases")
    names = [str(s) for s in z["grid_names"]]
    seed, it = (int(v) for v in z["reb_seed_it"])
    changed = 0
    for i in range(len(z["reb_idx"])):
        ad, rs = (int(v) for v in z["policies"][int(z["reb_policy"][i])])
        o, s, t = orc(names[int(z["reb_grid"][i])], ad, rs)
        beta = float(z["reb_beta"][i])
        sigma = float(z["reb_sigma"][0 if beta == 1.5 else 1])
        g = o.rng(seed, pfrng.DOM_MPA, it, int(z["reb_agent"][i]))
        inp = gio.csr_get(z["reb_in_off"], z["reb_in"], i)
        out, _, _, _ = o.mpa_rebuild(s, t, inp, gio.csr_get(z["reb_el_off"], z["reb_el"], i), int(z["reb_idx"][i]),
                                     int(z["reb_is_levy"][i]), float(z["reb_scale"][i]), beta, sigma, g)
        assert np.array_equal(out, gio.csr_get(z["reb_out_off"], z["reb_out"], i)) and g.ctr == z["reb_draws"][i], i
        assert np.array_equal(o.score(out, 1, 0.1, 0.05, 1.5, rs, 1000.0), z["reb_stats"][i]), i
        changed += not np.array_equal(out, inp)
    assert changed > 30


def test_scores_of_hand_built_paths():
    """helper.calculate_path_stats (variant 0) and MPA._calculate_path_stats (variant 1) under restrict 1 and 0: paths of
    1 .. 130 cells with turns and corner cuts at the 64-cell chunk boundaries, steps of any length, an obstacle-free map."""
    z = gio.load("policy_cases")
    names = [str(s) for s in z["sc_grid_names"]]
    for i in range(len(z["sc_variant"])):
        o, _, _ = orc(names[int(z["sc_grid"][i])], 1, 1)
        wt, ws, ms, dp = z["sc_weights"][int(z["sc_w"][i])]
        path = gio.csr_get(z["sc_path_off"], z["sc_path"], i)
        got = o.score(path, int(z["sc_variant"][i]), wt, ws, ms, int(z["sc_restrict"][i]), dp)
        assert np.array_equal(got, z["sc_stats"][i]), (i, got, z["sc_stats"][i])
    cut = z["sc_stats"][:, 3] > 0
    assert cut.any() and not (cut & (z["sc_restrict"] == 0)).any()
    assert ((z["sc_restrict"] == 1) & (z["sc_stats"][:, 3] >= 300)).any()        # several cuts in one path


def test_oracle_loops_match_reference_solves_4_connected():
    """GASolver.solve and MPA.solve_path_planning of the reference on fig7 with allow_diagonal_moves=False == the GA facade's
    host logic over the oracle and the oracle-driven MPA loop."""
    import pf_loops
    from test_e2e_golden import GA_KW, _NoEngine, _oracle_backed_ga, curve_eq
    z = gio.load("policy_cases")
    g, s, t = gio.grid("fig7")
    ga = _oracle_backed_ga(po.Oracle(g, 0, 1))(g, engine=_NoEngine(), seed=4, allow_diagonal_moves=False, **GA_KW)
    res = ga.solve()
    assert [r * 20 + c for r, c in res[0]] == list(z["ga_path"])
    assert np.array_equal(np.array(res[1:], float), z["ga_stats"])
    assert np.array_equal(np.array(ga.convergence_curve), z["ga_curve"])
    assert np.array_equal([p["fitness"] for p in ga.population], z["ga_pop_fitness"])
    ref = pf_loops.MpaOracle(po.Oracle(g, 0, 1), s, t, 30, 20, seed=2)
    best = ref.solve()
    assert np.array_equal(best[0], z["mpa_path"]) and np.array_equal(best[1], z["mpa_stats"])
    assert curve_eq(ref.curve, z["mpa_curve"])
    assert np.array_equal([p[1][4] for p in ref.pop], z["mpa_pop_fitness"])
    assert np.array_equal([len(p[0]) for p in ref.pop], z["mpa_pop_len"])
