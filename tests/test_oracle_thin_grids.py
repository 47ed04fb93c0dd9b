"""CPU oracle == the unmodified reference on maps with a side of 1, 2 or 3 cells (tests/thin_maps.py), up to row / column
4095: the reference's answers were captured into tests/golden/thin_cases.npz (oracle/capture_golden.py, `thin`).  Runs
anywhere (no GPU, no reference tree).  Also pins the capacity of a decode's path row (pathfit.solvers.path_capacity)."""
import numpy as np
import pytest

import golden_io as gio
import thin_maps as tm


@pytest.fixture(scope="module")
def env():
    import pf_oracle as po
    z = gio.load("thin_cases")
    names = [str(n) for n in z["grid_names"]]
    orcs = {n: po.Oracle(gio.thin_grid(z, n)[0]) for n in names}
    return z, po, names, orcs


def test_stored_grids_are_the_numpy_recipe(env):
    z, _, names, _ = env
    assert names == [tm.name_of(*m) for m in tm.all_maps()]
    for (R, C, ob), n in zip(tm.all_maps(), names):
        g, s, t = tm.thin_map(R, C, ob)
        g2, s2, t2 = gio.thin_grid(z, n)
        assert np.array_equal(g, g2) and (s, t) == (s2, t2), n
        if ob:
            assert 0.12 <= (g == 1).mean() <= 0.15 or R * C < 30, n


def test_connectors(env):
    z, _, names, orcs = env
    seen = {n: [0, 0] for n in names}                        # per grid: longest path, infeasible results
    for i in range(len(z["as_start"])):
        n = names[z["as_grid"][i]]
        o, v = orcs[n], int(z["as_variant"][i])
        av = [int(a) for a in gio.csr_get(z["as_avoid_off"], z["as_avoid"], i)] if z["as_has_avoid"][i] else None
        want = gio.csr_get_delta(z["as_path_off"], z["as_path_d"], i)
        got, st = o.astar(int(z["as_start"][i]), int(z["as_target"][i]), av, v)
        assert np.array_equal(got, want), (n, i, v)
        assert len(want) <= 1 or (st[0], st[1]) == tuple(z["as_counts"][i]), (n, i, v)
        if v != 1:                                           # AStarSolver / DijkstraSolver return the scored 6-tuple
            assert np.array_equal(o.score(got, 0, 0.3, 0.8, 1.8, True, 100.0), z["as_stats"][i]), (n, i, v)
        seen[n][0] = max(seen[n][0], len(want)); seen[n][1] += len(want) == 0
    for n in names:
        assert seen[n][0] >= max(orcs[n].R, orcs[n].C) / 2, n
        assert seen[n][1] > 0 or n.endswith("e"), n


def test_decodes_and_scores(env):
    z, _, names, orcs = env
    longer = 0
    for i in range(len(z["dec_kind"])):
        n = names[z["dec_grid"][i]]
        o = orcs[n]
        _, s, t = gio.thin_grid(z, n)
        wp = gio.csr_get(z["dec_wp_off"], z["dec_wp"], i)
        cells = wp.astype(np.int32) if z["dec_kind"][i] == 0 else o.pso_round(wp.reshape(-1, 2))
        got, _ = o.decode(s, t, cells)
        want = gio.csr_get_delta(z["dec_path_off"], z["dec_path_d"], i)
        assert np.array_equal(got, want), (n, i)
        w = z["dec_weights"][z["dec_w"][i]]
        assert np.array_equal(o.score(got, 0, w[0], w[1], w[2], True, w[3]), z["dec_stats"][i]), (n, i)
        longer += len(want) > o.R * o.C
    assert longer >= 2
    # the two decodes every waypoint of which is a cell the chain has already visited (astar.py:55-56 exempts the goal)
    a, b = (int(v) for v in z["dec_long"])
    assert list(gio.csr_get_delta(z["dec_path_off"], z["dec_path_d"], a)) == [0, 1, 0, 1]
    assert list(gio.csr_get_delta(z["dec_path_off"], z["dec_path_d"], b)) == [0, 1, 3, 2, 0, 3]


def test_maaco_iterations(env):
    z, po, names, orcs = env
    bp = z["maaco_base_params"]
    for ri, (gi, beta, n_ants, n_it, K, seed) in enumerate(z["maaco_runs"]):
        n = names[int(gi)]
        o = orcs[n]
        _, s, t = gio.thin_grid(z, n)
        P = po.MaacoParams(alpha=bp[0], beta=beta, rho=bp[1], Q=bp[2], a_turn=bp[3], wh_max=bp[4], wh_min=bp[5], k_h=bp[6],
                           q0_initial=bp[7], C0=bp[8], num_iterations=int(K))
        tau, dist = o.maaco_init(s, t, bp[8])
        assert np.array_equal(tau.reshape(o.R, o.C), z[f"maaco{ri}_tau0"]), (n, beta)
        best, k = float("inf"), 0
        for it in range(1, int(n_it) + 1):
            paths, lens = [], []
            for ant in range(int(n_ants)):
                want = gio.csr_get_delta(z[f"maaco{ri}_path_off"], z[f"maaco{ri}_path_d"], k)
                L, T = z[f"maaco{ri}_len_turns"][k]
                got, oL, oT, _ = o.maaco_walk(s, t, P, tau, dist, it, int(seed), ant)
                assert np.array_equal(got, want) and oL == L and (oT == T or (len(want) == 0 and T == -1)), (n, beta, it, ant)
                paths.append(got); lens.append(oL); best = min(best, oL); k += 1
            o.maaco_update(tau, bp[1], bp[2], paths, lens, best)
            assert np.array_equal(tau.reshape(o.R, o.C), z[f"maaco{ri}_tau"][it - 1]), (n, beta, it)


def test_mpa_rebuilds(env):
    z, _, names, orcs = env
    from pathfit import rng as pfrng
    seed, it = (int(v) for v in z["reb_seed_it"])
    kinds = set()
    for i in range(len(z["reb_idx"])):
        n = names[z["reb_grid"][i]]
        o = orcs[n]
        _, s, t = gio.thin_grid(z, n)
        beta = float(z["reb_beta"][i])
        sigma = float(z["reb_sigma"][0 if beta == 1.5 else 1])
        path = gio.csr_get_delta(z["reb_in_off"], z["reb_in_d"], i)
        elite = gio.csr_get_delta(z["reb_el_off"], z["reb_el_d"], i)
        g = o.rng(seed, pfrng.DOM_MPA, it, int(z["reb_agent"][i]))
        got, _, _, _ = o.mpa_rebuild(s, t, path, elite, int(z["reb_idx"][i]), bool(z["reb_is_levy"][i]), float(z["reb_scale"][i]),
                                     beta, sigma, g)
        assert np.array_equal(got, gio.csr_get_delta(z["reb_out_off"], z["reb_out_d"], i)) and g.ctr == z["reb_draws"][i], (n, i)
        assert np.array_equal(o.score(got, 1, 0.1, 0.05, 1.5, True, 1000.0), z["reb_stats"][i]), (n, i)
        kinds.add(bool(z["reb_is_levy"][i]))
    assert kinds == {True, False}


def test_path_capacity_of_a_decode():
    """A decode of W waypoints holds at most R * C + W + 1 cells (every segment may end on a visited cell); the linear bound
    16 (R + C) + 64 applies where it is smaller -- on every map of the benchmark, whose rows keep the size they had."""
    from pathfit.solvers import decode_bound, path_capacity
    assert path_capacity(1, 2, 3) == 6 and path_capacity(2, 2, 5) == 10 and path_capacity(3, 3, 1) == 11
    assert path_capacity(1, 2, 3) >= 4 and path_capacity(2, 2, 5) >= 6       # the two reference examples fit
    assert path_capacity(2, 17, 5) == 2 * 17 + 6 and path_capacity(3, 200, 4) == 3 * 200 + 5
    assert path_capacity(1, 4096, 5) == 4096 + 6
    for W in (0, 1, 5, 40):
        assert decode_bound(12, 12, W) == 144 + W + 1
        for n in (128, 256, 512, 1024, 2048):                     # the benchmark runs 128, 512 and 1024
            assert path_capacity(n, n, W) == 16 * 2 * n + 64
    assert path_capacity(20, 20, 5) == 406                                  # (was 400: the grid itself)
    assert path_capacity(20, 20, 500) == 16 * 40 + 64
