"""CPU oracle == the unmodified reference on random cases (fixed seeds): the reference's answers were captured into
tests/golden/vs_reference.npz (oracle/capture_golden.py, `vs_reference`).  Runs anywhere (no GPU, no reference tree)."""
import numpy as np
import pytest

import golden_io as gio


@pytest.fixture(scope="module")
def env():
    import pf_oracle as po
    g, _, _ = gio.grid("fig7")
    return gio.load("vs_reference"), po, g


def test_astar_random_triples(env):
    z, po, g = env
    orc = po.Oracle(g)
    for t, (s, e) in enumerate(z["astar_se"]):
        ac = [int(a) for a in gio.csr_get(z["astar_avoid_off"], z["astar_avoid"], t)] if z["astar_has_avoid"][t] else None
        for v in range(3):                                      # AStarSolver.solve, MPA._a_star, DijkstraSolver.solve
            pc = gio.csr_get(z[f"astar_v{v}_path_off"], z[f"astar_v{v}_path"], t)
            oc, st = orc.astar(int(s), int(e), ac, v)
            cnt = z[f"astar_v{v}_counts"][t]
            assert np.array_equal(pc, oc) and (len(pc) <= 1 or (cnt[0], cnt[1]) == (st[0], st[1])), (t, v)


def test_decode_score_random(env):
    z, po, g = env
    orc = po.Oracle(g)
    for t, chrom in enumerate(z["decode_chrom"]):
        oc, _ = orc.decode(0, 399, [int(w) for w in chrom])
        assert np.array_equal(gio.csr_get(z["decode_ga_path_off"], z["decode_ga_path"], t), oc)
        assert list(orc.score(oc, 0, 0.3, 0.8, 1.8, True, 100.0)) == list(z["decode_ga_stats"][t])
        oc, _ = orc.decode(0, 399, orc.pso_round(z["decode_pos"][t]))
        assert np.array_equal(gio.csr_get(z["decode_pso_path_off"], z["decode_pso_path"], t), oc)


@pytest.mark.parametrize("beta", [7.0, 2.0])
def test_maaco_iterations(env, beta):
    z, po, g = env
    k = f"maaco_b{beta:g}"
    orc = po.Oracle(g)
    P = po.MaacoParams(alpha=1.0, beta=beta, rho=0.1, Q=2.5, a_turn=1.0, wh_max=0.9, wh_min=0.2, k_h=0.9,
                       q0_initial=0.5, C0=0.1, num_iterations=10)
    tau, dist = orc.maaco_init(0, 399, 0.1)
    assert np.array_equal(tau.reshape(20, 20), z[k + "_tau0"])
    best = float("inf")
    for it in range(1, 5):
        paths, lens = [], []
        for ant in range(12):
            j = (it - 1) * 12 + ant
            pc, (L, T) = gio.csr_get(z[k + "_path_off"], z[k + "_path"], j), z[k + "_len_turns"][j]
            oc, oL, oT, _ = orc.maaco_walk(0, 399, P, tau, dist, it, 31, ant)
            assert np.array_equal(pc, oc) and L == oL and T == oT
            paths.append(oc); lens.append(oL); best = min(best, oL)
        orc.maaco_update(tau, 0.1, 2.5, paths, lens, best)
        assert np.array_equal(tau.reshape(20, 20), z[k + "_tau"][it - 1])


@pytest.mark.parametrize("beta", [1.5, 2.0])
def test_mpa_rebuild_random(env, beta):
    z, po, g = env
    from pathfit import rng as pfrng
    from pathfit.mpa import levy_sigma
    k = f"mpa_b{beta:g}"
    orc = po.Oracle(g)
    base, alt = z[k + "_base"], z[k + "_alt"]
    for t, (idx, is_levy, scale) in enumerate(z[k + "_cases"]):
        path_c, el_c = (base, alt) if t % 2 else (alt, base)
        gR = orc.rng(17, pfrng.DOM_MPA, 2, t)
        oc, _, _, _ = orc.mpa_rebuild(0, 399, path_c, el_c, int(idx), bool(is_levy), float(scale), beta, levy_sigma(beta), gR)
        assert np.array_equal(gio.csr_get(z[k + "_path_off"], z[k + "_path"], t), oc) and gR.ctr == z[k + "_draws"][t]
        assert list(orc.score(oc, 1, 0.1, 0.05, 1.5, True, 1000.0)) == list(z[k + "_res"][t])
