"""MAACOBatch: K colonies walked, scored and updated in one batched iteration.  Every colony must equal, bit for bit, a solo run
with its seed, start and target -- the oracle loop (oracle/pf_loops.py) on the 20 x 20 map, a solo pathfit.MAACO on the 128 x 128
bench map -- in best path, length, turns, convergence curve and pheromone."""
import ctypes as C

import numpy as np
import pytest

import golden_io as gio
from batch_edge_cases import free_pairs, moved               # noqa: F401  (shared by the batch test files)

pytestmark = pytest.mark.gpu

KW = dict(alpha=1.0, beta=7.0, rho=0.1, Q=2.5, a_turn_coef=1.0, wh_max=0.9, wh_min=0.2, k_h_adaptive=0.9, q0_initial=0.5)


def check_vs_oracle(col, ref, C_):
    assert [r * C_ + c for r, c in col.best_path_overall] == list(ref["path"])
    assert col.best_path_length_overall == ref["length"] and col.best_path_turns_overall == ref["turns"]
    assert col.convergence_curve_data == ref["curve"]
    assert np.array_equal(col.pheromone_matrix, ref["tau"])


def batch_vs_oracle(n_ants, iters, pairs_seeds, **kw):
    import pathfit, pf_oracle as po, pf_loops
    g, _, _ = gio.grid("fig7")
    seeds = [sd for _, sd in pairs_seeds]
    starts = [p[0] for p, _ in pairs_seeds]
    targets = [p[1] for p, _ in pairs_seeds]
    b = pathfit.MAACOBatch(g, n_ants, iters, C0_initial_pheromone=0.1, seeds=seeds, starts=starts, targets=targets, **kw)
    res = b.solve_path_planning()
    assert len(res) == len(seeds)
    orc = po.Oracle(g)
    for k, (s, t) in enumerate(zip(starts, targets)):
        ref = pf_loops.maaco_solve(orc, s[0] * 20 + s[1], t[0] * 20 + t[1], n_ants, iters, C0=0.1, seed=seeds[k], **kw)
        check_vs_oracle(b.colony(k), ref, 20)
        assert [r * 20 + c for r, c in res[k][0]] == list(ref["path"]) and res[k][1] == ref["length"]
    return b


@pytest.mark.parametrize("beta", [7.0, 2.0])
def test_batch_fig7_six_colonies_match_oracle_loop(beta):
    g, s, t = gio.grid("fig7")
    pairs = [((0, 0), (19, 19))] + free_pairs(g, 2, seed=7)
    kw = dict(KW, beta=beta)
    batch_vs_oracle(50, 12, [(p, sd) for p in pairs for sd in (3, 8)], **kw)


def test_batch_ant_ranges_cross_64_ant_words():
    """n = 100: colony c's ants are global ants [100 c, 100 c + 100), so 64-ant words of the walk straddle colonies while every
    colony's bit matrix and deposits stay at its local indices."""
    g, _, _ = gio.grid("fig7")
    pairs = free_pairs(g, 4, seed=11)
    batch_vs_oracle(100, 6, [(p, 20 + i) for i, p in enumerate(pairs)], **KW)


def test_batch_alpha_not_one_uses_host_pow_per_colony():
    g, _, _ = gio.grid("fig7")
    pairs = [((0, 0), (19, 19))] + free_pairs(g, 2, seed=5)
    kw = dict(KW, alpha=1.5, beta=3.0, rho=0.2, q0_initial=0.3)
    batch_vs_oracle(24, 5, [(p, 9 + i) for i, p in enumerate(pairs)], **kw)


def test_batch_dense_deposit_words_q110():
    """400 ants a colony on the 20 x 20 map: dense 64-ant words around every start, deposits on both sides of the scaling limit."""
    g, _, _ = gio.grid("fig7")
    pairs = [((0, 0), (19, 19))] + free_pairs(g, 1, seed=3)
    batch_vs_oracle(400, 3, [(p, 11 + i) for i, p in enumerate(pairs)], **dict(KW, Q=110.0))


@pytest.mark.parametrize("n_ants", [50, 3000])
def test_batch_path_rows_too_short_redo(n_ants):
    """Rows of 8 cells: the first attempt overflows (somewhere in the batch), no colony's pheromone moves, the iteration is redone
    with longer rows; the results equal the oracle loop (one ant per wave at 3 x 50 ants, eight per wave at 3 x 3000)."""
    import pathfit, pf_oracle as po, pf_loops
    g, _, _ = gio.grid("fig7")
    pairs = [((0, 0), (19, 19))] + free_pairs(g, 2, seed=13)
    seeds = [3, 4, 5]
    b = pathfit.MAACOBatch(g, n_ants, 4, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    tau0 = [b.colony(k).pheromone_matrix for k in range(3)]
    # one raw attempt with 8-cell rows: skipped, every colony's tau untouched
    b.path_cap = 8
    dc, dl, dp, dt, ds = b._alloc()
    bl = np.full(3, np.inf)
    bt = np.full(3, np.inf)
    out = np.empty((3, 13))
    b._ck(b.engine.L.pf_maaco_batch_iterate(b._b, 1, n_ants, 8, dc.ptr, dl.ptr, dp.ptr, dt.ptr, ds.ptr, bl.ctypes.data, bt.ctypes.data,
                                            out.ctypes.data))
    assert out[0, 12] > 0 and all(out[k, 8] == 1.0 for k in range(3))
    for k in range(3):
        assert np.array_equal(b.colony(k).pheromone_matrix, tau0[k])
    res = b.solve_path_planning()
    assert b.path_cap > 8
    orc = po.Oracle(g)
    for k, (s, t) in enumerate(pairs):
        ref = pf_loops.maaco_solve(orc, s[0] * 20 + s[1], t[0] * 20 + t[1], n_ants, 4, C0=0.1, seed=seeds[k], **KW)
        check_vs_oracle(b.colony(k), ref, 20)
        assert res[k][1] == ref["length"]


def solo_runs(g, pairs, seeds, n_ants, iters, eng):
    """per colony: tau after every iteration, curve, best path / length / turns of a solo MAACO (on one shared engine, one after another)"""
    import pathfit
    out = []
    for (s, t), sd in zip(pairs, seeds):
        m = pathfit.MAACO(moved(g, s, t), n_ants, iters, engine=eng, seed=sd, **KW)
        taus = []
        for it in range(1, iters + 1):
            m.iterate_dev(it)
            taus.append(m.pheromone_matrix.copy())
        out.append(dict(taus=taus, curve=list(m.convergence_curve_data), path=m.best_path_overall,
                        length=m.best_path_length_overall, turns=m.best_path_turns_overall))
    return out


@pytest.mark.parametrize("K,ahead", [(16, -1), (16, 0), (16, 1), (4, -1)])
def test_batch_bench128_matches_solo_maaco(K, ahead):
    """cfg-2 colonies (256 ants on the 128 x 128 bench map): K = 16 is 4096 ants, the packed kernel (both load-ahead forms forced
    once), K = 4 is 1024 ants, one ant per wave.  Pheromone compared after every iteration."""
    import pathfit
    from pathfit import env
    g = env.bench_grid(128)
    pairs = [((0, 0), (127, 127))] + free_pairs(g, K - 1, seed=128)
    seeds = [100 + k for k in range(K)]
    eng = pathfit.Engine(g)
    iters = 5
    ref = solo_runs(g, pairs, seeds, 256, iters, eng)
    b = pathfit.MAACOBatch(g, 256, iters, engine=eng, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    eng.set_option("maaco_load_ahead", ahead)
    try:
        for it in range(1, iters + 1):
            b.iterate_dev(it)
            for k in range(K):
                assert np.array_equal(b.colony(k).pheromone_matrix, ref[k]["taus"][it - 1]), (k, it)
    finally:
        eng.set_option("maaco_load_ahead", -1)
    for k in range(K):
        col = b.colony(k)
        assert col.convergence_curve_data == ref[k]["curve"], k
        assert col.best_path_overall == ref[k]["path"] and col.best_path_length_overall == ref[k]["length"], k
        assert col.best_path_turns_overall == ref[k]["turns"], k
        assert (col.start_node, col.target_node) == pairs[k]


def test_batch_colonies_are_independent():
    """Colony k of a K = 5 batch == a K = 1 batch with the same seed, start and target."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    pairs = free_pairs(g, 5, seed=21)
    seeds = [40, 41, 42, 43, 44]
    b5 = pathfit.MAACOBatch(g, 60, 6, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    r5 = b5.solve_path_planning()
    for k in (0, 2, 4):
        b1 = pathfit.MAACOBatch(g, 60, 6, engine=b5.engine, seeds=[seeds[k]], starts=[pairs[k][0]], targets=[pairs[k][1]], **KW)
        r1 = b1.solve_path_planning()
        assert r1[0] == r5[k]
        assert b1.colony(0).convergence_curve_data == b5.colony(k).convergence_curve_data
        assert np.array_equal(b1.colony(0).pheromone_matrix, b5.colony(k).pheromone_matrix)


def test_batch_shares_an_engine_with_a_solo_maaco():
    """A solo MAACO and a batch on one Engine, interleaved iteration by iteration: the solo run still equals its standalone run."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    alone = pathfit.MAACO(g, 50, 8, seed=6, **KW)
    want = alone.solve_path_planning()
    want_tau = alone.pheromone_matrix
    eng = pathfit.Engine(g)
    m = pathfit.MAACO(g, 50, 8, engine=eng, seed=6, **KW)
    pairs = free_pairs(g, 3, seed=2)
    b = pathfit.MAACOBatch(g, 50, 8, engine=eng, seeds=[1, 2, 3], starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    for it in range(1, 9):
        m.iterate_dev(it)
        b.iterate_dev(it)
    assert (m.best_path_overall, m.best_path_length_overall, m.best_path_turns_overall) == want
    assert m.convergence_curve_data == alone.convergence_curve_data
    assert np.array_equal(m.pheromone_matrix, want_tau)
    # and the batch's colonies equal their own batch run on a fresh engine
    b2 = pathfit.MAACOBatch(g, 50, 8, seeds=[1, 2, 3], starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    b2.solve_path_planning()
    for k in range(3):
        assert b2.colony(k).convergence_curve_data == b.colony(k).convergence_curve_data
        assert np.array_equal(b2.colony(k).pheromone_matrix, b.colony(k).pheromone_matrix)


def test_batch_pheromone_round_trip_and_grid_update():
    import pathfit
    from pathfit import PathfitError
    g, _, _ = gio.grid("fig7")
    b = pathfit.MAACOBatch(g, 20, 2, seeds=[1, 2], **KW)
    col = b.colony(1)
    tau = col.pheromone_matrix
    col.pheromone_matrix = tau * 2.0
    assert np.array_equal(col.pheromone_matrix, tau * 2.0)
    assert np.array_equal(b.colony(0).pheromone_matrix, tau)      # same start / target, untouched
    b.engine.update_grid(np.asarray(g))
    with pytest.raises(PathfitError, match="replaced grid"):
        b.iterate_dev(1)
    b.close()
