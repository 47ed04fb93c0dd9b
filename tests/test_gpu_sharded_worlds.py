"""The sharded solvers of pathfit/dist.py at 3, 5 and 8 ranks on the real engine: tests/sharded_cases.py, every case as `world` gloo
processes that share GPU 0.  These are the runs in which the device kernels see a non-zero agent offset and a local population
smaller than the global one -- pf_maaco_walk_batch with ant0 > 0 (both walk kernels), pf_maaco_deposit_cells on row chunks of a
received matrix, pf_mpa_local_view, pf_ga_breed_dev / pf_ga_assemble_dev with lo > 0, pf_pso_update with agent0 > 0, the device
scan and sort over an all-gathered column made of uneven blocks -- at splits with one-agent shards, boundaries off every
multiple of 8 and shards longer than a 64-agent word.

Every rank must equal the one-process solver, which in turn must equal the CPU oracle at these new populations; all comparisons
are exact except the one the all-reduce form of the pheromone update documents.  The oracle also says which agents' rows had to
cross a rank boundary (sharded_cases.winners), and the case asserts that one did.

Every case starts ONE group of ranks and waits for it under a time limit; nothing is retried.  The parent makes its own solo run
only after the group has been joined, on ONE engine it keeps for all cases, so at most 9 processes hold the GPU and the parent's
share of it does not grow.  If a rank ends by itself with a non-zero status -- a signal, 134 / 139, or status 1: a HIP error
reaches Python as an exception -- or is still running at the limit, the cases after it skip themselves: nothing more is started
on a GPU that may have faulted (sharded_cases.run_group; tests/test_sharded_cases.py pins the launcher on any host)."""
import numpy as np
import pytest

import sharded_cases as sc

pytestmark = pytest.mark.gpu

_solo = {}
_engine = []


def solo(case):
    """The one-process solver at this population (shared by the cases that differ only in how the run is sharded).  All solo runs
    take turns on one engine: the parent holds one device context and one set of fig7-sized buffers while the groups run.  What
    is kept per population are host arrays (a 20 x 20 matrix, columns of at most 200 rows), and the oracle runs that
    sharded_cases caches never touch the device."""
    import pathfit
    key = (case["solver"], case["n"], case["seed"], bool(case.get("sync")))
    if key in _solo:
        return _solo[key]
    g, s, t = sc.grid()
    if not _engine:
        _engine.append(pathfit.Engine(g))
    eng = _engine[0]
    n, seed = case["n"], case["seed"]
    if case["solver"] == "maaco":
        m = pathfit.MAACO(g, n, sc.MAACO_ITERS, seed=seed, engine=eng, **sc.MK)
        path, length, turns = m.solve_path_planning()
        out = dict(path=path, length=length, turns=turns, tau=np.array(m.pheromone_matrix), curve=list(m.convergence_curve_data))
    elif case["solver"] == "mpa":
        m = pathfit.MPA(g, n, sc.MPA_ITERS, seed=seed, engine=eng)
        res = m.solve_path_planning()
        out = dict(res=res, curve=list(m.convergence_curve_data))
    elif case["solver"] == "pso":
        ps = pathfit.PSOSolver(g, seed=seed, engine=eng, num_particles=n, asynchronous=not case.get("sync"), **sc.PSO_KW)
        res = ps.solve()
        out = dict(res=res, curve=list(ps.convergence_curve), pos=ps._pos.copy(), pbf=ps._pbest_fit.copy())
    else:
        ga = pathfit.GASolver(g, seed=seed, engine=eng, population_size=n, **sc.GA_KW)
        res = ga.solve()
        out = dict(res=res, curve=list(ga.convergence_curve), popfit=np.array([p["fitness"] for p in ga.population]))
    _solo[key] = out
    return out


def check_solo_vs_oracle(case, so):
    C = sc.grid()[0].shape[1]
    n, seed = case["n"], case["seed"]
    if case["solver"] == "maaco":
        ref = sc.maaco_oracle(n, seed)[0]
        assert [r * C + c for r, c in so["path"]] == list(ref["path"]) and so["length"] == ref["length"] and so["turns"] == ref["turns"]
        assert so["curve"] == ref["curve"] and np.array_equal(so["tau"], ref["tau"])
    elif case["solver"] == "mpa":
        mo, best, _ = sc.mpa_oracle(n, seed)
        got = so["res"]
        assert [r * C + c for r, c in got[0]] == list(best[0])
        assert (got[1], got[2], got[3], got[4], got[5]) == (best[1][0], int(best[1][1]), best[1][2], best[1][3], best[1][4])
        assert so["curve"] == mo.curve
    elif case["solver"] == "pso":
        ref = sc.pso_oracle(n, seed, bool(case.get("sync")))
        got = so["res"]
        assert got[0] == ref["path"] and so["curve"] == ref["curve"]
        assert (got[1], got[2], got[3], got[4], got[5]) == (ref["stats"][0], int(ref["stats"][1]), ref["stats"][2], ref["stats"][3], ref["stats"][4])
        assert np.array_equal(so["pos"], ref["pos"]) and np.array_equal(so["pbf"], ref["pbf"])
    else:
        res, curve, popfit = sc.ga_oracle(n, seed)
        assert so["res"] == res and so["curve"] == curve and np.array_equal(so["popfit"], popfit)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c["id"])
def test_every_rank_equals_solo_equals_oracle(tmp_path, case):
    if sc.stopped:
        pytest.skip("not started: " + sc.stopped[0])
    ok, report, wall = sc.run_group(case, tmp_path)
    print("group wall seconds: %.1f (limit %.0f)" % (wall, sc.GROUP_LIMIT_S))
    assert ok, report
    z = sc.load_ranks(case, tmp_path)
    so = solo(case)                                           # only now: the group's processes are gone
    check_solo_vs_oracle(case, so)
    if case["solver"] != "ga":                                # from the oracle: a winner's row had to come from another rank than 0
        assert any(r != 0 for r in sc.winner_owners(case)), sc.winners(case)
    for r, zz in enumerate(z):
        if case["solver"] == "maaco":
            assert np.array_equal(zz["path"], np.array(so["path"])) and float(zz["length"]) == so["length"], r
            assert float(zz["turns"]) == so["turns"] and np.array_equal(zz["curve"], np.array(so["curve"], float)), r
            if case.get("strict", 1):
                assert np.array_equal(zz["tau"], so["tau"]), r        # the ordered, pipelined fold == the sequential deposits
            else:
                # all_reduce(SUM) of the ranks' deltas adds the deposits in another order than the reference's ant-by-ant loop:
                # the documented ulp-level deviation of strict=False (pathfit/dist.py, C1) -- the one comparison that is not
                # exact.  Among the ranks the matrix is the same bit for bit (every rank receives the same sum).
                assert np.allclose(zz["tau"], so["tau"], rtol=1e-12, atol=0), r
                assert np.array_equal(zz["tau"], z[0]["tau"]), r
        else:
            res = so["res"]
            assert np.array_equal(zz["path"], np.array(res[0])) and np.array_equal(zz["stats"], np.array(res[1:], float)), r
            assert np.array_equal(zz["curve"], np.array(so["curve"], float)), r
            if case["solver"] == "ga":
                assert np.array_equal(zz["popfit"], so["popfit"]), r
    if case["solver"] == "pso":
        cn = sc.counts_of(case)
        assert [len(zz["pos"]) for zz in z] == cn and [len(zz["pbf"]) for zz in z] == cn
        assert np.array_equal(np.concatenate([zz["pos"] for zz in z]), so["pos"])
        assert np.array_equal(np.concatenate([zz["pbf"] for zz in z]), so["pbf"])
