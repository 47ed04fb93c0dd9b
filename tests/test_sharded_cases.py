"""The sharded cases (tests/sharded_cases.py) and the exchange logic of pathfit/dist.py, checked on the CPU: the shard arithmetic
for every world up to 16, the case table and the cross-boundary winners it promises (from the oracle), ShardedMAACO over the
oracle-backed stand-ins at the populations of the GPU cases, what a world larger than the population does, and the group launcher
of the GPU file (its time limit, ending the survivors, the per-rank report, what stops the file) with trivial ranks.  No GPU."""
import os

import numpy as np
import pytest

import sharded_cases as sc
from test_dist_gloo import _single, _spawn, _worker


def test_shard_arithmetic_every_world_and_population():
    from pathfit.dist import _counts, owner_of, shard_range
    for world in range(1, 17):
        for n in range(0, 201):
            rng = [shard_range(n, r, world) for r in range(world)]
            cn = _counts(n, world)
            assert rng[0][0] == 0 and rng[-1][1] == n
            assert all(rng[r][1] == rng[r + 1][0] for r in range(world - 1))          # contiguous and ordered: they cover [0, n)
            assert cn == [b - a for a, b in rng] and min(cn) >= 0 and max(cn) - min(cn) <= 1 and sum(cn) == n
            assert cn == sorted(cn, reverse=True)                                     # the larger shards come first
            for r, (a, b) in enumerate(rng):
                for g in range(a, b):
                    assert owner_of(g, cn) == (r, g - a), (world, n, g)
            with pytest.raises(IndexError):
                owner_of(n, cn)


def test_case_table_holds_what_the_gpu_cases_need():
    by = {}
    for c in sc.CASES:
        by.setdefault(c["solver"], []).append(c)
        assert c["n"] == sc.POPULATIONS[c["world"]] and sc.counts_of(c) == sc.SPLITS[c["world"]]
    assert len(set(sc.CASE_IDS)) == len(sc.CASES)
    assert sc.SPLITS == {8: [2, 2, 2, 1, 1, 1, 1, 1], 5: [27, 27, 27, 26, 26], 3: [67, 67, 66]}
    assert sc.POPULATIONS == {8: 11, 5: 133, 3: 200}
    for solver in ("maaco", "mpa", "pso", "ga"):
        assert {c["world"] for c in by[solver]} == {3, 5, 8}, solver
    # what the splits are for: one-agent shards; boundaries off every multiple of 8 across three words; shards of two words
    assert sc.SPLITS[8].count(1) == 5
    assert all(b % 8 for b in np.cumsum(sc.SPLITS[5])[:-1]) and -(-133 // 64) == 3
    assert min(sc.SPLITS[3]) > 64
    mc = by["maaco"]
    assert {c["world"] for c in mc if c.get("pack8")} == {3, 5, 8}                    # the packed walk kernel at every population
    assert {c["chunks"] for c in mc} == {3, 7} and sum(c.get("strict", 1) == 0 for c in mc) == 1
    rows = sc.grid()[0].shape[0]
    for k in (3, 7):                                                                  # no chunk bound of the fold is a multiple of 64
        assert all((rows * j // k) * sc.grid()[0].shape[1] % 64 for j in range(1, k))
    assert sc.MPA_ITERS == 6 and sc.MAACO_ITERS == 4 and sc.PSO_SWEEPS == 4 and sc.GA_GENS == 3 and sc.W == 3
    assert any(c.get("sync") for c in by["pso"])


@pytest.mark.parametrize("case", [c for c in sc.CASES if c["solver"] != "ga"], ids=lambda c: c["id"])
def test_a_winner_crosses_a_rank_boundary(case):
    """From the oracle alone: at least once the overall best is taken over from an ant rank 0 does not own (MAACO), the elite lives
    off rank 0 (MPA), the gbest moves to a particle off rank 0 (PSO) -- the row then travels from its owner to every rank."""
    ids, owners = sc.winners(case), sc.winner_owners(case)
    assert ids and all(0 <= g < case["n"] for g in ids)
    assert any(r != 0 for r in owners), (ids, owners)


def test_oracle_runs_are_not_degenerate():
    """The short runs still move: the curves improve, the phases of MPA accept rebuilt paths, the GA's population is no constant."""
    for n in sc.POPULATIONS.values():
        ref, takers = sc.maaco_oracle(n, sc.SEEDS["maaco"][n])
        assert len(ref["curve"]) == sc.MAACO_ITERS and np.isfinite(ref["length"]) and takers
        mo, best, elites = sc.mpa_oracle(n, sc.SEEDS["mpa"][n])
        assert len(mo.curve) == sc.MPA_ITERS + 1 and mo.curve[-1] < mo.curve[0] and len(elites) == sc.MPA_ITERS
        assert sorted(mo.gorder.tolist()) == list(range(n))
        p = sc.pso_oracle(n, sc.SEEDS["pso"][n], False)
        assert len(p["curve"]) == sc.PSO_SWEEPS + 1 and p["curve"][-1] < p["curve"][0] and p["pos"].shape == (n, sc.W, 2)
        res, curve, popfit = sc.ga_oracle(n, sc.SEEDS["ga"][n])
        assert len(curve) == sc.GA_GENS + 1 and curve[-1] < curve[0] and len(popfit) == n and len(set(popfit.tolist())) > 1
        assert res[5] == curve[-1] and list(popfit) == sorted(popfit)


@pytest.mark.parametrize("chunks", [3, 7])
@pytest.mark.parametrize("world", [8, 5, 3])
def test_sharded_maaco_over_the_fakes_at_the_gpu_populations(tmp_path, world, chunks):
    """The CPU twin of the GPU cases: ShardedMAACO over tests/dist_fakes.py at (8 ranks, 11 ants), (5, 133) and (3, 200), the
    ordered fold pipelined over 3 and 7 row chunks, against the one-rank run -- result, curve and pheromone on every rank."""
    ants = sc.POPULATIONS[world]
    port = 23100 + (os.getpid() % 1500) * 2 + (chunks == 7) + 3000 * [8, 5, 3].index(world)
    _spawn(_worker, args=(world, port, str(tmp_path), True, ants, chunks), nprocs=world)
    ref = _single(True, ants)
    for r in range(world):
        z = np.load(tmp_path / f"r{r}.npz")
        assert np.array_equal(z["path"], ref[0]) and float(z["length"]) == ref[1] and float(z["turns"]) == ref[2], r
        assert np.array_equal(z["curve"], ref[4]) and np.array_equal(z["tau"], ref[3]), r


# ---- a world larger than the population -----------------------------------------------------------------------------------------
class _Dist:
    """rank and world size only: any collective is an error"""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def __getattr__(self, name):
        raise AssertionError("collective %s before the population was checked" % name)


class _Engine:
    def __getattr__(self, name):
        raise AssertionError("engine call %s before the population was checked" % name)


def test_world_larger_than_population_is_rejected_up_front():
    """A rank without agents.  The engine calls reject n <= 0, so such a rank would raise in its first launch while the others wait
    for it in a collective.  Before the check in pathfit/dist.py the constructors let it through: ShardedMAACO built a rank with
    counts[rank] = 0 (its walk of 0 ants is the first engine call to refuse); ShardedMPA handed n_local = 0 to pathfit.MPA, which
    reads 0 as "not sharded" and stored all N predators on that rank; ShardedPSO and ShardedGA built the solver and sized its
    buffers for max(n, 1) rows.  Now every rank raises ValueError, naming N and the world size, in the constructor -- the same
    verdict everywhere, before any collective and before any engine call, so no rank is left waiting."""
    from pathfit.dist import Comm, ShardedGA, ShardedMAACO, ShardedMPA, ShardedPSO
    g = sc.grid()[0]

    def no_local(*a):
        raise AssertionError("the local solver was built before the population was checked")
    for world, n in ((8, 7), (3, 2), (2, 1), (5, 0)):
        for rank in range(world):
            comm = Comm(_Dist(rank, world), None)
            makers = {
                "ShardedMAACO": lambda: ShardedMAACO(comm, no_local, n, strict=True, chunks=3),
                "ShardedMPA": lambda: ShardedMPA(comm, no_local, n),
                "ShardedPSO": lambda: ShardedPSO(comm, g, engine=_Engine(), num_particles=n, **sc.PSO_KW),
                "ShardedGA": lambda: ShardedGA(comm, g, engine=_Engine(), population_size=n, **sc.GA_KW),
            }
            for name, make in makers.items():
                with pytest.raises(ValueError, match=r"%s: N = %d agents .* world size of %d ranks" % (name, n, world)):
                    make()
    # world == N is the smallest legal population: one agent on every rank (the constructor gets as far as the local solver)
    with pytest.raises(AssertionError, match="local solver"):
        ShardedMAACO(Comm(_Dist(2, 3), None), no_local, 3)


# ---- the group launcher itself, with trivial ranks ------------------------------------------------------------------------------
def _rank(rank, world, port, out_dir, case):
    """A rank without a GPU: what it does is in case["ranks"][rank]."""
    import signal
    import time
    what = case["ranks"][rank]
    if what == "ok":
        return
    if what == "sleep":                                  # waits to be ended by the parent
        time.sleep(60)
    elif what == "exit3":
        os._exit(3)
    elif what == "segv":
        os.kill(os.getpid(), signal.SIGSEGV)
    elif what == "late_segv":                            # dies on a signal a moment after another rank has failed
        time.sleep(0.15)
        os.kill(os.getpid(), signal.SIGSEGV)
    elif what == "hip":                                  # what a HIP fault looks like from outside: an exception, .err, status 1
        try:
            from pathfit._lib import PathfitError
            raise PathfitError("hipMemcpy: an illegal memory access was encountered")
        except BaseException:
            import traceback
            with open(os.path.join(out_dir, "%s%d.err" % (case["solver"], rank)), "w") as f:
                f.write(traceback.format_exc())
            raise


def _launch(tmp_path, ranks, limit=30.0):
    case = dict(id="launcher", solver="maaco", world=len(ranks), ranks=ranks)
    before = list(sc.stopped)                            # (a real stop of the GPU file, if this process ran it, stays in force)
    del sc.stopped[:]
    try:
        ok, report, wall = sc.run_group(case, tmp_path, limit=limit, target=_rank)
        return ok, report, wall, list(sc.stopped)
    finally:
        sc.stopped[:] = before


def test_launcher_all_ranks_end_well(tmp_path):
    ok, report, wall, stopped = _launch(tmp_path, ["ok", "ok", "ok"])
    assert ok and report == "" and not stopped


def test_launcher_ends_every_rank_at_the_limit_and_stops(tmp_path):
    ok, report, wall, stopped = _launch(tmp_path, ["sleep", "sleep"], limit=1.0)
    assert not ok and wall < 25.0                                    # nobody waited for the sleepers
    assert "rank 0: still running at the 1 s limit" in report and "rank 1: still running at the 1 s limit" in report
    assert len(stopped) == 2 and all("still running" in s for s in stopped)


def test_launcher_reports_every_exit_code_and_ends_the_survivors(tmp_path):
    ok, report, wall, stopped = _launch(tmp_path, ["sleep", "exit3", "sleep"])
    assert not ok and wall < 25.0
    assert "rank 1: exit code 3" in report
    assert "rank 0: ended by the parent after another rank failed" in report and "rank 2: ended by the parent" in report
    assert len(stopped) == 1 and "rank 1: exit code 3" in stopped[0]   # a rank that failed by itself stops the file; the ended ones do not


def test_launcher_a_rank_that_dies_on_a_signal_stops(tmp_path):
    ok, report, wall, stopped = _launch(tmp_path, ["sleep", "segv", "sleep"])
    assert not ok and "rank 1: exit code -11" in report and "rank 2: ended by the parent" in report
    assert len(stopped) == 1 and "exit code -11" in stopped[0]


def test_launcher_a_hip_error_is_status_1_and_stops(tmp_path):
    """A HIP fault reaches Python as PathfitError: the rank writes its .err and exits 1.  That stops the file too."""
    ok, report, wall, stopped = _launch(tmp_path, ["sleep", "hip"])
    assert not ok and "rank 1: exit code 1" in report and "illegal memory access" in report and "PathfitError" in report
    assert len(stopped) == 1 and "rank 1: exit code 1" in stopped[0]


def test_launcher_reads_the_exit_codes_after_the_joins(tmp_path):
    """A second rank that dies by itself a moment after the first is reported and classified by the code it ended with, read
    after the joins: its own signal stops the file, the parent's SIGTERM does not."""
    ok, report, wall, stopped = _launch(tmp_path, ["exit3", "late_segv"])
    assert not ok and "rank 0: exit code 3" in report
    # either the parent's SIGTERM came first (-15: ended by the parent) or the rank's own SIGSEGV did (-11: reported as such)
    assert ("rank 1: exit code -11" in report) != ("rank 1: ended by the parent" in report)
    assert ("exit code -11" in report) == any("exit code -11" in s for s in stopped)
