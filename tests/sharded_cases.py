"""The sharded solvers of pathfit/dist.py at 3, 5 and 8 ranks: the case table, the rank's program, the group launcher and the CPU
oracle runs the assertions rest on.  tests/test_sharded_cases.py checks the table and the CPU facts (no GPU);
tests/test_gpu_sharded_worlds.py runs every case as `world` gloo processes that share GPU 0 (the host-staged transport: the
exchange logic is transport independent, multi-rank RCCL needs one GPU per rank).

All cases run on fig7 (20 x 20, RC = 400): a rank's device work is milliseconds.  The populations are chosen for their splits:

    world 8, N  11: 2,2,2,1,1,1,1,1   shards of one agent -- the owner's local index is 0, a one-row block sits in every gather
    world 5, N 133: 27,27,27,26,26    boundaries 27 / 54 / 81 / 107, none a multiple of 8; the population spans three 64-agent words
    world 3, N 200: 67,67,66          every shard longer than one 64-agent word: two local words, local index != global index mod 64

A winner has to cross a rank boundary at least once in every MAACO, MPA and PSO case (the overall best taken over from an ant rank 0
does not own, the MPA elite, the PSO global best): `winners()` derives the global ids on the CPU, from the oracle alone, and the
seeds of the table were chosen so that one of them lies outside rank 0's block."""
import functools
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "maaco-path-planing_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import golden_io as gio                                                   # noqa: E402

INF = float("inf")
MAP = "fig7"
POPULATIONS = {8: 11, 5: 133, 3: 200}                                     # world -> ants / predators / particles / chromosomes
SPLITS = {8: [2, 2, 2, 1, 1, 1, 1, 1], 5: [27, 27, 27, 26, 26], 3: [67, 67, 66]}
MAACO_ITERS, MPA_ITERS, PSO_SWEEPS, GA_GENS, W = 4, 6, 4, 3, 3            # MPA: two iterations per phase, so all three phases and FADs run
MK = dict(alpha=1.0, beta=2.0, rho=0.1, Q=2.5, a_turn_coef=1.0, wh_max=0.9, wh_min=0.2, k_h_adaptive=0.9, q0_initial=0.5)
PSO_KW = dict(num_iterations=PSO_SWEEPS, num_waypoints_per_particle=W, w=0.7, c1=1.5, c2=1.5, turn_penalty_factor=0.3,
              safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0)
GA_KW = dict(num_generations=GA_GENS, num_waypoints_per_chromosome=W, mutation_rate=0.1, crossover_rate=0.8, tournament_size=3,
             turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0)
SEEDS = {"maaco": {11: 7, 133: 7, 200: 7}, "mpa": {11: 3, 133: 3, 200: 3}, "pso": {11: 6, 133: 6, 200: 6}, "ga": {11: 4, 133: 4, 200: 4}}


def _case(solver, world, **opts):
    n = POPULATIONS[world]
    tag = "".join("-%s%s" % (k, v) for k, v in sorted(opts.items()))
    return dict(id="%s-w%d-n%d%s" % (solver, world, n, tag), solver=solver, world=world, n=n, seed=SEEDS[solver][n], **opts)


def _cases():
    out = []
    # MAACO: chunks 3 and 7 (20 rows: every chunk bound is a non-multiple of 64), each population once more with the packed walk
    # kernel forced (eight ants per wavefront: ant0 != 0 and a local count that is no multiple of 8), one all-reduce run
    for world, chunks in ((8, 3), (5, 7), (3, 3)):
        out.append(_case("maaco", world, chunks=chunks))
        out.append(_case("maaco", world, chunks=10 - chunks, pack8=1))
    out.append(_case("maaco", 5, chunks=3, strict=0))
    for world in (8, 5, 3):
        out.append(_case("mpa", world))
    for world in (8, 5, 3):
        out.append(_case("pso", world))
    out.append(_case("pso", 5, sync=1))                                   # one batch per sweep: the other rule for the improver's rank
    for world in (8, 5, 3):
        out.append(_case("ga", world))
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def grid():
    return gio.grid(MAP)


def counts_of(case):
    from pathfit.dist import _counts
    return _counts(case["n"], case["world"])


# ---- one rank -----------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_dir, case):
    """Rank `rank` of one case: a gloo process group, an engine on GPU 0, the sharded solver; this rank's result and local state go
    to <solver><rank>.npz.  Anything that goes wrong leaves <solver><rank>.err and a non-zero exit status."""
    solver = case["solver"]
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        # An engine sizes its open-list scratch for a whole chip: 8 search slots per CU, 11.4 GB on an MI355X.  Up to eight ranks share
        # one chip here, next to whatever the parent process and the machine's other users hold, and eight such pools did run out of
        # memory inside the whole suite.  One slot per CU (256 slots, 1.4 GB) still gives each of a rank's at most 67 agents a slot of
        # its own; the slot count is a residency knob and never changes a result (README: PF_SLOTS_PER_CU).  Read when the library loads.
        os.environ["PF_SLOTS_PER_CU"] = "1"
        import pathfit
        from pathfit.dist import Comm, ShardedMAACO, ShardedMPA, ShardedPSO, ShardedGA
        g, s, t = grid()
        eng = pathfit.Engine(g, device=0)
        comm = Comm(dist, None)
        n, seed = case["n"], case["seed"]
        if solver == "maaco":
            if case.get("pack8"):
                eng.set_option("maaco_pack8_min", 1)
            try:
                sm = ShardedMAACO(comm, lambda: pathfit.MAACO(g, n, MAACO_ITERS, engine=eng, seed=seed, **MK), n,
                                  strict=bool(case.get("strict", 1)), chunks=case["chunks"])
                path, length, turns = sm.solve_path_planning()
                out = dict(path=np.array(path), length=length, turns=turns, tau=sm.local.pheromone_matrix,
                           curve=np.array(sm.local.convergence_curve_data, float))
            finally:
                eng.set_option("maaco_pack8_min", 2048)
        elif solver == "mpa":
            sm = ShardedMPA(comm, lambda k: pathfit.MPA(g, n, MPA_ITERS, engine=eng, seed=seed, n_local=k), n)
            res = sm.solve_path_planning()
            out = dict(path=np.array(res[0]), stats=np.array(res[1:], float), curve=np.array(sm.local.convergence_curve_data, float))
        elif solver == "pso":
            ps = ShardedPSO(comm, g, engine=eng, seed=seed, num_particles=n, asynchronous=not case.get("sync"), **PSO_KW)
            res = ps.solve()
            out = dict(path=np.array(res[0]), stats=np.array(res[1:], float), curve=np.array(ps.convergence_curve), pos=ps._pos,
                       pbf=ps._pbest_fit)
        else:
            ga = ShardedGA(comm, g, engine=eng, seed=seed, population_size=n, **GA_KW)
            res = ga.solve()
            out = dict(path=np.array(res[0]), stats=np.array(res[1:], float), curve=np.array(ga.convergence_curve),
                       popfit=np.array([p["fitness"] for p in ga.population]))
        np.savez(os.path.join(out_dir, "%s%d.npz" % (solver, rank)), **out)
        dist.barrier(); dist.destroy_process_group()
    except BaseException:
        with open(os.path.join(out_dir, "%s%d.err" % (solver, rank)), "w") as f:
            f.write(traceback.format_exc())
        raise


# ---- one group of `world` ranks -------------------------------------------------------------------------------------------------
# The limit is a hang guard, not a pass criterion.  Measured on an MI355X: the slowest world-8 group (PSO, 11 particles) took 3.4 s of
# wall time from the first start to the last exit, every group between 2.4 and 3.4 s -- process start-up and the torch import dominate
# and vary with load, the device work is milliseconds.  The limit is five times the measurement and no less than 60 s: 60 s.
MEASURED_WORLD8_S = 3.4
GROUP_LIMIT_S = max(60.0, 5.0 * MEASURED_WORLD8_S)
stopped = []                        # why no further group is started (tests/test_gpu_sharded_worlds.py skips on it)


def run_group(case, out_dir, limit=None, target=None):
    """Start the case's `world` ranks as fresh `spawn` interpreters (torch is not imported into this process) and wait for them, at
    most `limit` seconds; as soon as one rank fails, or at the limit, every rank still running is terminated.  -> (ok, report, wall
    seconds): `report` names every rank that did not exit 0, with its exit code as read AFTER the joins (a rank that dies a moment
    after the first one is reported with its own code) and the end of its .err file.

    What goes into `stopped` (nothing more may be started after that): every rank that was still running at the limit, and every
    rank that ended by itself with a non-zero status -- a signal, 134 / 139, and status 1 too: the worker asserts nothing, so an
    exception in a rank is an error on the way, and a HIP fault reaches Python as exactly that (Engine._ck raises PathfitError with
    the text of the HIP error).  Only a rank the parent itself ended after another one had failed (its own SIGTERM / SIGKILL) is
    reported without stopping the file.  `target` replaces the worker (tests/test_sharded_cases.py drives the launcher with
    trivial ranks, no GPU)."""
    import multiprocessing
    limit = GROUP_LIMIT_S if limit is None else limit
    world = case["world"]
    port = 20000 + (os.getpid() % 200) * 40 + (CASE_IDS.index(case["id"]) if case["id"] in CASE_IDS else len(CASE_IDS))
    ctx = multiprocessing.get_context("spawn")
    procs = [ctx.Process(target=target or _worker, args=(r, world, port, str(out_dir), case)) for r in range(world)]
    t0 = time.monotonic()
    for pr in procs:
        pr.start()
    timed_out = False
    ended = set()                                             # the ranks the parent terminated
    try:
        while any(pr.exitcode is None for pr in procs):
            if any(pr.exitcode not in (None, 0) for pr in procs):
                break
            if time.monotonic() - t0 > limit:
                timed_out = True
                break
            time.sleep(0.02)
    finally:
        for r, pr in enumerate(procs):
            if pr.exitcode is None:
                ended.add(r)
                pr.terminate()
        for pr in procs:
            pr.join(10)
            if pr.exitcode is None:
                pr.kill(); pr.join(10)
    wall = time.monotonic() - t0
    report = []
    for r, pr in enumerate(procs):
        code = pr.exitcode                                    # after the joins
        if code == 0:
            continue
        by_parent = r in ended and code in (-15, -9, None)
        err = os.path.join(str(out_dir), "%s%d.err" % (case["solver"], r))
        tail = open(err).read()[-1500:] if os.path.exists(err) else ""
        if by_parent and timed_out:
            what = "still running at the %.0f s limit" % limit
        elif by_parent:
            what = "ended by the parent after another rank failed"
        else:
            what = "exit code %d" % code
        report.append("rank %d: %s\n%s" % (r, what, tail))
        if not by_parent or timed_out:
            stopped.append("%s, rank %d: %s" % (case["id"], r, what))
    return not report, "\n".join(report), wall


def load_ranks(case, out_dir):
    return [np.load(os.path.join(str(out_dir), "%s%d.npz" % (case["solver"], r))) for r in range(case["world"])]


# ---- the CPU oracle runs --------------------------------------------------------------------------------------------------------
class NoEngine:
    """The `engine` of an oracle-backed facade: decode and score come from the oracle, nothing may reach a device."""


def _oracle_backed(cls):
    import pf_oracle as po
    from test_gpu_solvers import _oracle_backed as ob
    g, s, t = grid()
    return ob(cls, po.Oracle(g)), po.Oracle(g), g


@functools.lru_cache(maxsize=None)
def maaco_oracle(n, seed):
    """pf_loops.maaco_solve at this population, and the ants that took the overall best over: the same loop once more through the
    one-rank ShardedMAACO over the oracle-backed stand-ins of tests/dist_fakes.py, whose best-of-iteration scan is watched."""
    import pf_loops, pf_oracle as po
    from dist_fakes import FakeMAACO
    from pathfit.dist import Comm, ShardedMAACO
    g, s, t = grid()
    ref = pf_loops.maaco_solve(po.Oracle(g), s, t, n, MAACO_ITERS, C0=0.1, seed=seed, **MK)
    sm = ShardedMAACO(Comm(None), lambda: FakeMAACO(g, s, t, n, MAACO_ITERS, seed, **MK), n, strict=True)
    m, e = sm.local, sm.local.engine
    scans, takers = [], []
    scan = e.maaco_best_dev
    e.maaco_best_dev = lambda *a: scans.append(scan(*a)) or scans[-1]
    for it in range(1, MAACO_ITERS + 1):
        before = (m.best_path_length_overall, m.best_path_turns_overall, list(map(tuple, m.best_path_overall)))
        sm.step(it)
        if (m.best_path_length_overall, m.best_path_turns_overall, list(map(tuple, m.best_path_overall))) != before:
            takers.append(int(scans[-1][2]))
    C = g.shape[1]
    assert [r * C + c for r, c in m.best_path_overall] == list(ref["path"]) and m.best_path_length_overall == ref["length"]
    assert np.array_equal(e.maaco_get_pheromone(), ref["tau"]) and m.convergence_curve_data == ref["curve"]
    return ref, takers


def _tracked_mpa_oracle():
    import pf_loops

    class Tracked(pf_loops.MpaOracle):
        """MpaOracle that also keeps the list as the sharded solver stores it: gorder[position] = the storage id (= global predator
        id) of the predator at that list position, and the id of the elite of every iteration."""

        def _sort(self):
            if not hasattr(self, "gorder"):
                self.gorder, self.elites = np.arange(self.N), []
            order = np.argsort(np.array([x[1][4] for x in self.pop]), kind="stable")
            self.pop = [self.pop[i] for i in order]
            self.gorder = self.gorder[order]

        def step(self, it, predators=None):
            self._sort()                                   # (MpaOracle.step sorts again: a stable sort of a sorted list)
            self.elites.append(int(self.gorder[0]))
            super().step(it, predators)
    return Tracked


@functools.lru_cache(maxsize=None)
def mpa_oracle(n, seed):
    """-> (MpaOracle after solve(), its best, the global ids of the elites)"""
    import pf_oracle as po
    g, s, t = grid()
    ref = _tracked_mpa_oracle()(po.Oracle(g), s, t, n, MPA_ITERS, seed=seed)
    best = ref.solve()
    return ref, best, list(ref.elites)


@functools.lru_cache(maxsize=None)
def pso_oracle(n, seed, sync):
    """The loop of pso.py:178-231 over the oracle-backed facade (test_gpu_solvers._oracle_backed: the facade's own keyed
    initialisation, decode and score from the oracle).  Asynchronous (the default): particle by particle, each with the gbest the
    particles before it left; synchronous: one batch per sweep on the sweep-start gbest, as test_pso_solve_matches_oracle_loop.
    -> dict(path, stats, curve, pos, pbf, movers): `movers` are the global indices of the particles the gbest moved to."""
    import pathfit
    OB, orc, g = _oracle_backed(pathfit.PSOSolver)
    kw = dict(PSO_KW, num_particles=n, seed=seed, asynchronous=not sync)
    b = OB(g, engine=NoEngine(), **kw)
    assert b._initialize_particles()
    pos, vel, pb, pbf = b._pos.copy(), b._vel.copy(), b._pbest.copy(), b._pbest_fit.copy()
    gd = b.gbest_particle_data
    gb, gfit, gpath = np.array(gd["position"]), gd["fitness"], gd["path"]
    gstats = np.array([gd["length"], gd["turns"], gd["safety_penalty"], gd["diag_penalty"], gd["fitness"]])
    curve, movers = [gfit], []
    for it in range(PSO_SWEEPS):
        if sync:                  # the sweep of tests/test_gpu_solvers.py::test_pso_solve_matches_oracle_loop (its `for it in range(8)` body,
            # lines 215-225), which lives inside that test and cannot be imported: keep the two alike
            pos, vel = orc.pso_update(pos, vel, pb, gb, kw["w"], kw["c1"], kw["c2"], b.max_vel, seed, it, 0)
            cps, stats, feas = b._evaluate(wp_pos=pos)
            imp = feas & (stats[:, 4] < pbf)
            pb[imp] = pos[imp]; pbf[imp] = stats[imp, 4]
            cand = np.flatnonzero(imp)
            if cand.size:
                j = int(cand[np.argmin(stats[cand, 4])])
                if stats[j, 4] < gfit:
                    gfit, gb, gpath, gstats = stats[j, 4], pos[j].copy(), cps[j], stats[j].copy()
                    movers.append(j)
        else:
            for i in range(n):
                p, v = orc.pso_update(pos[i:i + 1], vel[i:i + 1], pb[i:i + 1], gb, kw["w"], kw["c1"], kw["c2"], b.max_vel, seed, it, i)
                pos[i], vel[i] = p[0], v[0]
                cps, stats, feas = b._evaluate(wp_pos=p)
                if feas[0] and stats[0, 4] < pbf[i]:                    # pso.py:216-220
                    pb[i], pbf[i] = p[0], stats[0, 4]
                    if stats[0, 4] < gfit:                               # :222-229
                        gfit, gb, gpath, gstats = stats[0, 4], p[0].copy(), cps[0], stats[0].copy()
                        movers.append(i)
        curve.append(gfit)
    path = gpath.tolist() if hasattr(gpath, "tolist") else gpath
    return dict(path=path, stats=gstats, curve=curve, pos=pos, pbf=pbf, movers=movers)


@functools.lru_cache(maxsize=None)
def ga_oracle(n, seed):
    """The oracle-backed GA facade (test_gpu_solvers._oracle_backed) with no engine at all: the host loop, the native operators,
    decode and score from the oracle.  -> (result tuple, curve, population fitness)"""
    import pathfit
    OB, orc, g = _oracle_backed(pathfit.GASolver)
    b = OB(g, engine=NoEngine(), population_size=n, seed=seed, **GA_KW)
    res = b.solve()
    return res, list(b.convergence_curve), np.array([p["fitness"] for p in b.population])


def winners(case):
    """Global ids of the agents whose row has to travel: the ants that took the overall best over (MAACO), the elite of every
    iteration (MPA), the particles the gbest moved to (PSO).  From the oracle alone."""
    if case["solver"] == "maaco":
        return maaco_oracle(case["n"], case["seed"])[1]
    if case["solver"] == "mpa":
        return mpa_oracle(case["n"], case["seed"])[2]
    if case["solver"] == "pso":
        return pso_oracle(case["n"], case["seed"], bool(case.get("sync")))["movers"]
    return []


def winner_owners(case):
    from pathfit.dist import owner_of
    cn = counts_of(case)
    return [owner_of(gid, cn)[0] for gid in winners(case)]
