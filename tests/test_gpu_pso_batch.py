"""PSOBatch: K independent PSO swarms in one batched sweep (pf_pso_*_batch around pf_decode_batch_multi).  Every swarm must
equal, bit for bit, a solo run with its seed, start and target -- the reference's golden, a particle-by-particle loop over the
C oracle on the 20 x 20 map, a solo pathfit.PSOSolver everywhere -- in its result tuple, its convergence curve, its gbest
record and every particle's position, velocity, pbest and current path and stats.  All comparisons are exact (== on cells
and indices; bit patterns of the doubles); no swarm and no particle is left out."""
import numpy as np
import pytest

import golden_io as gio
from batch_edge_cases import moved, bits               # noqa: F401  (shared by the batch test files)

pytestmark = pytest.mark.gpu

POLICIES = ((1, 1), (1, 0), (0, 1), (0, 0))          # (allow_diag, restrict_corner), as tests/test_gpu_move_policies.py
# the PSO run of tests/test_e2e_golden.py (seed 6 between the markers of fig7)
PSO_KW = dict(num_iterations=8, num_particles=24, num_waypoints_per_particle=5, w=0.7, c1=1.5, c2=1.5, turn_penalty_factor=0.3,
              safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0)
# free-cell pairs of fig7: tests/test_gpu_ga_batch.py's PAIRS6 (np.random.default_rng(7) over the free cells)
PAIRS6 = [((19, 3), (12, 18)), ((18, 5), (12, 1)), ((4, 10), (17, 0)), ((6, 3), (5, 14)), ((0, 1), (18, 10)), ((16, 15), (2, 4))]
STARTS6 = [(0, 0)] + [p[0] for p in PAIRS6[:5]]
TARGETS6 = [(19, 19)] + [p[1] for p in PAIRS6[:5]]
SEEDS6 = [6, 14, 25, 13, 12, 11]
# Rounds per sweep of the six swarms, counted with the SOLO solver of the parent commit (decode launches per sweep in eng.klog):
# the inputs were chosen so that the swarms' repair rounds are uneven (conditions on the inputs, not measurements).
SOLO_ROUNDS6 = [[1, 2, 1, 2, 1, 1, 3, 1], [1, 1, 2, 4, 1, 2, 1, 1], [1, 1, 1, 3, 1, 2, 1, 1], [3, 2, 2, 2, 3, 1, 2, 1], [1, 1, 1, 1, 1, 1, 1, 1],
                [2, 2, 3, 1, 1, 1, 1, 3]]
INF = float("inf")


def components(g):
    """labels of the free cells' 8-connected components"""
    R, C = g.shape
    lab = -np.ones((R, C), int)
    n = 0
    for r0, c0 in np.argwhere(g != 1):
        if lab[r0, c0] >= 0:
            continue
        lab[r0, c0] = n
        todo = [(int(r0), int(c0))]
        while todo:
            r, c = todo.pop()
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < R and 0 <= cc < C and g[rr, cc] != 1 and lab[rr, cc] < 0:
                        lab[rr, cc] = n
                        todo.append((rr, cc))
        n += 1
    return lab, n


def cellpath(p, cols):
    return [r * cols + c for r, c in (p.tolist() if hasattr(p, "tolist") else p)]


def result_bits(res, cols):
    return (cellpath(res[0], cols), bits([float(v) for v in res[1:]]).tolist())


def gbest_record(g, cols):
    """a gbest dict, exactly: position bits, path cells, the five stats as bit patterns"""
    if not len(g["path"]):
        return (bits(np.array(g["position"], float).reshape(-1)).tolist(), [], bits([g["fitness"]]).tolist())
    return (bits(np.array(g["position"], float).reshape(-1)).tolist(), cellpath(g["path"], cols),
            bits([g["length"], g["turns"], g["safety_penalty"], g["diag_penalty"], g["fitness"]]).tolist())


def particle(x, cols):
    return (bits(np.array(x["position"]).reshape(-1)).tolist(), bits(np.array(x["velocity"]).reshape(-1)).tolist(),
            bits(np.array(x["pbest_position"]).reshape(-1)).tolist(), bits([x["pbest_fitness"], x["current_fitness"]]).tolist(),
            cellpath(x["pbest_path"], cols), cellpath(x["current_path"], cols))


def solo_rows(ps):
    """the solo solver's device rows after finish(): what PSOBatch.device_state(k) must equal, row for row"""
    cols = ps.cols
    return (bits(ps._pos).tolist(), bits(ps._vel).tolist(), bits(ps._pbest).tolist(), bits(ps._pbest_fit).tolist(),
            [cellpath(p, cols) for p in ps._cur_path], bits(np.array(ps._cur_stats)).tolist(), [cellpath(p, cols) for p in ps._pbest_path])


def batch_rows(b, k):
    pos, vel, pb, pbf, cells, lens, stats, pbc, pbl = b.device_state(k)
    n = len(lens)
    return (bits(pos).tolist(), bits(vel).tolist(), bits(pb).tolist(), bits(pbf).tolist(), [cells[i, :lens[i]].tolist() for i in range(n)],
            bits(stats).tolist(), [pbc[i, :pbl[i]].tolist() for i in range(n)])


def solo_run(e, g, s, t, seed, kw, **more):
    """a solo PSOSolver on the moved grid -> (solver, result, rounds per sweep = its decode launches per sweep in eng.klog)"""
    import pathfit
    ps = pathfit.PSOSolver(moved(g, s, t), engine=e, seed=seed, **dict(kw, **more))
    assert ps.begin()
    rounds = []
    for _ in range(ps.num_iterations):
        e.klog = []
        ps.sweep()
        rounds.append(sum(1 for x in e.klog if x[0] == "decode"))
        e.klog = None
    return ps, ps.finish(), rounds


def assert_swarm_equals(b, k, res, ps, ref, tag):
    p, cols = b.swarm(k), b.cols
    assert result_bits(res, cols) == result_bits(ref, cols), (tag, "result tuple")
    assert bits(p.convergence_curve).tolist() == bits(ps.convergence_curve).tolist(), (tag, "curve")
    assert gbest_record(p.gbest_particle_data, cols) == gbest_record(ps.gbest_particle_data, cols), (tag, "gbest record")
    x, y = p.particles, ps.particles
    assert len(x) == len(y) == b.num_particles, tag
    for i in range(len(x)):
        assert particle(x[i], cols) == particle(y[i], cols), (tag, "particle", i)
    for name, u, v in zip(("pos", "vel", "pbest", "pbest_fit", "current paths", "current stats", "pbest paths"), batch_rows(b, k), solo_rows(ps)):
        assert u == v, (tag, "device rows", name)


_fig7 = {}


def fig7_batch():
    """the K = 6 batch of checks 1, 2 and 4 (run once): swarm 0 is the golden's run, 1 - 5 are strangers"""
    if not _fig7:
        import pathfit
        g, _, _ = gio.grid("fig7")
        e = pathfit.Engine(g)
        b = pathfit.PSOBatch(g, seeds=SEEDS6, starts=STARTS6, targets=TARGETS6, engine=e, **PSO_KW)
        res = b.solve()
        _fig7.update(g=g, e=e, b=b, res=res)
    return _fig7


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    if _fig7:
        _fig7["b"].close()
        _fig7["e"].close()
        _fig7.clear()


# --------------------------------------------------------------------------- 1. the reference golden inside a batch, solo runs
def test_swarm_0_reproduces_the_reference_golden_among_strangers():
    """fig7, PSO_KW, K = 6: swarm 0 (markers, seed 6) == pso0_* of tests/golden/e2e.npz, the unmodified reference's run, while
    sharing every launch with five other swarms.  N = 24 is no multiple of 64; the first round's 144 items go through the
    decode's queue, later rounds fall to <= 64 items, where no queue is built."""
    f = fig7_batch()
    z = gio.load("e2e")
    b, res = f["b"], f["res"][0]
    assert [r * 20 + c for r, c in res[0]] == list(z["pso0_path"])
    assert np.array_equal(bits(np.array(res[1:], float)), bits(z["pso0_stats"]))
    assert np.array_equal(bits(b.swarm(0).convergence_curve), bits(z["pso0_curve"]))
    pos, _, _, pbf = b.device_state(0)[:4]
    assert np.array_equal(bits(pos), bits(z["pso0_pos"])) and np.array_equal(bits(pbf), bits(z["pso0_pbest_fit"]))
    # the golden curve shows swarm 0 moving its gbest in sweeps 2, 4 and 7 only (decided on the CPU, from the golden)
    c = z["pso0_curve"]
    assert [i for i in range(1, len(c)) if c[i] != c[i - 1]] == [2, 4, 7]


def test_every_swarm_equals_its_solo_solver_and_the_rounds_are_uneven():
    """Same batch: every swarm == a solo PSOSolver on grid_k in everything (result tuple, curve, gbest record, every particle,
    every device row), and its rounds per sweep are the solo solver's decode launches per sweep -- the expected values were
    counted with the parent commit's solo solver, and are counted again here.  The inputs make the rounds uneven: some sweep has two swarms with different
    rounds, some swarm has a one-round sweep, some swarm a sweep of >= 3 rounds."""
    f = fig7_batch()
    b = f["b"]
    assert b.live == list(range(6))
    want = SOLO_ROUNDS6
    assert any(len({r[s] for r in want}) > 1 for s in range(8)), "no sweep with two swarms of different rounds"
    assert any(1 in r for r in want) and any(max(r) >= 3 for r in want), want
    for k in range(6):
        ps, ref, rounds = solo_run(f["e"], f["g"], STARTS6[k], TARGETS6[k], SEEDS6[k], PSO_KW)
        print("swarm", k, "solo rounds", rounds, "batch rounds", b.swarm(k).rounds)
        assert rounds == want[k], (k, rounds)
        assert b.swarm(k).rounds == want[k], (k, b.swarm(k).rounds)
        assert_swarm_equals(b, k, f["res"][k], ps, ref, k)
        assert (b.swarm(k).start_node, b.swarm(k).target_node, b.swarm(k).seed) == (STARTS6[k], TARGETS6[k], SEEDS6[k])


# --------------------------------------------------------------------------- 2. the sequential loop through the CPU oracle
class _NoEngine:
    """The initialisation needs no device when decode + score come from the oracle."""


def oracle_pso(g, s, t, seed, kw):
    """pso.py:178-231, literally: particle by particle, the gbest moving inside the sweep, no speculation; update, rounding,
    decode and score from the C oracle; the initial swarm from the oracle-backed facade."""
    import pathfit
    import pf_oracle as po
    from pathfit.paths import CellPath
    gk = moved(g, s, t)
    orc = po.Oracle(gk, kw.get("allow_diagonal_moves", True), kw.get("restrict_diagonal_near_obstacle_policy", True))

    def evaluate(self, wp):
        p, _ = orc.decode(self._cell(self.start_node), self._cell(self.target_node), wp)
        sp = self._sp
        return p, orc.score(p, 0, sp.w_turn, sp.w_safe, sp.min_safe, bool(sp.restrict_policy), sp.diag_pen)

    class OB(pathfit.PSOSolver):
        def _evaluate(self, wp_cells=None, wp_pos=None):
            n = len(wp_pos)
            cps, stats, feas = [], np.zeros((n, 5)), np.zeros(n, bool)
            for i in range(n):
                p, stats[i] = evaluate(self, orc.pso_round(wp_pos[i]))
                cps.append(CellPath(p, self.cols)); feas[i] = len(p) > 0
            return cps, stats, feas
    o = OB(gk, engine=_NoEngine(), seed=seed, **kw)
    assert o._initialize_particles()
    pos, vel, pb, pbf = o._pos.copy(), o._vel.copy(), o._pbest.copy(), o._pbest_fit.copy()
    gd = o.gbest_particle_data
    gb, gfit, gpath = np.array(gd["position"]), gd["fitness"], cellpath(gd["path"], o.cols)
    curve = [gfit]
    for it in range(kw["num_iterations"]):
        for a in range(kw["num_particles"]):
            p1, v1 = orc.pso_update(pos[a:a + 1], vel[a:a + 1], pb[a:a + 1], gb, kw["w"], kw["c1"], kw["c2"], o.max_vel, seed, it, a)   # :183-206
            pos[a], vel[a] = p1[0], v1[0]
            path, st = evaluate(o, orc.pso_round(pos[a]))                                                                            # :209-211
            if len(path) and st[4] < pbf[a]:                                                                                           # :216
                pbf[a], pb[a] = st[4], pos[a]
                if st[4] < gfit:                                                                                                       # :222
                    gfit, gb, gpath = st[4], pos[a].copy(), path.tolist()
        curve.append(gfit)
    return curve, pos, pbf, gpath


def test_every_swarm_equals_the_sequential_loop_over_the_oracle():
    """The batch of check 1 == the literal asynchronous loop on the CPU, per swarm: curve, final positions, pbest fitnesses and
    gbest path."""
    f = fig7_batch()
    b = f["b"]
    for k in range(6):
        curve, pos, pbf, gpath = oracle_pso(f["g"], STARTS6[k], TARGETS6[k], SEEDS6[k], PSO_KW)
        assert bits(b.swarm(k).convergence_curve).tolist() == bits(curve).tolist(), (k, "curve")
        got = b.device_state(k)
        assert np.array_equal(bits(got[0]), bits(pos)) and np.array_equal(bits(got[3]), bits(pbf)), (k, "positions / pbest fitness")
        assert cellpath(f["res"][k][0], 20) == gpath, (k, "gbest path")


# --------------------------------------------------------------------------- 3. synchronous mode, move policies
def test_synchronous_mode_is_one_round_per_sweep():
    """The setup of check 1 with asynchronous=False against solo: every swarm, exactly one round per sweep."""
    import pathfit
    f = fig7_batch()
    e, g = f["e"], f["g"]
    b = pathfit.PSOBatch(g, seeds=SEEDS6, starts=STARTS6, targets=TARGETS6, engine=e, asynchronous=False, **PSO_KW)
    res = b.solve()
    for k in range(6):
        ps, ref, rounds = solo_run(e, g, STARTS6[k], TARGETS6[k], SEEDS6[k], PSO_KW, asynchronous=False)
        assert rounds == [1] * 8 and b.swarm(k).rounds == [1] * 8, (k, rounds, b.swarm(k).rounds)
        assert_swarm_equals(b, k, res[k], ps, ref, ("sync", k))
    assert any(bits(b.swarm(k).convergence_curve).tolist() != bits(f["b"].swarm(k).convergence_curve).tolist() or
               batch_rows(b, k) != batch_rows(f["b"], k) for k in range(6)), "the synchronous run equals the asynchronous one: the inputs show nothing"
    b.close()


@pytest.mark.parametrize("ad, rs", POLICIES)
def test_move_policies(ad, rs):
    """K = 3, N = 24, 4 iterations, asynchronous, under each (allow_diagonal_moves, restrict_diagonal_near_obstacle_policy)."""
    import pathfit
    f = fig7_batch()
    e, g = f["e"], f["g"]
    kw = dict(PSO_KW, num_iterations=4, allow_diagonal_moves=bool(ad), restrict_diagonal_near_obstacle_policy=bool(rs))
    b = pathfit.PSOBatch(g, seeds=SEEDS6[:3], starts=STARTS6[:3], targets=TARGETS6[:3], engine=e, **kw)
    res = b.solve()
    for k in range(3):
        ps, ref, rounds = solo_run(e, g, STARTS6[k], TARGETS6[k], SEEDS6[k], kw)
        assert b.swarm(k).rounds == rounds, (ad, rs, k)
        assert_swarm_equals(b, k, res[k], ps, ref, (ad, rs, k))
    b.close()


# --------------------------------------------------------------------------- 4. K = 1, and more than one wavefront per segment
@pytest.mark.parametrize("K, N", [(1, 24), (1, 70), (2, 70)])
def test_one_swarm_and_seventy_particles(K, N):
    """K = 1 (the batch is a solo run with a staging copy) and N = 70 (a scan block's stride loop stays below 256, but a segment
    is more than one wavefront of items and no multiple of one) on fig7 against solo."""
    import pathfit
    f = fig7_batch()
    e, g = f["e"], f["g"]
    kw = dict(PSO_KW, num_iterations=4, num_particles=N)
    b = pathfit.PSOBatch(g, seeds=SEEDS6[:K], starts=STARTS6[:K], targets=TARGETS6[:K], engine=e, **kw)
    res = b.solve()
    assert len(res) == K
    for k in range(K):
        ps, ref, rounds = solo_run(e, g, STARTS6[k], TARGETS6[k], SEEDS6[k], kw)
        assert b.swarm(k).rounds == rounds, (K, N, k)
        assert_swarm_equals(b, k, res[k], ps, ref, (K, N, k))
    b.close()


# --------------------------------------------------------------------------- 5. the bench map, small
def test_bench_map_128():
    """env.bench_grid(128), K = 4, N = 64, W = 5, 3 iterations: swarm 0 between the markers, the others between seeded random
    free cells of the markers' component; against solo, device rows included."""
    import pathfit
    from pathfit import env
    g = env.bench_grid(128)
    s0, t0 = env.find_marker(g, 2, "PSO"), env.find_marker(g, 3, "PSO")
    lab, _ = components(g)
    assert lab[s0] == lab[t0]
    free = np.argwhere(lab == lab[s0])
    rnd = np.random.default_rng(5)
    pairs = [(s0, t0)]
    while len(pairs) < 4:
        i, j = rnd.choice(len(free), 2, replace=False)
        pairs.append((tuple(int(v) for v in free[i]), tuple(int(v) for v in free[j])))
    starts, targets, seeds = [p[0] for p in pairs], [p[1] for p in pairs], [50, 51, 52, 53]
    kw = dict(PSO_KW, num_iterations=3, num_particles=64)
    e = pathfit.Engine(g)
    try:
        b = pathfit.PSOBatch(g, seeds=seeds, starts=starts, targets=targets, engine=e, **kw)
        res = b.solve()
        assert b.live == [0, 1, 2, 3]
        for k in range(4):
            ps, ref, rounds = solo_run(e, g, starts[k], targets[k], seeds[k], kw)
            assert b.swarm(k).rounds == rounds, k
            assert_swarm_equals(b, k, res[k], ps, ref, ("G128", k))
        b.close()
    finally:
        e.close()


# --------------------------------------------------------------------------- 6. a degenerate swarm inside a batch
def test_degenerate_swarm_inside_a_batch():
    """The 12 x 12 serpentine map of tests/golden/e2e_pso_fallback.npz (none of the 20 N random particles decodes: pso.py:126-143)
    with its parameters as swarm 0, a second swarm with another seed the other way round: swarm 0 == the reference's golden, both
    swarms are reported and equal their solo runs."""
    import pathfit
    from pathfit import env
    z = gio.load("e2e_pso_fallback")
    g = z["grid"].astype(np.int64)
    C = g.shape[1]
    s, t = env.find_marker(g, 2, "PSO"), env.find_marker(g, 3, "PSO")
    kw = dict(PSO_KW, num_iterations=4, num_particles=4)
    e = pathfit.Engine(g)
    try:
        b = pathfit.PSOBatch(g, seeds=[21, 22], starts=[s, t], targets=[t, s], engine=e, **kw)
        res = b.solve()
        assert len(res) == 2 and 0 not in b.live
        assert [r * C + c for r, c in res[0][0]] == list(z["path"]) and np.array_equal(bits(np.array(res[0][1:], float)), bits(z["stats"]))
        assert np.array_equal(bits(b.swarm(0).convergence_curve), bits(z["curve"]))
        p0 = b.swarm(0).particles
        assert np.array_equal(bits(np.array([x["position"] for x in p0])), bits(z["pos"]))
        assert np.array_equal(bits([x["pbest_fitness"] for x in p0]), bits(z["pbest_fit"]))
        for k, (sk, tk, seed) in enumerate(((s, t, 21), (t, s, 22))):
            ps = pathfit.PSOSolver(moved(g, sk, tk), engine=e, seed=seed, **kw)
            ref = ps.solve()
            p = b.swarm(k)
            assert result_bits(res[k], C) == result_bits(ref, C) and result_bits(p.result(), C) == result_bits(ref, C), k
            assert bits(p.convergence_curve).tolist() == bits(ps.convergence_curve).tolist(), k
            assert gbest_record(p.gbest_particle_data, C) == gbest_record(ps.gbest_particle_data, C), k
            assert [particle(x, C) for x in p.particles] == [particle(x, C) for x in ps.particles], k
        b.close()
    finally:
        e.close()


def test_degenerate_swarm_between_two_batched_swarms():
    """A 12 x 12 map with a walled-off free cell as the target of the MIDDLE swarm of three: that swarm is degenerate (no attempt
    decodes and there is no direct path -> ([], inf, 0, 0.0, 0.0, inf), run by the solo class), swarms 0 and 2 run batched as live
    swarms 0 and 1 -- the live index differs from the swarm index for swarm 2, with its own seed, start and target.  Both equal
    their solo runs bit for bit after begin() and after every sweep (device rows, curve, gbest record, rounds), and sweep()
    returns K values in swarm order."""
    import pathfit
    g = np.zeros((12, 12), int)
    g[3:8, 5] = 1
    g[8:11, 8:11] = 1
    g[9, 9] = 0                                                        # free, enclosed
    kw = dict(PSO_KW, num_iterations=4, num_particles=8, num_waypoints_per_particle=3)
    starts, targets, seeds = [(0, 0), (0, 0), (11, 0)], [(11, 11), (9, 9), (0, 11)], [1, 2, 3]
    e = pathfit.Engine(g)
    try:
        solo = {}
        for k in (0, 2):                                               # a solo run with num_iterations = i IS the first i sweeps
            for its in range(5):
                ps, ref, rounds = solo_run(e, g, starts[k], targets[k], seeds[k], dict(kw, num_iterations=its))
                solo[k, its] = (solo_rows(ps), bits(ps.convergence_curve).tolist(), gbest_record(ps.gbest_particle_data, 12), rounds,
                                result_bits(ref, 12))
        ps1 = pathfit.PSOSolver(moved(g, starts[1], targets[1]), engine=e, seed=seeds[1], **kw)
        ref1 = ps1.solve()
        assert ref1 == ([], INF, 0, 0.0, 0.0, INF)
        b = pathfit.PSOBatch(g, seeds=seeds, starts=starts, targets=targets, engine=e, **kw)
        b.begin()
        assert b.live == [0, 2]
        for its in range(5):
            if its:
                out = b.sweep()
                assert len(out) == 3 and out[1] == INF, out
                assert bits([out[0], out[2]]).tolist() == [solo[0, its][1][-1], solo[2, its][1][-1]], (its, out)
            for k in (0, 2):
                p = b.swarm(k)
                got = (batch_rows(b, k), bits(p.convergence_curve).tolist(), gbest_record(p.gbest_particle_data, 12), p.rounds,
                       result_bits(p.result(), 12))
                for name, u, v in zip(("device rows", "curve", "gbest record", "rounds", "result"), got, solo[k, its]):
                    assert u == v, (k, its, name)
        assert any(max(solo[k, 4][3]) > 1 for k in (0, 2)), "no repair round in either live swarm: the inputs show nothing"
        assert solo[0, 4][0] != solo[2, 4][0]
        p1 = b.swarm(1)
        assert p1.result() == ref1 and p1.convergence_curve == ps1.convergence_curve and p1.rounds == []
        assert gbest_record(p1.gbest_particle_data, 12) == gbest_record(ps1.gbest_particle_data, 12)
        assert len(p1.particles) == len(ps1.particles)
        with pytest.raises(ValueError, match="^PSOBatch: swarm 1 is degenerate"):
            b.device_state(1)                                          # (a degenerate swarm has no rows in the batch)
        b.close()
    finally:
        e.close()


# --------------------------------------------------------------------------- 7. traffic and isolation
def test_sweeps_keep_everything_in_hbm_and_a_round_costs_the_same_for_any_K(monkeypatch):
    """Per round the host-bound copies are the K scan records (ONE copy of 16 K bytes: 96 B at K = 6, a small copy; the library
    counts a copy above 128 B as bulk, so from K = 9 on this one read per round is a bulk copy of 16 K bytes), the
    decode's counter block and its range flag -- three small copies, no bulk copy; and a round is one decode launch whatever K
    is: a sweep of K = 2 and a sweep of K = 6 both log max_k rounds(k) decode launches."""
    import pathfit
    f = fig7_batch()
    e, g = f["e"], f["g"]
    calls = []

    def counted(name):
        fn = getattr(e, name)
        monkeypatch.setattr(e, name, lambda *a, **k: (calls.append(name), fn(*a, **k))[1])
    for name in ("pso_update_batch", "decode_multi", "pso_scan_batch", "pso_commit_batch"):
        counted(name)
    for K in (2, 6):
        b = pathfit.PSOBatch(g, seeds=SEEDS6[:K], starts=STARTS6[:K], targets=TARGETS6[:K], engine=e, **PSO_KW)
        b.begin()
        for it in range(PSO_KW["num_iterations"]):
            c0 = e.d2h_counts()
            e.klog = []
            calls.clear()
            b.sweep()
            launches = [x[0] for x in e.klog]
            e.klog = None
            c1 = e.d2h_counts()
            rounds = max(b.swarm(k).rounds[it] for k in range(K))
            # every entry is one launch of its kernel: one update, one decode, one scan and one commit per round, whatever K is
            assert calls == ["pso_update_batch", "decode_multi", "pso_scan_batch", "pso_commit_batch"] * rounds, (K, it, calls)
            assert rounds == max(SOLO_ROUNDS6[k][it] for k in range(K))
            assert launches == ["decode"] * rounds, (K, it, launches)
            assert c1[1] - c0[1] == 0 and c1[2] - c0[2] == 0, (K, it, c0, c1)
            assert c1[0] - c0[0] == 3 * rounds, (K, it, c0, c1)
        # the gbest record is read only when somebody asks for it: four reads (position, length, path row, stats), then none
        c0 = e.d2h_counts()
        moved_ = [k for k in range(K) if b.swarm(k)._gdev is not None]
        for _ in range(2):
            for k in range(K):
                b.swarm(k).gbest_particle_data
        c1 = e.d2h_counts()
        assert moved_ and sum(c1[:2]) - sum(c0[:2]) == 4 * len(moved_), (K, c0, c1, moved_)
        b.close()


def test_neighbours_on_the_same_engine_and_close():
    """A solo PSOSolver and a GABatch stepped on the same Engine BETWEEN two sweeps of a PSOBatch change nothing in either;
    close() twice is harmless; a closed batch raises PathfitError."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    ga_kw = dict(num_generations=3, population_size=24, num_waypoints_per_chromosome=5, mutation_rate=0.1, crossover_rate=0.8)

    def neighbours(e):
        ps = pathfit.PSOSolver(g, engine=e, seed=9, **PSO_KW)
        assert ps.begin()
        gb = pathfit.GABatch(g, seeds=[5, 6], starts=STARTS6[1:3], targets=TARGETS6[1:3], engine=e, **ga_kw)
        gb.begin()
        return ps, gb

    def step(ps, gb, it):
        ps.sweep()
        gb.step(it)

    def state(ps, gb):
        ps._download_state()
        return (solo_rows(ps), bits(ps.convergence_curve).tolist(), gbest_record(ps.gbest_particle_data, 20),
                [[x.tolist() for x in gb.device_state(k)[:2]] + [bits(gb.device_state(k)[2]).tolist()] for k in range(2)],
                [bits(gb.population(k).convergence_curve).tolist() for k in range(2)])

    def batch_state(b):
        return [(batch_rows(b, k), bits(b.swarm(k).convergence_curve).tolist(), gbest_record(b.swarm(k).gbest_particle_data, 20)) for k in range(3)]
    e0 = pathfit.Engine(g)
    ps, gb = neighbours(e0)
    for it in range(2):
        step(ps, gb, it)
    alone = state(ps, gb)
    b0 = pathfit.PSOBatch(g, seeds=SEEDS6[:3], starts=STARTS6[:3], targets=TARGETS6[:3], engine=e0, **PSO_KW)
    b0.begin()
    for _ in range(3):
        b0.sweep()
    batch_alone = batch_state(b0)
    e0.close()
    e = pathfit.Engine(g)
    try:
        ps, gb = neighbours(e)
        b = pathfit.PSOBatch(g, seeds=SEEDS6[:3], starts=STARTS6[:3], targets=TARGETS6[:3], engine=e, **PSO_KW)
        b.begin()
        b.sweep()
        step(ps, gb, 0)
        b.sweep()
        step(ps, gb, 1)
        b.sweep()
        assert state(ps, gb) == alone
        assert batch_state(b) == batch_alone
        b.close()
        b.close()
        for use in (b.begin, b.sweep, lambda: b.device_state(0), lambda: b.swarm(0).particles):
            with pytest.raises(pathfit.PathfitError, match="closed"):
                use()
        b2 = pathfit.PSOBatch(g, seeds=SEEDS6[:3], starts=STARTS6[:3], targets=TARGETS6[:3], engine=e, **PSO_KW)
        b2.begin()
    finally:
        e.close()
    with pytest.raises(pathfit.PathfitError, match="closed"):
        b2.sweep()
    b2.close()


def test_unbegun_batch_raises():
    import pathfit
    f = fig7_batch()
    b = pathfit.PSOBatch(f["g"], seeds=[1], engine=f["e"], **PSO_KW)
    with pytest.raises(pathfit.PathfitError, match="begin\\(\\) has not run"):
        b.sweep()
    b.begin()
    with pytest.raises(pathfit.PathfitError, match="already run"):
        b.begin()
    b.close()
