"""Every kernel on maps with a side of 1, 2 or 3 cells (tests/thin_maps.py), up to 4096 long: every cell a border cell, maps
narrower than the 3 x 3 neighbourhood and than the safety window, R * C below one wavefront, row / column 4095.  HIP == the CPU
oracle (which tests/test_oracle_thin_grids.py ties to the unmodified reference on these maps) == the reference's own answers in
tests/golden/thin_cases.npz, bit for bit.  Also the decodes that are LONGER than their grid (astar.py:55-56 exempts the goal from
the avoid set, so each of the W + 1 segments may end on a visited cell: up to R * C + W + 1 cells)."""
import numpy as np
import pytest

import golden_io as gio
import thin_maps as tm

pytestmark = pytest.mark.gpu

POLICIES = ((1, 1), (1, 0), (0, 1))      # corner restriction on, off, 4-connected
MAIN_W = (0.3, 0.8, 1.8, 100.0)
WIDE = 20.0                              # a min_safe_distance wider than the short side of every map here (the wide-window EDT)
KEYS = [tm.name_of(*m) for m in tm.all_maps()] + ["2x4096f", "4096x2f"]


def build_map(key):
    if key.endswith("f"):
        R, C = (int(v) for v in key[:-1].split("x"))
        return tm.few_obstacles_map(R, C)
    R, C = (int(v) for v in key[:-1].split("x"))
    return tm.thin_map(R, C, key.endswith("o"))


@pytest.fixture(scope="module")
def gold():
    z = gio.load("thin_cases")
    return z, [str(n) for n in z["grid_names"]]


@pytest.fixture(scope="module", params=KEYS)
def world(request):
    """One engine per shape, and one oracle per move policy."""
    from pathfit.engine import Engine
    import pf_oracle as po
    g, s, t = build_map(request.param)
    e = Engine(g)
    yield dict(key=request.param, g=g, s=s, t=t, e=e, o={p: po.Oracle(g, *p) for p in POLICIES})
    for name in ("astar_settle", "plateau_kernels"):
        e.set_option(name, -1)
    e.close()


def thin_searches(g, seed=0):
    """60 (start, target, avoid list or None): random pairs, nearby pairs, start == target, adjacent cells, end to end, start or
    target on an obstacle, avoid sets that cut the corridor between the two."""
    R, C = g.shape
    rnd = np.random.default_rng(seed)
    flat = g.reshape(-1)
    free, obst = np.flatnonzero(flat != 1), np.flatnonzero(flat == 1)
    coord = (lambda c: c % C) if C >= R else (lambda c: c // C)
    out = []
    for k in range(24):
        s, t = (int(v) for v in rnd.choice(free, 2))
        av = rnd.choice(free, int(rnd.integers(0, max(2, len(free) // 12)) + 1)).astype(np.int32) if k % 3 == 1 else None
        out.append((s, t, av))
    for k in range(8):
        s = int(rnd.choice(free))
        out.append((s, int(rnd.choice(free[np.abs(coord(free) - coord(s)) <= 10])), None))
    for k in range(4):
        s = int(rnd.choice(free))
        out.append((s, s, None if k % 2 else np.array([s], np.int32)))
    for k in range(6):
        s = int(rnd.choice(free))
        nb = free[(np.abs(free // C - s // C) <= 1) & (np.abs(free % C - s % C) <= 1) & (free != s)]
        out.append((s, int(rnd.choice(nb)) if len(nb) else s, None))
    out += [(int(free[0]), int(free[-1]), None), (int(free[-1]), int(free[0]), None), (0, R * C - 1, None), (R * C - 1, 0, None)]
    for k in range(6):
        s, t = (int(v) for v in rnd.choice(free, 2))
        if len(obst):
            s, t = (int(rnd.choice(obst)), t) if k % 2 else (s, int(rnd.choice(obst)))
        out.append((s, t, None))
    for k in range(8):
        s, t = (int(v) for v in rnd.choice(free, 2))
        mid = (coord(s) + coord(t)) // 2
        out.append((s, t, free[coord(free) == mid].astype(np.int32)))
    assert len(out) == 60
    return ([c[0] for c in out], [c[1] for c in out], [c[2] for c in out])


def test_connectors(world):
    """pf_astar_batch, three variants x three move policies x sequential loop / settling engine x plateau kernels off / on."""
    e, g = world["e"], world["g"]
    S, T, A = thin_searches(g)
    cap = g.size
    feasible = 0
    for ad, rs in POLICIES:
        o = world["o"][(ad, rs)]
        want = [[o.astar(s, t, a, v) for s, t, a in zip(S, T, A)] for v in range(3)]
        feasible += sum(len(w[0]) > 1 for w in want[0])
        if world["key"].endswith("f"):                           # 2 x 4096 / 4096 x 2: the run from row / column 0 to 4095 is open
            assert (S[44], T[44], S[45], T[45]) == (0, g.size - 1, g.size - 1, 0)
            assert all(len(want[v][i][0]) >= max(g.shape) for v in range(3) for i in (44, 45))
        for settle in (0, 1):
            e.set_option("astar_settle", settle)
            for plateau in (0, 1):
                e.set_option("plateau_kernels", plateau)
                for v in range(3):
                    paths, st, cnt = e.astar_host(v, S, T, A, path_cap=cap, want_counters=True, allow_diag=ad, restrict_corner=rs)
                    for i, (wp, wst) in enumerate(want[v]):
                        where = (world["key"], ad, rs, settle, plateau, v, i)
                        assert st[i] != 3 and (st[i] == 0) == (len(wp) > 0) and np.array_equal(paths[i], wp), (where, st[i])
                        if len(wp) > 1 and (settle == 0 or v == 1):          # the sequential loop's counters are the reference's
                            assert (cnt[i, 0], cnt[i, 1]) == (wst[0], wst[1]), (where, cnt[i], wst)
    assert feasible > 0


def golden_decodes(gold, key):
    """The reference's decodes of this map: [(kind, weight set, W, waypoints [n][...], paths, stats [n][5])] grouped for a batch."""
    z, names = gold
    if key not in names:
        return []
    gi, groups = names.index(key), {}
    for i in np.flatnonzero(z["dec_grid"] == gi):
        wp = gio.csr_get(z["dec_wp_off"], z["dec_wp"], i)
        kind = int(z["dec_kind"][i])
        W = len(wp) if kind == 0 else len(wp) // 2
        groups.setdefault((kind, int(z["dec_w"][i]), W), []).append((wp, gio.csr_get_delta(z["dec_path_off"], z["dec_path_d"], i), z["dec_stats"][i]))
    return [(k[0], z["dec_weights"][k[1]], k[2], np.array([r[0] for r in rows]), [r[1] for r in rows], np.array([r[2] for r in rows]))
            for k, rows in groups.items()]


def test_decode_and_score(world, gold):
    """pf_decode_batch / pf_decode_batch_multi from cells and from positions, W = 1..5, scored with min_safe_distance 1.8 and 20:
    the reference's goldens of this map, then random chains against the oracle."""
    from pathfit.engine import score_params
    e, g, s, t, o = world["e"], world["g"], world["s"], world["t"], world["o"][(1, 1)]
    R, C = g.shape
    for kind, w, W, wp, want, wstats in golden_decodes(gold, world["key"]):
        sp = score_params(0, True, w[0], w[1], w[2], w[3])
        kw = dict(wp_cells=wp.astype(np.int32)) if kind == 0 else dict(wp_pos=wp.reshape(len(wp), W, 2))
        for ends in ((s, t), (np.full(len(wp), s, np.int32), np.full(len(wp), t, np.int32))):      # one launch's ends, or per agent
            paths, st, stats = e.decode_host(ends[0], ends[1], sp=sp, **kw)
            for i in range(len(wp)):
                assert st[i] == (0 if len(want[i]) else 1) and np.array_equal(paths[i], want[i]), (world["key"], kind, W, i, st[i])
            assert np.array_equal(stats, wstats), (world["key"], kind, W, w[2])
    rnd = np.random.default_rng(11)
    free = np.flatnonzero(g.reshape(-1) != 1)
    got_path = 0
    for W in range(1, 6):
        n = 8
        cells = rnd.choice(free, (n, W)).astype(np.int32)
        cells[rnd.random((n, W)) < 0.08] = int(rnd.integers(0, R * C))
        pos = np.stack([rnd.uniform(-1.5, R + 0.5, (n, W)), rnd.uniform(-1.5, C + 0.5, (n, W))], axis=2)
        pos[0] = np.floor(pos[0]) + 0.5                          # exact .5 ties: round half to even
        pos[1, :, 0], pos[1, :, 1] = -3.0, C + 40.25             # outside the grid: clamped
        pos[2] = np.stack([np.resize(free, W) // C, np.resize(free, W) % C], axis=1) + 0.5
        starts, targets = rnd.choice(free, n).astype(np.int32), rnd.choice(free, n).astype(np.int32)
        for kind, wp in ((0, cells), (1, pos)):
            wc = wp if kind == 0 else np.stack([o.pso_round(p) for p in wp])
            kw = dict(wp_cells=wp) if kind == 0 else dict(wp_pos=wp)
            for ends in ((s, t), (starts, targets)):
                multi = np.ndim(ends[0]) > 0
                want = [o.decode(int(ends[0][a]) if multi else s, int(ends[1][a]) if multi else t, wc[a])[0] for a in range(n)]
                got_path += sum(len(p) > 0 for p in want)
                for ms in (1.8, WIDE):
                    paths, st, stats = e.decode_host(ends[0], ends[1], sp=score_params(0, True, 0.3, 0.8, ms, 100.0),
                                                     path_cap=None if ms == 1.8 else R * C + W + 1, **kw)
                    for a in range(n):
                        where = (world["key"], W, kind, multi, ms, a)
                        assert st[a] == (0 if len(want[a]) else 1) and np.array_equal(paths[a], want[a]), (where, st[a])
                        assert np.array_equal(stats[a], o.score(want[a], 0, 0.3, 0.8, ms, True, 100.0)), where
    assert got_path > 0


@pytest.mark.parametrize("R,C", [(1, 9), (2, 17), (17, 2), (3, 200), (200, 3), (1, 300)])
def test_update_grid_closes_and_reopens_the_corridor(R, C):
    from pathfit.engine import Engine, score_params
    import pf_oracle as po
    g, s, t = tm.thin_map(R, C, False)
    closed = g.copy()
    if C >= R:
        closed[:, C // 2] = 1
    else:
        closed[R // 2, :] = 1
    S, T, A = thin_searches(g, 3)
    e = Engine(g)
    cuts = []
    try:
        for grid in (g, closed, g, closed):
            e.update_grid(grid)
            o = po.Oracle(grid)
            cut = 0
            for v in range(3):
                paths, st = e.astar_host(v, S, T, A, path_cap=R * C)
                for i in range(len(S)):
                    want = o.astar(S[i], T[i], A[i], v)[0]
                    assert st[i] != 3 and np.array_equal(paths[i], want), (R, C, v, i)
                    cut += len(want) == 0
            cuts.append(cut)
            paths, st, stats = e.decode_host(s, t, wp_cells=np.array([[s, t], [t, s]], np.int32), sp=score_params(0, True, *MAIN_W))
            for a, wp in enumerate(([s, t], [t, s])):
                want = o.decode(s, t, wp)[0]
                assert st[a] == (0 if len(want) else 1) and np.array_equal(paths[a], want), (R, C, a, st[a])
                assert np.array_equal(stats[a], o.score(want, 0, *MAIN_W[:3], True, MAIN_W[3])), (R, C, a)
        assert cuts[1] > cuts[0] and cuts[2:] == cuts[:2], cuts  # the wall costs paths, and each state is reproduced
    finally:
        e.close()


MAACO_BASE = dict(alpha=1.0, rho=0.1, Q=2.5, a_turn=1.0, wh_max=0.9, wh_min=0.2, k_h=0.9, q0_initial=0.5, C0=0.1, num_iterations=10)


def maaco_far_target(key, g):
    """On an obstacle map at least 9 long: the last free cell, beyond the zone of dead ends and cut corridors -- walks towards it
    end in pockets (status 1, no deposit), the branch that the walks towards the map's own target almost never take."""
    if not key.endswith("o") or max(g.shape) < 9:
        return None
    return int(np.flatnonzero(g.reshape(-1) != 1)[-1])


def oracle_maaco_loop(o, s, t, P, n_ants, seed):
    """The reference's loop (MAACO.py:340-359) around the oracle's walk and update, 3 iterations -> (tau0, [per iteration])."""
    import pf_oracle as po
    tau, dist = o.maaco_init(s, t, 0.1)
    tau0 = tau.copy()
    want, best_len, best_turns = [], po.INF, po.INF
    for it in range(1, 4):
        walks = [o.maaco_walk(s, t, P, tau, dist, it, seed, ant)[:3] for ant in range(n_ants)]
        ib_len, ib_turns, ib = po.INF, po.INF, -1
        for ant, (p, L, Tn) in enumerate(walks):
            if L < ib_len or (abs(L - ib_len) < 1e-9 and Tn < ib_turns):
                ib_len, ib_turns, ib = L, Tn, ant
        took = ib_len < best_len or (abs(ib_len - best_len) < 1e-9 and ib_turns < best_turns)
        if took:
            best_len, best_turns = ib_len, ib_turns
        o.maaco_update(tau, 0.1, 2.5, [w[0] for w in walks], [w[1] for w in walks], best_len)
        want.append((walks, ib_len, ib_turns, ib, took, best_len, best_turns, tau.copy()))
    return tau0, want


@pytest.mark.parametrize("key", KEYS)
def test_maaco_iterate(key, gold):
    """pf_maaco_iterate, 3 iterations, on every map (on the 4096-long ones a row of the deposit bit matrix spans 64 words and the
    packed walk and the tabu slots meet coordinate 4095): 6 and 70 ants (70 crosses a 64-ant word of the deposit bit matrix),
    eight ants per wavefront and one, load-ahead form off and on, beta 7 and 2 -- every walk, the iteration's answer block and
    the whole pheromone matrix equal the oracle's loop; with 6 ants on the maps the goldens cover, the reference's own walks and
    pheromone too.  On the obstacle maps a second colony (70 ants, beta 2) walks towards the far end of the obstacle zone, so
    that failed walks (status 1, turns -1, no deposit) are compared too: the test asserts that some fail."""
    from pathfit._lib import MaacoParams
    from pathfit.engine import Engine
    import pf_oracle as po
    z, names = gold
    g, s, t = build_map(key)
    R, C = g.shape
    o, e = po.Oracle(g), Engine(g)
    cap = R * C
    far = maaco_far_target(key, g)
    # (goal, beta, ants, seed, index of the reference's run or None): the reference's runs of this map (6 ants), then 6 ants where
    # it has none, 70 ants, and the colony that fails
    colonies = [(t, float(r[1]), 6, int(r[5]), ri) for ri, r in enumerate(z["maaco_runs"]) if names[int(r[0])] == key]
    colonies += [(t, beta, 6, 77, None) for beta in (7.0, 2.0) if not any(c[1] == beta for c in colonies)]
    colonies += [(t, beta, 70, 77, None) for beta in (7.0, 2.0)] + ([(far, 2.0, 70, 78, None)] if far is not None else [])
    failed = {t: 0, far: 0}
    try:
        for goal, beta, n_ants, seed, ri in colonies:
            P = po.MaacoParams(beta=beta, **MAACO_BASE)
            tau0, want = oracle_maaco_loop(o, s, goal, P, n_ants, seed)
            failed[goal] += sum(len(w[0]) == 0 for it in want for w in it[0])
            if ri is not None:                                   # ... is the reference's
                assert np.array_equal(tau0.reshape(R, C), z[f"maaco{ri}_tau0"])
                for it in range(3):
                    assert np.array_equal(want[it][7].reshape(R, C), z[f"maaco{ri}_tau"][it])
                    for ant in range(6):
                        assert np.array_equal(want[it][0][ant][0], gio.csr_get_delta(z[f"maaco{ri}_path_off"], z[f"maaco{ri}_path_d"], it * 6 + ant))
            dc, dl, dp, dt, ds = e.buf((n_ants, cap), np.int32), e.buf(n_ants, np.int32), e.buf(n_ants, np.float64), \
                e.buf(n_ants, np.int32), e.buf(n_ants, np.int32)
            for pack8 in (1, 1 << 30):
                for ahead in (0, 1):
                    e.set_option("maaco_pack8_min", pack8)
                    e.set_option("maaco_load_ahead", ahead)
                    e.maaco_setup(MaacoParams(1.0, beta, 0.1, 2.5, 1.0, 0.9, 0.2, 0.9, 0.5, 0.1, 10, s, goal))
                    assert np.array_equal(e.maaco_get_pheromone().reshape(-1), tau0)
                    bl, bt = po.INF, po.INF
                    for it in range(1, 4):
                        walks, ib_len, ib_turns, ib, took, best_len, best_turns, wtau = want[it - 1]
                        r = e.maaco_iterate(it, seed, 0, n_ants, cap, dc, dl, dp, dt, ds, bl, bt)
                        where = (key, goal, beta, n_ants, pack8, ahead, it)
                        assert r["overflow_agents"] == 0 and not r["skipped"], where
                        cells, lens, plen, turns, st = dc.download(), dl.download(), dp.download(), dt.download(), ds.download()
                        for ant, (p, L, Tn) in enumerate(walks):
                            assert st[ant] == (0 if len(p) else 1) and np.array_equal(cells[ant, :lens[ant]], p), (where, ant)
                            assert plen[ant] == L and turns[ant] == (Tn if len(p) else -1), (where, ant)
                        assert (r["ib_len"], r["took"], r["best_len"]) == (ib_len, took, best_len), (where, r)
                        if ib >= 0:
                            assert (r["ib_turns"], r["ib_idx"], r["best_turns"]) == (ib_turns, ib, best_turns), (where, r)
                        bl, bt = r["best_len"], r["best_turns"]
                        assert np.array_equal(e.maaco_get_pheromone().reshape(-1), wtau), where
        assert far is None or failed[far] > 0, (key, failed)
    finally:
        e.set_option("maaco_pack8_min", 2048)
        e.set_option("maaco_load_ahead", -1)
        e.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("key", ["3x200e", "3x200o", "2x17e", "2x17o"])
def test_mpa_solve(key, fused):
    import pathfit, pf_oracle as po, pf_loops
    g, s, t = build_map(key)
    C = g.shape[1]
    for seed, kw, okw in ((1, {}, {}),
                          (5, dict(FADs_rate=0.5, P_const=0.5, levy_beta=2.0, turn_penalty_factor=0.1, safety_penalty_factor=0.8,
                                   min_safe_distance=1.8, diagonal_obstacle_penalty=100.0),
                           dict(FADs_rate=0.5, P_const=0.5, levy_beta=2.0, w_turn=0.1, w_safe=0.8, min_safe=1.8, diag_pen=100.0))):
        m = pathfit.MPA(g, 16, 6, seed=seed, fused=fused, **kw)
        try:
            got = m.solve_path_planning()
            ref = pf_loops.MpaOracle(po.Oracle(g), s, t, 16, 6, seed=seed, **okw)
            best = ref.solve()
            assert [r * C + c for r, c in got[0]] == list(best[0]) and got[5] == best[1][4], (key, seed)
            assert m.convergence_curve_data == ref.curve
            for a, b in zip(m.population, ref.pop):
                assert np.array_equal(a["path"].cells, b[0]) and a["fitness"] == b[1][4]
        finally:
            m.engine.close()


def oracle_backed(cls, orc):
    """The facade with decode + score from the CPU oracle (as tests/test_gpu_solvers.py does it)."""
    from pathfit.paths import CellPath

    class OB(cls):
        def _evaluate(self, wp_cells=None, wp_pos=None):
            n = len(wp_cells) if wp_cells is not None else len(wp_pos)
            cps, stats, feas = [], np.zeros((n, 5)), np.zeros(n, bool)
            for i in range(n):
                wp = wp_cells[i] if wp_cells is not None else orc.pso_round(wp_pos[i])
                p, _ = orc.decode(self._cell(self.start_node), self._cell(self.target_node), wp)
                sp = self._sp
                stats[i] = orc.score(p, 0, sp.w_turn, sp.w_safe, sp.min_safe, bool(sp.restrict_policy), sp.diag_pen)
                cps.append(CellPath(p, self.cols)); feas[i] = len(p) > 0
            return cps, stats, feas
    return OB


def ga_vs_oracle(g, W, seed):
    import pathfit, pf_oracle as po
    kw = dict(num_generations=5, population_size=16, num_waypoints_per_chromosome=W, mutation_rate=0.2, crossover_rate=0.8,
              tournament_size=3, turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8,
              diagonal_obstacle_penalty_value=100.0, seed=seed)
    a = pathfit.GASolver(g, **kw)
    try:
        ra = a.solve()
        b = oracle_backed(pathfit.GASolver, po.Oracle(g))(g, engine=a.engine, **kw)
        b.device_loop = False                                    # the host loop of ga_solver.py:178-213 around the oracle
        rb = b.solve()
        assert ra == rb and a.convergence_curve == b.convergence_curve
        assert [x["fitness"] for x in a.population] == [x["fitness"] for x in b.population]
        return ra, a
    finally:
        a.engine.close()


def pso_vs_oracle(g, W, seed):
    """PSOSolver.solve (synchronous sweeps) == the same loop around the oracle, as tests/test_gpu_solvers.py runs it on fig7."""
    import pathfit, pf_oracle as po
    orc = po.Oracle(g)
    kw = dict(num_iterations=6, num_particles=16, num_waypoints_per_particle=W, w=0.7, c1=1.5, c2=1.5, turn_penalty_factor=0.3,
              safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0, seed=seed, asynchronous=False)
    a = pathfit.PSOSolver(g, **kw)
    try:
        ra = a.solve()
        b = oracle_backed(pathfit.PSOSolver, orc)(g, engine=a.engine, **kw)
        assert b._initialize_particles()
        pos, vel, pb, pbf = b._pos.copy(), b._vel.copy(), b._pbest.copy(), b._pbest_fit.copy()
        gb, gfit, gpath = np.array(b.gbest_particle_data["position"]), b.gbest_particle_data["fitness"], b.gbest_particle_data["path"]
        curve = [gfit]
        for it in range(6):
            pos, vel = orc.pso_update(pos, vel, pb, gb, 0.7, 1.5, 1.5, b.max_vel, seed, it, 0)
            cps, stats, feas = b._evaluate(wp_pos=pos)
            imp = feas & (stats[:, 4] < pbf)
            pb[imp] = pos[imp]; pbf[imp] = stats[imp, 4]
            cand = np.flatnonzero(imp)
            if cand.size:
                j = cand[np.argmin(stats[cand, 4])]
                if stats[j, 4] < gfit:
                    gfit, gb, gpath = stats[j, 4], pos[j].copy(), cps[j]
            curve.append(gfit)
        assert a.convergence_curve == curve and ra[5] == gfit
        assert ra[0] == (gpath.tolist() if hasattr(gpath, "tolist") else gpath)
        assert np.array_equal(a._pos, pos) and np.array_equal(a._pbest_fit, pbf)
        return ra, a
    finally:
        a.engine.close()


@pytest.mark.parametrize("key", ["2x17e", "2x17o"])
def test_ga_and_pso_solve(key):
    g, s, t = build_map(key)
    ra, _ = ga_vs_oracle(g, 4, 4)
    assert ra[0][0] == (0, 0) and ra[0][-1] == (t // 17, t % 17)
    ra, _ = pso_vs_oracle(g, 4, 6)
    assert ra[0][0] == (0, 0) and ra[0][-1] == (t // 17, t % 17)


# ---- decodes longer than the grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["1x2e", "2x2e"])
def test_long_decode_reference_examples(key, gold):
    """1 x 2, chromosome [(0,1),(0,0),(0,1)] -> 4 cells on 2; 2 x 2, [(0,1),(1,1),(1,0),(0,0),(1,1)] -> 6 cells on 4: the
    reference's paths and stats through decode_host, GASolver and PSOSolver (capacity R * C + W + 1, not R * C)."""
    import pathfit
    from pathfit.engine import Engine, score_params
    z, names = gold
    i = int(z["dec_long"][0 if key == "1x2e" else 1])
    assert names[z["dec_grid"][i]] == key and z["dec_kind"][i] == 0 and z["dec_kind"][i + 1] == 1
    g, s, t = gio.thin_grid(z, key)
    R, C = g.shape
    chrom = gio.csr_get(z["dec_wp_off"], z["dec_wp"], i).astype(np.int32)
    want = gio.csr_get_delta(z["dec_path_off"], z["dec_path_d"], i)
    W = len(chrom)
    assert len(want) > R * C and np.array_equal(want, gio.csr_get_delta(z["dec_path_off"], z["dec_path_d"], i + 1))
    e = Engine(g)
    try:
        sp = score_params(0, True, *MAIN_W)
        pos = gio.csr_get(z["dec_wp_off"], z["dec_wp"], i + 1).reshape(1, W, 2)
        for kw in (dict(wp_cells=chrom[None, :]), dict(wp_pos=pos)):
            for ends in ((s, t), (np.array([s], np.int32), np.array([t], np.int32))):
                paths, st, stats = e.decode_host(ends[0], ends[1], sp=sp, **kw)
                assert st[0] == 0 and np.array_equal(paths[0], want) and np.array_equal(stats[0], z["dec_stats"][i])
        w = dict(turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0)
        rc = [(int(c) // C, int(c) % C) for c in want]
        ga = pathfit.GASolver(g, 1, 2, W, 0.1, 0.8, engine=e, **w)
        assert ga._reconstruct_path_from_chromosome([(int(c) // C, int(c) % C) for c in chrom]) == rc
        ps = pathfit.PSOSolver(g, 1, 2, W, 0.7, 1.5, 1.5, engine=e, **w)
        assert ps._reconstruct_path_from_position(pos[0].tolist()) == rc
    finally:
        e.close()
    # whole solves on the map: with rows of R * C cells the GA / PSO decode raised a capacity overflow
    ra, a = ga_vs_oracle(g, W, 2)
    assert ra[0][0] == (0, 0) and ra[0][-1] == (R - 1, C - 1)
    ra, a = pso_vs_oracle(g, W, 3)
    assert ra[0][0] == (0, 0) and ra[0][-1] == (R - 1, C - 1)


@pytest.mark.parametrize("R,C", [(2, 2), (2, 3), (3, 3)])
def test_long_decode_sweep(R, C):
    """500 random chromosomes, W = 1..5, on an empty map: device == oracle, through the default capacity and through
    decode_retry, and the sweep does contain paths longer than the grid (seed checked on the CPU)."""
    from pathfit.engine import Engine, score_params
    from pathfit.solvers import decode_retry
    import pf_oracle as po
    g, s, t = tm.thin_map(R, C, False)
    o = po.Oracle(g)
    e = Engine(g)
    sp = score_params(0, True, *MAIN_W)
    try:
        rnd = np.random.default_rng(100 * R + C)
        longest = 0
        for W in range(1, 6):
            wp = rnd.integers(0, R * C, (100, W)).astype(np.int32)
            want = [o.decode(s, t, w)[0] for w in wp]
            longest = max(longest, max(len(p) for p in want))
            paths, st, stats = e.decode_host(s, t, wp_cells=wp, sp=sp)
            cps, stats2, feas, launches = decode_retry(e, s, t, R, C, wp_cells=wp, sp=sp)
            assert launches == 1 and np.array_equal(stats, stats2)
            for a in range(100):
                assert st[a] == (0 if len(want[a]) else 1) and np.array_equal(paths[a], want[a]) and np.array_equal(cps[a].cells, want[a]), (W, a)
                assert np.array_equal(stats[a], o.score(want[a], 0, *MAIN_W[:3], True, MAIN_W[3])), (W, a)
        assert longest > R * C, longest
    finally:
        e.close()
