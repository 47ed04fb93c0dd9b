"""GABatch: K independent GA populations in one batched generation, and the per-agent-endpoint decode under it
(pf_decode_batch_multi).  Every population must equal, bit for bit, a solo run with its seed, start and target -- the
reference's golden, the oracle-backed host loop on the 20 x 20 map, a solo pathfit.GASolver on the bench maps -- in its result
tuple, its best individual, its convergence curve and its whole final population in order.  All comparisons are exact (== on
cells, ids and orders; bit patterns of the doubles); no population and no individual is left out."""
import numpy as np
import pytest

import golden_io as gio
from batch_edge_cases import free_pairs, moved, bits               # noqa: F401  (shared by the batch test files)

pytestmark = pytest.mark.gpu

POLICIES = ((1, 1), (1, 0), (0, 1), (0, 0))          # (allow_diag, restrict_corner), as tests/test_gpu_move_policies.py
GA_KW = dict(num_generations=6, population_size=24, num_waypoints_per_chromosome=5, mutation_rate=0.1, crossover_rate=0.8,
             tournament_size=3, turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8,
             diagonal_obstacle_penalty_value=100.0)
PAIRS6 = [((19, 3), (12, 18)), ((18, 5), (12, 1)), ((4, 10), (17, 0)), ((6, 3), (5, 14)), ((0, 1), (18, 10)), ((16, 15), (2, 4))]
INF = float("inf")


def components(g):
    """labels of the free cells' 8-connected components (the most permissive policy: cells in different ones are apart under all)"""
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


# --------------------------------------------------------------------------- 1. the multi-endpoint decode alone
def _grid(name):
    from pathfit import env
    return env.bench_grid(128) if name == "G128" else gio.grid("fig7")[0]


def _decode_case(name, seed, n=512, npairs=24, W=4):
    """n agents on `npairs` distinct (start, target) pairs of free cells: some pairs with start == target, some across
    components (if the map has more than one), random waypoints of which some lie on obstacles; and the positions form."""
    g = np.asarray(_grid(name))
    R, C = g.shape
    rnd = np.random.default_rng(seed)
    free = np.flatnonzero(g.reshape(-1) != 1)
    lab, ncomp = components(g)
    pairs = [(int(a), int(b)) for a, b in rnd.choice(free, (npairs, 2))]
    pairs[0] = (pairs[0][0], pairs[0][0])                              # start == target
    pairs[1] = (pairs[1][1], pairs[1][1])
    if ncomp > 1:                                                      # a pair across two components
        flat = lab.reshape(-1)
        a = int(free[0])
        b = int(next(c for c in free if flat[c] != flat[a]))
        pairs[2] = (a, b)
    assert len(set(pairs)) == npairs
    which = rnd.integers(0, npairs, n)
    which[:npairs] = np.arange(npairs)                                 # every pair is used
    wp = rnd.choice(free, (n, W)).astype(np.int32)
    on_obst = rnd.random((n, W)) < 0.04                                # ~15 % of the agents have a waypoint on an obstacle
    obst = np.flatnonzero(g.reshape(-1) == 1)
    wp[on_obst] = rnd.choice(obst, int(on_obst.sum()))
    pos = np.stack([wp // C, wp % C], axis=-1).astype(np.float64) + rnd.uniform(-0.5, 0.5, (n, W, 2))
    ties = rnd.random((n, W, 2)) < 0.15
    pos[ties] = np.floor(pos[ties]) + 0.5                              # x.5: round-half-even
    far = rnd.random((n, W, 2)) < 0.03
    pos[far] = rnd.choice([-3.7, -0.5, R + 2.5, 1e6], int(far.sum()))  # out of range: clamped (pso.py:69-70)
    return g, pairs, which, wp, pos


def _rounded(pos, R, C):
    r = np.clip(np.rint(pos[..., 0]), 0, R - 1).astype(np.int64)
    c = np.clip(np.rint(pos[..., 1]), 0, C - 1).astype(np.int64)
    return (r * C + c).astype(np.int32)


@pytest.mark.parametrize("name", ["G128", "fig7"])
def test_multi_endpoint_decode_equals_solo_decode_and_oracle(name):
    """pf_decode_batch_multi == pf_decode_batch called per distinct pair == the C oracle's decode + score, for every agent:
    cells, length, status and the five stats; both waypoint encodings, with and without scoring, all four move policies."""
    import pf_oracle as po
    from pathfit.engine import Engine, score_params
    from pathfit import PathfitError
    g, pairs, which, wp, pos = _decode_case(name, 31 if name == "G128" else 32)
    R, C = g.shape
    n = len(which)
    starts = np.array([pairs[w][0] for w in which], np.int32)
    targets = np.array([pairs[w][1] for w in which], np.int32)
    e = Engine(g)
    try:
        cap = R * C
        for ad, rs in POLICIES:
            o = po.Oracle(g, ad, rs)
            sp = score_params(0, rs, 0.3, 0.8, 1.8, 100.0)
            for enc in ("cells", "pos"):
                kw = dict(wp_cells=wp) if enc == "cells" else dict(wp_pos=pos)
                cells_of_agent = wp if enc == "cells" else _rounded(pos, R, C)
                for scored in (True, False):
                    paths, st, stats = e.decode_multi_host(starts, targets, sp=sp if scored else None, path_cap=cap, allow_diag=ad,
                                                           restrict_corner=rs, **kw)
                    assert stats is not None if scored else stats is None
                    feas = 0
                    for pi, (s, t) in enumerate(pairs):                # one solo call per distinct pair
                        ids = np.flatnonzero(which == pi)
                        sub = dict(wp_cells=wp[ids]) if enc == "cells" else dict(wp_pos=pos[ids])
                        p1, st1, stats1 = e.decode_host(s, t, sp=sp if scored else None, path_cap=cap, allow_diag=ad, restrict_corner=rs, **sub)
                        for j, a in enumerate(ids):
                            tag = (name, ad, rs, enc, scored, int(a))
                            assert np.array_equal(paths[a], p1[j]) and st[a] == st1[j], tag
                            if scored:
                                assert np.array_equal(bits(stats[a]), bits(stats1[j])), tag
                                want, _ = o.decode(s, t, cells_of_agent[a])
                                assert np.array_equal(paths[a], want) and st[a] == (0 if len(want) else 1), tag
                                assert np.array_equal(bits(stats[a]), bits(o.score(want, 0, 0.3, 0.8, 1.8, rs, 100.0))), tag
                            feas += len(paths[a]) > 0
                    assert feas >= n // 8, (name, ad, rs, enc, feas)
        # all agents on ONE pair: the new entry equals pf_decode_batch on the same inputs, work counters included (sequential loop)
        e.set_option("astar_settle", 0)
        s, t = pairs[5]
        for ad, rs in POLICIES:
            sp = score_params(0, rs, 0.3, 0.8, 1.8, 100.0)
            a = e.decode_host(s, t, wp_cells=wp, sp=sp, path_cap=cap, allow_diag=ad, restrict_corner=rs)
            ca = e.counters()
            b = e.decode_multi_host(np.full(n, s, np.int32), np.full(n, t, np.int32), wp_cells=wp, sp=sp, path_cap=cap, allow_diag=ad,
                                    restrict_corner=rs)
            cb = e.counters()
            assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])
            assert np.array_equal(bits(a[2]), bits(b[2]))
            for key in ("pops", "pushes", "nbr_examined", "path_cells", "overflow_agents"):
                assert ca[key] == cb[key], (ad, rs, key, ca[key], cb[key])
            assert ca["pops"] > 0
        e.set_option("astar_settle", -1)
        # an endpoint outside the grid is an argument error, found before the launch -- for small and for queued batches
        for m in (8, n):
            for bad in (R * C, -1, 1 << 30):
                s2 = starts[:m].copy()
                s2[m // 2] = bad
                with pytest.raises(PathfitError, match="outside the grid"):
                    e.decode_multi_host(s2, targets[:m], wp_cells=wp[:m], sp=None, path_cap=cap)
                with pytest.raises(PathfitError, match="outside the grid"):
                    e.decode_multi_host(targets[:m], s2, wp_cells=wp[:m], sp=None, path_cap=cap)
        # ... and the engine is fine afterwards
        p2, st2, _ = e.decode_multi_host(starts[:8], targets[:8], wp_cells=wp[:8], sp=None, path_cap=cap)
        assert len(p2) == 8 and not (st2 == 3).any()
    finally:
        e.close()


# --------------------------------------------------------------------------- the CPU reference: GASolver's host loop on the oracle
class _NoEngine:
    """The GA host logic needs no device when decode + score come from the oracle."""


def oracle_ga(g, s, t, seed, **kw):
    """GASolver on grid g moved to (s, t), its _evaluate served by the C oracle; records what each evaluation did."""
    import pathfit
    import pf_oracle as po
    from pathfit.paths import CellPath
    gk = moved(g, s, t)
    orc = po.Oracle(gk)

    class OB(pathfit.GASolver):
        in_init = False
        init_calls, gen_calls = [], []

        def _initialize_population(self):
            self.in_init, self.init_calls, self.gen_calls = True, [], []
            try:
                return super()._initialize_population()
            finally:
                self.in_init = False

        def _evaluate(self, wp_cells=None, wp_pos=None):
            n = len(wp_cells)
            cps, stats, feas = [], np.zeros((n, 5)), np.zeros(n, bool)
            for i in range(n):
                p, _ = orc.decode(self._cell(self.start_node), self._cell(self.target_node), wp_cells[i])
                sp = self._sp
                stats[i] = orc.score(p, 0, sp.w_turn, sp.w_safe, sp.min_safe, bool(sp.restrict_policy), sp.diag_pen)
                cps.append(CellPath(p, self.cols)); feas[i] = len(p) > 0
            (self.init_calls if self.in_init else self.gen_calls).append((n, int(feas.sum())))
            return cps, stats, feas
    ga = OB(gk, engine=_NoEngine(), seed=seed, **kw)
    res = ga.solve()
    return ga, res


def cellpath(p, cols):
    return [r * cols + c for r, c in (p.tolist() if hasattr(p, "tolist") else p)]


def individual(x, cols):
    """an individual dict, exactly: chromosome cells, path cells, the five stats as bit patterns"""
    return ([r * cols + c for r, c in x["chromosome"]], cellpath(x["path"], cols),
            bits([x["length"], x["turns"], x["safety_penalty"], x["diag_penalty"], x["fitness"]]).tolist())


def result_bits(res, cols):
    return (cellpath(res[0], cols), bits([float(v) for v in res[1:]]).tolist())


def assert_population_equals(p, res, ga, ref_res, cols, tag):
    assert result_bits(res, cols) == result_bits(ref_res, cols), (tag, "result tuple")
    assert individual(p.best_solution_overall, cols) == individual(ga.best_solution_overall, cols), (tag, "best individual")
    assert bits(p.convergence_curve).tolist() == bits(ga.convergence_curve).tolist(), (tag, "curve")
    a, b = p.population, ga.population
    assert len(a) == len(b), tag
    for i, (x, y) in enumerate(zip(a, b)):
        assert individual(x, cols) == individual(y, cols), (tag, "final population, position", i)


_fig7 = {}


def fig7_batch():
    """the K = 6 batch of checks 2 and 3 (run once): population 0 is the golden's run, 1 - 5 are strangers"""
    if not _fig7:
        import pathfit
        g, _, _ = gio.grid("fig7")
        assert free_pairs(g, 6, 7) == PAIRS6
        starts = [(0, 0)] + [p[0] for p in PAIRS6[:5]]
        targets = [(19, 19)] + [p[1] for p in PAIRS6[:5]]
        seeds = [4, 11, 12, 13, 14, 15]
        b = pathfit.GABatch(g, seeds=seeds, starts=starts, targets=targets, **GA_KW)
        res = b.solve()
        _fig7.update(g=g, b=b, res=res, starts=starts, targets=targets, seeds=seeds)
    return _fig7


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    if _fig7:
        _fig7["b"].close()
        _fig7["b"].engine.close()
        _fig7.clear()


def test_population_0_reproduces_the_reference_golden_among_strangers():
    """fig7, GA_KW, K = 6: population 0 (markers, seed 4) == ga0_* of tests/golden/e2e.npz, the unmodified reference's run,
    while sharing every launch with five other populations."""
    f = fig7_batch()
    z = gio.load("e2e")
    p, res = f["b"].population(0), f["res"][0]
    assert [r * 20 + c for r, c in res[0]] == list(z["ga0_path"])
    assert np.array_equal(bits(np.array(res[1:], float)), bits(z["ga0_stats"]))
    assert np.array_equal(bits(p.convergence_curve), bits(z["ga0_curve"]))
    assert np.array_equal(bits([x["fitness"] for x in p.population]), bits(z["ga0_pop_fitness"]))
    assert res[5] == 36.9184502021829


def test_every_population_equals_the_oracle_backed_host_loop():
    """Same batch: every population == GASolver's host loop with decode + score from the C oracle on grid_k (result tuple, best
    individual, curve, final population).  The CPU run also says what the inputs exercise, per population: children that fell
    back to a parent (ga_solver.py:204-205), generations that improved the best, generations that did not -- each must be >= 1
    for EVERY population (conditions on the inputs, decided on the CPU)."""
    f = fig7_batch()
    N, G = GA_KW["population_size"], GA_KW["num_generations"]
    seen = []
    for k in range(6):
        ga, ref = oracle_ga(f["g"], f["starts"][k], f["targets"][k], f["seeds"][k], **GA_KW)
        fallbacks = sum(n - ok for n, ok in ga.gen_calls)
        c = ga.convergence_curve
        improved = sum(c[i + 1] < c[i] for i in range(G))
        flat = G - improved
        infeasible = sum(n - ok for n, ok in ga.init_calls)
        seen.append((fallbacks, improved, flat, infeasible))
        assert len(ga.gen_calls) == G and all(n == N for n, _ in ga.gen_calls) and len(c) == G + 1
        assert fallbacks >= 1 and improved >= 1 and flat >= 1, (k, seen[-1])
        assert_population_equals(f["b"].population(k), f["res"][k], ga, ref, 20, k)
        assert f["b"].population(k).attempts == sum(n for n, _ in ga.init_calls)
    print("per population (fallback children, improving generations, flat generations, infeasible initial attempts):", seen)


def test_uneven_initialisation_rounds():
    """fig7, N = 40, 2 generations, K = 6: populations 0, 2 and 5 need a second round of attempts (144 in all), 1, 3 and 4 are
    complete after the first 80 -- the second multi-endpoint launch of begin() carries three populations only, with attempt
    indices that continue at 80.  All six equal their oracle-backed CPU runs."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    kw = dict(GA_KW, population_size=40, num_generations=2)
    seeds = [21, 22, 23, 21, 22, 23]
    starts, targets = [p[0] for p in PAIRS6], [p[1] for p in PAIRS6]
    refs = [oracle_ga(g, starts[k], targets[k], seeds[k], **kw) for k in range(6)]
    attempts = [sum(n for n, _ in ga.init_calls) for ga, _ in refs]
    assert attempts == [144, 80, 144, 80, 80, 144], attempts              # the 3 / 3 split, from the CPU runs
    e = pathfit.Engine(g)
    try:
        b = pathfit.GABatch(g, seeds=seeds, starts=starts, targets=targets, engine=e, **kw)
        res = b.solve()
        assert b.init_launches == 2 and [b.population(k).attempts for k in range(6)] == attempts
        for k in range(6):
            assert_population_equals(b.population(k), res[k], refs[k][0], refs[k][1], 20, k)
        b.close()
    finally:
        e.close()


# --------------------------------------------------------------------------- 4. against solo GASolvers, state after every step
def solo_state(ga):
    d = ga._gd
    N, W, cap = ga.population_size, ga.num_waypoints, d["cap"]
    cells, lens = d["cells"][d["cur"]].download().reshape(N, cap), d["len"][d["cur"]].download()
    return (d["gorder"].download().tolist(), d["chrom_all"].download().reshape(N, W).tolist(), bits(d["stats_all"].download()).reshape(-1).tolist(),
            [cells[i, :lens[i]].tolist() for i in range(N)])


def batch_state(b, k):
    order, chrom, stats, cells, lens = b.device_state(k)
    return (order.tolist(), chrom.tolist(), bits(stats).reshape(-1).tolist(), [cells[i, :lens[i]].tolist() for i in range(len(lens))])


@pytest.mark.parametrize("size, K, N", [(512, 4, 256), (128, 16, 64)])
def test_batch_state_equals_solo_runs_after_begin_and_every_step(size, K, N):
    """After begin() and after EVERY step each population's device state (order, chromosomes, stats bits, path rows) equals the
    solo GASolver's on the same engine.  GASolver has no step(); its streams are keyed by generation, so a solo run with
    num_generations = g IS the first g generations.  Population 0 runs between the map's markers (the ga512 pair at 512), the
    others between seeded random free cells.  The batch runs three times: default engine choice, astar_settle 0 and 1 -- in a
    batch the choice is made by the BATCH's tail, and the results must not depend on it."""
    import pathfit
    from pathfit import env
    g = env.bench_grid(size)
    R, C = g.shape
    G, W = 3, 5
    kw = dict(population_size=N, num_waypoints_per_chromosome=W, mutation_rate=0.1, crossover_rate=0.8, tournament_size=3,
              turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0)
    pairs = [(env.find_marker(g, 2, "GA"), env.find_marker(g, 3, "GA"))] + free_pairs(g, K - 1, 5)
    starts, targets = [p[0] for p in pairs], [p[1] for p in pairs]
    seeds = [40 + k for k in range(K)]
    e = pathfit.Engine(g)
    try:
        solo = {}
        for k in range(K):
            for gen in range(G + 1):
                ga = pathfit.GASolver(moved(g, starts[k], targets[k]), num_generations=gen, engine=e, seed=seeds[k], **kw)
                res = ga.solve()
                assert ga._gd is not None, "the solo run left its device loop"
                solo[k, gen] = (solo_state(ga), result_bits(res, C), individual(ga.best_solution_overall, C),
                                bits(ga.convergence_curve).tolist())
        for settle in (-1, 0, 1):
            e.set_option("astar_settle", settle)
            b = pathfit.GABatch(g, G, seeds=seeds, starts=starts, targets=targets, engine=e, **kw)
            b.begin()
            assert b.live == list(range(K))
            for gen in range(G + 1):
                if gen:
                    b.step(gen - 1)
                for k in range(K):
                    p = b.population(k)
                    tag = (size, settle, k, gen)
                    assert batch_state(b, k) == solo[k, gen][0], (tag, "device state")
                    assert result_bits(p.result(), C) == solo[k, gen][1], (tag, "result")
                    assert individual(p.best_solution_overall, C) == solo[k, gen][2], (tag, "best individual")
                    assert bits(p.convergence_curve).tolist() == solo[k, gen][3], (tag, "curve")
            b.close()
        e.set_option("astar_settle", -1)
    finally:
        e.close()


# --------------------------------------------------------------------------- 5. degenerate populations inside a batch
def test_unreachable_target_inside_a_batch():
    """A 12 x 12 map with a walled-off cell: population 1's target is that cell -> ([], inf, 0, 0.0, 0.0, inf) as the solo class
    returns it; populations 0 and 2 equal their solo runs."""
    import pathfit
    g = np.zeros((12, 12), int)
    g[3:8, 5] = 1
    g[8:11, 8:11] = 1
    g[9, 9] = 0                                                        # free, enclosed
    kw = dict(num_generations=3, population_size=8, num_waypoints_per_chromosome=3, mutation_rate=0.2, crossover_rate=0.8)
    starts, targets, seeds = [(0, 0), (0, 0), (11, 0)], [(11, 11), (9, 9), (0, 11)], [1, 2, 3]
    e = pathfit.Engine(g)
    try:
        b = pathfit.GABatch(g, seeds=seeds, starts=starts, targets=targets, engine=e, **kw)
        res = b.solve()
        assert b.live == [0, 2]
        assert res[1] == ([], INF, 0, 0.0, 0.0, INF)
        for k in range(3):
            ga = pathfit.GASolver(moved(g, starts[k], targets[k]), engine=e, seed=seeds[k], **kw)
            ref = ga.solve()
            if k == 1:
                assert ref == res[1] and b.population(1).convergence_curve == ga.convergence_curve
                assert len(b.population(1).population) == len(ga.population)
                continue
            assert_population_equals(b.population(k), res[k], ga, ref, 12, k)
        b.close()
    finally:
        e.close()


# --------------------------------------------------------------------------- 6. neighbours are not disturbed
def test_neighbours_on_the_same_engine_and_close():
    """A solo GASolver and an MPABatch created on the Engine BEFORE the GABatch and run AFTER it give what they give alone;
    close() twice is harmless; use after close() raises PathfitError."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    pairs = free_pairs(g, 3, 9)
    starts, targets = [p[0] for p in pairs], [p[1] for p in pairs]

    def neighbours(e):
        ga = pathfit.GASolver(g, seed=4, engine=e, **GA_KW)
        mb = pathfit.MPABatch(g, 16, 4, seeds=[5, 6, 7], starts=starts, targets=targets, engine=e)
        mb.begin()
        return ga, mb

    def run(ga, mb):
        res = ga.solve()
        for it in range(1, 5):
            mb.step(it)
        return (result_bits(res, 20), bits(ga.convergence_curve).tolist(), [individual(x, 20) for x in ga.population],
                [(list(mb.school(k).best_path_overall), bits([mb.school(k).best_fitness_overall]).tolist(),
                  bits(mb.school(k).convergence_curve_data).tolist()) for k in range(3)], bits(mb.d_stats.download()).tolist())
    e0 = pathfit.Engine(g)
    alone = run(*neighbours(e0))
    e0.close()
    e = pathfit.Engine(g)
    try:
        ga, mb = neighbours(e)
        b = pathfit.GABatch(g, seeds=[8, 9, 10], starts=starts, targets=targets, engine=e, **GA_KW)
        b.solve()
        assert run(ga, mb) == alone
        b.close()
        b.close()
        for use in (b.begin, lambda: b.step(0), lambda: b.device_state(0), lambda: b.population(0).population):
            with pytest.raises(pathfit.PathfitError, match="closed"):
                use()
        # a second batch on the same engine, and one closed by closing the engine
        b2 = pathfit.GABatch(g, seeds=[8, 9, 10], starts=starts, targets=targets, engine=e, **GA_KW)
        r2 = b2.solve()
        assert [result_bits(r, 20) for r in r2] == [result_bits(b.population(k).result(), 20) for k in range(3)]
    finally:
        e.close()
    with pytest.raises(pathfit.PathfitError, match="closed"):
        b2.step(0)
    b2.close()


# --------------------------------------------------------------------------- 7. everything stays in HBM
def test_generations_keep_everything_in_hbm():
    """Per generation the host-bound copies are: the decode's 4-byte range flag, its counter block and the K best rows (ONE copy
    of K x 48 B), plus one chromosome (small), one length (small) and one path row per population whose best improves."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    K, G = 6, GA_KW["num_generations"]
    starts = [(0, 0)] + [p[0] for p in PAIRS6[:5]]
    targets = [(19, 19)] + [p[1] for p in PAIRS6[:5]]
    e = pathfit.Engine(g)
    try:
        b = pathfit.GABatch(g, seeds=[4, 11, 12, 13, 14, 15], starts=starts, targets=targets, engine=e, **GA_KW)
        b.begin()
        for gen in range(G):
            before = [b.population(k).best_solution_overall["fitness"] for k in range(K)]
            c0 = e.d2h_counts()
            b.step(gen)
            c1 = e.d2h_counts()
            took = [k for k in range(K) if b.population(k).best_solution_overall["fitness"] < before[k]]
            rows = [len(b.population(k).best_solution_overall["path"]) * 4 for k in took]
            bulk_rows = [r for r in rows if r > 128]
            assert c1[1] - c0[1] == 1 + len(bulk_rows), (gen, c0, c1, took)
            assert c1[2] - c0[2] == K * 48 + sum(bulk_rows), (gen, c0, c1, took)
            assert c1[0] - c0[0] == 2 + 2 * len(took) + (len(rows) - len(bulk_rows)), (gen, c0, c1, took)
        assert sum(len(b.population(k).convergence_curve) for k in range(K)) == K * (G + 1)
        b.close()
    finally:
        e.close()
