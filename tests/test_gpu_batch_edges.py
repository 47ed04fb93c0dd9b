"""MAACOBatch, MPABatch, GABatch and PSOBatch at the edges the solo solvers are tested at (the table of
tests/batch_edge_cases.py): the move policies other than the default, thin maps, wipes of the shared search and tabu slots in
the middle of a batched sweep, and MPABatch rows of exactly L and L - 1 cells.  The batches run device code of their own at
these edges -- the bound tables of pf_mpa_batch_create, k_tau_update_batch's per-colony strides, k_maaco_best_take_batch's rows,
k_decode_multi's slot begin -- so each case is compared with the CPU oracle loop under the same policy (the primary reference)
and with the solo solver on the grid whose markers were moved to the unit's endpoints.  Every comparison is exact: == on cells,
lengths and orders, bit patterns of the doubles; no unit, predator, ant or iteration is left out.  The option hooks are
process-wide: every test puts them back in a `finally` and closes its engines."""
import numpy as np
import pytest

import batch_edge_cases as bc
from batch_edge_cases import bits, moved

pytestmark = pytest.mark.gpu

CANARY = -7777
DEFAULTS = (("mpa_prune", 1), ("mpa_bounds_device", 0), ("maaco_pack8_min", 2048), ("maaco_load_ahead", -1), ("maaco_tabu_epoch", -1),
            ("astar_slot_avoid_epoch", -1), ("astar_slot_tag", -1), ("astar_settle", -1), ("mpa_lookahead", -1))


def reset_and_close(*engines):
    for i, e in enumerate(engines):
        if getattr(e, "h", None):
            if i == 0:
                for name, value in DEFAULTS:
                    e.set_option(name, value)
            e.close()


def ends(pairs):
    return dict(starts=[p[0] for p in pairs], targets=[p[1] for p in pairs])


# ---- MPA helpers ----------------------------------------------------------------------------------------------------------------
def mpa_run(b, ref, iters, cols, tag, upto=None):
    """begin() and `upto` (default: all) steps of an MPABatch, each compared with the oracle's log `ref` (None: no comparison)
    -> (log in test_gpu_mpa_batch's format, curves, pruned rebuilds per iteration)"""
    from test_gpu_mpa_batch import best_of, state_of_batch
    N, log, pruned = b.num_predators, [], []
    b.begin()
    upto = iters if upto is None else upto
    for it in range(1, upto + 1):
        b.step(it)
        pruned.append(b.counters()[0]["pruned_rebuilds"])
        st = state_of_batch(b)
        log.append((st, [best_of(b.school(k)) for k in range(b.K)]))
        if ref is None:
            continue
        for k in range(b.K):
            order, rows, sb = st[k]
            paths, sbits, best, bestbits = ref["log"][it - 1][k]
            assert sorted(order) == list(range(N)), (tag, k, it)
            assert [rows[slot] for slot in order] == paths, (tag, "school", k, "iteration", it, "paths")
            assert np.array_equal(sb[order], sbits), (tag, "school", k, "iteration", it, "stats")
            sc = b.school(k)
            assert [r * cols + c for r, c in sc.best_path_overall] == best, (tag, "school", k, "iteration", it, "best path")
            assert best_of(sc)[1] == bestbits, (tag, "school", k, "iteration", it, "best row")
    curves = [list(b.school(k).convergence_curve_data) for k in range(b.K)]
    if ref is not None and upto == iters:
        assert curves == ref["curves"], (tag, "curves")
    return log, curves, pruned


def check_solo(m, k, iters, log, curves, tag):
    """a solo MPA on the moved grid, begun as solve_path_planning() begins it (MPA.py:321-330) and stepped alongside school k of
    the batch's log: population, order and best row after EVERY iteration, and the curve"""
    from test_gpu_mpa_batch import best_of, same_state, state_of_solo
    m._sort()
    slot, s0 = m._best_row()
    m._take_first(s0, m._fetch(slot))
    for it in range(1, iters + 1):
        m.step(it)
        assert same_state(state_of_solo(m), log[it - 1][0][k]), (tag, "school", k, "iteration", it, "population / order differ from the solo run")
        assert best_of(m) == log[it - 1][1][k], (tag, "school", k, "iteration", it, "best row differs from the solo run")
    assert list(m.convergence_curve_data) == curves[k], (tag, "school", k, "curve")


def same_logs(a, b):
    from test_gpu_mpa_batch import same_state
    return len(a) == len(b) and all(same_state(x[0][k], y[0][k]) and x[1][k] == y[1][k] for x, y in zip(a, b) for k in range(len(x[0])))


# ---- 1. move policies -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ad,rs", bc.POLICIES)
def test_mpa_batch_move_policies(ad, rs):
    """fig7, K = 4 (two schools share a start cell, two a target cell: shared bound tables), N = 24, 9 iterations, non-default
    weights: every iteration equals MpaOracle under the same policy, with the bound tables from the host and from the device, with
    pruning on and off.  Pruning fires with mpa_prune 1, never with 0, and changes nothing; the tables of the two builders prune
    the same rebuilds; and in every iteration the batch prunes exactly as many rebuilds as the K solo runs on the moved grids do -- their tables are
    built for the same policy from the same cells, so a batch table built for another policy shows here even where it only makes
    the bound weaker."""
    import pathfit
    c, g = bc.MPA_POLICY, bc.fig7()
    ref = bc.mpa_policy_reference(ad, rs)
    kw = dict(allow_diagonal_moves=bool(ad), restrict_diagonal_near_obstacle=bool(rs), **bc.MPA_KW, **bc.MPA_W)
    eb, es = pathfit.Engine(g), pathfit.Engine(g)
    runs = {}
    try:
        for device in (0, 1):
            for prune in (1, 0):
                eb.set_option("mpa_bounds_device", device)
                eb.set_option("mpa_prune", prune)
                b = pathfit.MPABatch(g, c["N"], c["iters"], seeds=c["seeds"], engine=eb, **ends(c["pairs"]), **kw)
                runs[device, prune] = mpa_run(b, ref, c["iters"], 20, (ad, rs, device, prune))
                b.close()
        eb.set_option("mpa_bounds_device", 0)                            # (process-wide: the solo runs prune, with host-built tables)
        eb.set_option("mpa_prune", 1)
        eb.set_option("mpa_lookahead", 0)                                # (a solo sweep that runs ahead also counts the levels it may discard)
        solo_pruned = np.zeros(c["iters"], int)
        log, curves, pruned = runs[0, 1]
        for k, (s, t) in enumerate(c["pairs"]):
            m = pathfit.MPA(moved(g, s, t), c["N"], c["iters"], seed=c["seeds"][k], engine=es, **kw)
            step, count = m.step, []

            def counted(it):
                out = step(it)
                count.append(es.counters()["pruned_rebuilds"])
                return out
            m.step = counted
            check_solo(m, k, c["iters"], log, curves, (ad, rs))
            solo_pruned += np.array(count)
        print("pruned rebuilds per iteration:", {key: r[2] for key, r in runs.items()}, "the solo runs together:", solo_pruned.tolist())
        for device in (0, 1):
            assert sum(runs[device, 1][2]) > 0 and sum(runs[device, 0][2]) == 0, (device, runs[device, 1][2], runs[device, 0][2])
        assert runs[0, 1][2] == runs[1, 1][2], "the host-built and the device-built bound tables prune different rebuilds"
        assert pruned == solo_pruned.tolist(), "the batch's bound tables prune other rebuilds than the solo runs' tables"
        for key in runs:
            assert same_logs(runs[key][0], log) and runs[key][1] == curves, key
        if not ad:
            for st, bests in log:
                for order, rows, _ in st:
                    assert all(bc.four_connected(r, 20) for r in rows)
                assert all(bc.four_connected([r * 20 + c_ for r, c_ in p], 20) for p, _ in bests)
    finally:
        reset_and_close(eb, es)


def ga_units_equal(b, res, refs, solo_of, cols, tag):
    """every population of a GABatch == the oracle-backed host loop (refs[k], None for a degenerate one) == the solo GASolver"""
    from test_gpu_ga_batch import assert_population_equals
    for k in range(b.K):
        ga = solo_of(k)
        want = ga.solve()
        if refs[k] is None:                                              # degenerate: handed to the solo class, reported in its place
            assert k not in b.live and res[k] == want and b.population(k).convergence_curve == ga.convergence_curve, (tag, k)
            assert len(b.population(k).population) == len(ga.population), (tag, k)
            continue
        assert k in b.live, (tag, k)
        assert_population_equals(b.population(k), res[k], refs[k][0], refs[k][1], cols, (tag, k, "oracle loop"))
        assert_population_equals(b.population(k), res[k], ga, want, cols, (tag, k, "solo"))


@pytest.mark.parametrize("ad,rs", bc.POLICIES)
def test_ga_batch_move_policies(ad, rs):
    """fig7, K = 3, N = 24, 4 generations under each policy: result tuple, best individual, curve and whole final population."""
    import pathfit
    c, g = bc.GA_POLICY, bc.fig7()
    kw = dict(allow_diagonal_moves=bool(ad), restrict_diagonal_near_obstacle_policy=bool(rs), **c["kw"])
    e = pathfit.Engine(g)
    try:
        b = pathfit.GABatch(g, seeds=c["seeds"], engine=e, **ends(c["pairs"]), **kw)
        res = b.solve()
        ga_units_equal(b, res, bc.ga_policy_reference(ad, rs),
                       lambda k: pathfit.GASolver(moved(g, *c["pairs"][k]), engine=e, seed=c["seeds"][k], **kw), 20, (ad, rs))
        if not ad:
            assert all(bc.four_connected([r * 20 + c_ for r, c_ in x["path"].tolist()], 20) for k in range(3) for x in b.population(k).population)
        b.close()
    finally:
        reset_and_close(e)


# ---- 2. thin maps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", bc.THIN_KEYS + [bc.THIN_LONG])
def test_maaco_batch_thin_maps(key):
    """K = 3 colonies (2 on 1 x 4096), 6 and 70 ants, beta 7 and 2, 3 iterations, eight ants per wavefront and one, load-ahead
    form off and on: best path, length, turns, curve and the whole pheromone matrix of every colony equal the oracle loop, and a
    solo MAACO on the moved grid.  On R * C <= 64 one 64-cell stretch holds a whole colony of k_tau_update_batch's grid; on the
    obstacle maps the far-target colony's walks fail (no deposit, no take-over row) beside colonies that do take over."""
    import pathfit
    from test_gpu_maaco_batch import check_vs_oracle
    g, pairs, seeds = bc.thin_units(key)
    cols, iters = g.shape[1], 2 if key == bc.THIN_LONG else 3
    e, es = pathfit.Engine(g), pathfit.Engine(g)
    try:
        for n_ants, beta in bc.thin_maaco_runs(key):
            kw = dict(bc.MAACO_KW, beta=beta)
            ref = bc.thin_maaco_reference(key, n_ants, beta)
            solos = []
            for (s, t), sd in zip(pairs, seeds):
                m = pathfit.MAACO(moved(g, s, t), n_ants, iters, engine=es, seed=sd, **kw)
                m.solve_path_planning()
                solos.append((m.best_path_overall, m.best_path_length_overall, m.best_path_turns_overall, list(m.convergence_curve_data),
                              m.pheromone_matrix.copy()))
            for pack8 in (1, 1 << 30):
                for ahead in (0, 1):
                    e.set_option("maaco_pack8_min", pack8)
                    e.set_option("maaco_load_ahead", ahead)
                    b = pathfit.MAACOBatch(g, n_ants, iters, C0_initial_pheromone=0.1, seeds=seeds, engine=e, **ends(pairs), **kw)
                    res = b.solve_path_planning()
                    for k in range(len(pairs)):
                        where = (key, n_ants, beta, pack8, ahead, k)
                        col = b.colony(k)
                        check_vs_oracle(col, ref[k][0], cols)
                        assert [r * cols + c for r, c in res[k][0]] == list(ref[k][0]["path"]) and res[k][1] == ref[k][0]["length"], where
                        assert (col.best_path_overall, col.best_path_length_overall, col.best_path_turns_overall) == solos[k][:3], where
                        assert col.convergence_curve_data == solos[k][3] and np.array_equal(col.pheromone_matrix, solos[k][4]), where
                    b.close()
    finally:
        reset_and_close(e, es)


@pytest.mark.parametrize("key", bc.THIN_KEYS)
def test_mpa_batch_thin_maps(key):
    """K = 3 schools of 16 predators, 6 iterations: every iteration equals MpaOracle and a solo MPA on the moved grid.  On 1 x 2 the
    rows are 2 cells (path_cap = min(R C, ...)); on the obstacle maps a school whose target cannot be reached keeps the fallback
    population [start, target] beside live schools."""
    import pathfit
    g, pairs, seeds = bc.thin_units(key)
    N, iters = bc.THIN_MPA["N"], bc.THIN_MPA["iters"]
    kw = dict(bc.MPA_KW, **bc.MPA_W)
    e, es = pathfit.Engine(g), pathfit.Engine(g)
    try:
        b = pathfit.MPABatch(g, N, iters, seeds=seeds, engine=e, **ends(pairs), **kw)
        assert b.path_cap == min(g.size, 8 * sum(g.shape) + 64)
        log, curves, _ = mpa_run(b, bc.thin_mpa_reference(key), iters, g.shape[1], key)
        for k, (s, t) in enumerate(pairs):
            check_solo(pathfit.MPA(moved(g, s, t), N, iters, seed=seeds[k], engine=es, **kw), k, iters, log, curves, key)
        b.close()
    finally:
        reset_and_close(e, es)


@pytest.mark.parametrize("key", bc.THIN_WP_KEYS)
def test_ga_batch_thin_maps(key):
    """W = 3, N = 12, 3 generations on 2 x 17 (empty, obstacles) and 2 x 2, where the decodes are longer than the grid (rows of
    R C + W + 1 cells)."""
    import pathfit
    g, pairs, seeds = bc.thin_units(key)
    e = pathfit.Engine(g)
    try:
        b = pathfit.GABatch(g, seeds=seeds, engine=e, **ends(pairs), **bc.THIN_GA_KW)
        assert b.path_cap >= g.size + 3 + 1
        res = b.solve()
        ga_units_equal(b, res, bc.thin_ga_reference(key),
                       lambda k: pathfit.GASolver(moved(g, *pairs[k]), engine=e, seed=seeds[k], **bc.THIN_GA_KW), g.shape[1], key)
        b.close()
    finally:
        reset_and_close(e)


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("key", bc.THIN_WP_KEYS)
def test_pso_batch_thin_maps(key, sync):
    """W = 3, N = 12, 3 iterations, asynchronous and synchronous: curve, positions, pbest fitnesses and gbest path equal the loop
    over the oracle; everything (gbest record, every particle, every device row, rounds per sweep) equals the solo PSOSolver."""
    import pathfit
    from test_gpu_pso_batch import assert_swarm_equals, cellpath, result_bits, solo_run
    g, pairs, seeds = bc.thin_units(key)
    cols = g.shape[1]
    kw = dict(bc.THIN_PSO_KW, asynchronous=not sync)
    refs = bc.thin_pso_reference(key, sync)
    e = pathfit.Engine(g)
    try:
        b = pathfit.PSOBatch(g, seeds=seeds, engine=e, **ends(pairs), **kw)
        res = b.solve()
        for k, (s, t) in enumerate(pairs):
            if refs[k] is None:                                          # degenerate: the solo class runs it whole
                ps = pathfit.PSOSolver(moved(g, s, t), engine=e, seed=seeds[k], **kw)
                want = ps.solve()
                assert k not in b.live and result_bits(res[k], cols) == result_bits(want, cols), (key, sync, k)
                assert bits(b.swarm(k).convergence_curve).tolist() == bits(ps.convergence_curve).tolist(), (key, sync, k)
                continue
            assert k in b.live, (key, sync, k)
            got = b.device_state(k)
            assert bits(b.swarm(k).convergence_curve).tolist() == bits(refs[k]["curve"]).tolist(), (key, sync, k, "curve")
            assert np.array_equal(bits(got[0]), bits(refs[k]["pos"])) and np.array_equal(bits(got[3]), bits(refs[k]["pbest_fit"])), (key, sync, k)
            assert cellpath(res[k][0], cols) == refs[k]["gpath"], (key, sync, k, "gbest path")
            ps, want, rounds = solo_run(e, g, s, t, seeds[k], kw)
            assert b.swarm(k).rounds == rounds, (key, sync, k)
            assert_swarm_equals(b, k, res[k], ps, want, (key, sync, k))
        b.close()
    finally:
        reset_and_close(e)


# ---- 3. slot wipes inside batched sweeps ----------------------------------------------------------------------------------------
def slot_hooks():
    """(name, option hook, astar_settle, index into slot_state, bound the counter is back under afterwards)"""
    from test_gpu_slot_wraps import AVOID_LIMIT, TAG_LIMIT
    return (("avoid", ("astar_slot_avoid_epoch", AVOID_LIMIT - 2), -1, 1, 64), ("avoid, sequential loop", ("astar_slot_avoid_epoch", AVOID_LIMIT - 2), 0, 1, 64),
            ("tag", ("astar_slot_tag", TAG_LIMIT - 1), 0, 0, 1 << 16))


def slots_wiped_or_waiting(e, n, idx, max_evals):
    """The first n slots after a run of at most max_evals evaluations that began with a hook: a slot that evaluated twice or more
    since the hook has been wiped and counts up from 1 again (an evaluation takes one avoid epoch and at most two tags here, W + 1
    in a decode); a slot that evaluated less still waits at the hooked value (tag: or just past its limit).  No stored avoid epoch
    reaches its limit -- the evaluation that takes it there wipes first -- and at least one slot has been wiped."""
    from test_gpu_slot_wraps import AVOID_LIMIT, TAG_LIMIT
    vals = [e.slot_state(i)[idx] for i in range(n)]
    lo, hi, small = ((AVOID_LIMIT - 2, AVOID_LIMIT, max_evals + 1) if idx == 1 else (TAG_LIMIT - 1, TAG_LIMIT + 2 * 0x8000, 6 * max_evals + 1))
    assert small < lo
    assert all(1 <= v <= small or lo <= v < hi for v in vals), vals
    assert any(v <= small for v in vals), vals


def test_mpa_batch_slot_wipes():
    """The wrap map, K = 3, N = 32, 6 iterations.  On fresh counters the batch equals MpaOracle; then, on fresh engines, every
    slot's avoid epoch starts two evaluations below its wipe (by default and with the sequential pop loop), or every slot's tag one
    search below its limit: the wipes fall inside the batched sweeps, and every iteration equals the fresh run.  An item whose gate fails or
    that is pruned evaluates nothing, so no particular slot is sure to evaluate twice: the counters of the first 32 slots are read
    instead of slot 0's alone."""
    import pathfit
    import test_gpu_slot_wraps as sw
    c, g, pairs = bc.WIPE_MPA, bc.wrap_grid(), bc.wipe_mpa_pairs()
    n = g.shape[0]
    engines = []

    def run(hook, settle, ref):
        e = pathfit.Engine(g)
        engines.insert(0, e)
        e.set_option("astar_settle", settle)
        b = pathfit.MPABatch(g, c["N"], c["iters"], seeds=c["seeds"], engine=e, **ends(pairs), **sw.MPA_KW)
        if hook:
            e.set_option(*hook)                                          # applied in front of the next search launch: step(1)'s sweep
        return e, mpa_run(b, ref, c["iters"], n, (hook, settle))
    try:
        e, fresh = run(None, -1, bc.wipe_mpa_reference())
        assert e.slot_state(0)[1] < 64
        for name, hook, settle, idx, bound in slot_hooks():
            e, got = run(hook, settle, None)
            assert same_logs(got[0], fresh[0]) and got[1] == fresh[1], name
            slots_wiped_or_waiting(e, 32, idx, 2 * 3 * c["N"] * c["iters"])
    finally:
        reset_and_close(*engines)


def test_ga_batch_slot_wipes():
    """The wrap map, K = 2, N = 24, W = 5, 2 generations: the fresh run equals the oracle-backed loop; with the hooks set before
    begin() the initial rounds and both generations run k_decode_multi on slots that are wiped between them, and the device state
    after begin() and after every generation equals the fresh run.  Only k_decode_multi evaluates between the hook and the
    read of the counters, so they come back through ITS slot begin."""
    import pathfit
    from test_gpu_ga_batch import assert_population_equals, batch_state, individual, result_bits
    c, g, pairs = bc.WIPE_GA, bc.wrap_grid(), bc.wipe_ga_pairs()
    cols, G = g.shape[1], c["kw"]["num_generations"]
    engines = []

    def run(hook, settle):
        e = pathfit.Engine(g)
        engines.insert(0, e)
        e.set_option("astar_settle", settle)
        b = pathfit.GABatch(g, seeds=c["seeds"], engine=e, **ends(pairs), **c["kw"])
        if hook:
            e.set_option(*hook)
        b.begin()
        assert b.live == [0, 1]
        states = []
        for gen in range(G + 1):
            if gen:
                b.step(gen - 1)
            states.append([(batch_state(b, k), result_bits(b.population(k).result(), cols), individual(b.population(k).best_solution_overall, cols),
                            bits(b.population(k).convergence_curve).tolist()) for k in range(2)])
        return e, b, states
    try:
        e, b, fresh = run(None, -1)
        for k, (s, t) in enumerate(pairs):
            ga, want = bc.oracle_ga(g, s, t, c["seeds"][k], **c["kw"])
            assert_population_equals(b.population(k), b.population(k).result(), ga, want, cols, ("fresh", k))
        for name, hook, settle, idx, bound in slot_hooks():
            e, b, got = run(hook, settle)
            assert got == fresh, name
            slots_wiped_or_waiting(e, 24, idx, 20 * 2 * 24 + 2 * 2 * 24)       # (at most 20 N initial attempts a population)
            assert 1 <= e.slot_state(0)[idx] < bound, (name, e.slot_state(0))
    finally:
        reset_and_close(*engines)


@pytest.mark.parametrize("pack8", [1, 1 << 30])
def test_maaco_batch_tabu_epoch_wrap(pack8):
    """fig7, K = 3, 70 ants, both walk kernels: every tabu slot starts just below the 16-bit epoch wrap, so the ants of the batch
    cross it (slot wipe + epoch restart) inside the run; pheromone and paths equal the oracle loop."""
    import pathfit
    from test_gpu_maaco_batch import check_vs_oracle
    c, g, pairs = bc.WIPE_MAACO, bc.fig7(), bc.wipe_maaco_pairs()
    ref = bc.wipe_maaco_reference()
    e = pathfit.Engine(g)
    try:
        e.set_option("maaco_pack8_min", pack8)
        for ep in bc.TABU_EPOCHS:                                        # (descending: a slot never revisits an epoch between two wipes)
            b = pathfit.MAACOBatch(g, c["n_ants"], c["iters"], C0_initial_pheromone=0.1, seeds=c["seeds"], engine=e, **ends(pairs),
                                   **dict(bc.MAACO_KW, beta=c["beta"]))
            e.set_option("maaco_tabu_epoch", ep)
            res = b.solve_path_planning()
            for k in range(3):
                check_vs_oracle(b.colony(k), ref[k][0], 20)
                assert [r * 20 + c_ for r, c_ in res[k][0]] == list(ref[k][0]["path"]), (pack8, ep, k)
            b.close()
    finally:
        reset_and_close(e)


def test_interleaved_solvers_share_one_wipe():
    """One Engine on the wrap map: a solo MPA step, an MPABatch step and a MAACOBatch iteration, three times over, with the
    avoid-epoch hook set once in front: whichever kernel crosses the limit first wipes the slots for all of them, and each solver
    equals its isolated run on an engine of its own."""
    import pathfit
    import test_gpu_slot_wraps as sw
    from test_gpu_mpa_batch import best_of, same_state, state_of_batch, state_of_solo
    c, g, pairs = bc.WIPE_MPA, bc.wrap_grid(), bc.wipe_mpa_pairs()
    iters = 3
    mkw = dict(bc.MAACO_KW, beta=7.0)
    engines = []

    def make(e_solo, e_batch, e_maaco):
        m = pathfit.MPA(g, 36, c["iters"], seed=77, engine=e_solo, **sw.MPA_KW)
        b = pathfit.MPABatch(g, c["N"], c["iters"], seeds=c["seeds"], engine=e_batch, **ends(pairs), **sw.MPA_KW)
        a = pathfit.MAACOBatch(g, 70, iters, C0_initial_pheromone=0.1, seeds=[1, 2, 3], engine=e_maaco, **ends(pairs), **mkw)
        b.begin()
        return m, b, a

    def step(m, b, a, it):
        m.step(it)
        b.step(it)
        a.iterate_dev(it)
        return ((state_of_solo(m), best_of(m)), (state_of_batch(b), [best_of(b.school(k)) for k in range(3)]),
                [(a.colony(k).pheromone_matrix.copy(), list(a.colony(k).convergence_curve_data)) for k in range(3)])
    try:
        engines[:] = [pathfit.Engine(g) for _ in range(3)]
        alone = make(*engines)
        want = [step(*alone, it) for it in range(1, iters + 1)]
        e = pathfit.Engine(g)
        engines.insert(0, e)
        shared = make(e, e, e)
        e.set_option("astar_slot_avoid_epoch", sw.AVOID_LIMIT - 2)
        for it in range(1, iters + 1):
            (ms, mb), (bs, bb), cols = step(*shared, it)
            (wms, wmb), (wbs, wbb), wcols = want[it - 1]
            assert same_state(ms, wms) and mb == wmb, ("solo MPA", it)
            assert all(same_state(bs[k], wbs[k]) for k in range(3)) and bb == wbb, ("MPABatch", it)
            assert all(np.array_equal(cols[k][0], wcols[k][0]) and cols[k][1] == wcols[k][1] for k in range(3)), ("MAACOBatch", it)
        slots_wiped_or_waiting(e, 32, 1, iters * 2 * (36 + 3 * c["N"]))
    finally:
        reset_and_close(*engines)


# ---- 4. exact-fit rows ------------------------------------------------------------------------------------------------------------
class FramedRows:
    """rows x cap candidate cells between two guard rows of a canary value, handed to the facade as its candidate buffer"""

    def __init__(self, e, rows, cap):
        from pathfit.engine import _View
        self.buf = e.put(np.full((rows + 2, cap), CANARY, np.int32))
        self.view = _View(e, self.buf.at(cap), rows * cap, np.int32)

    def guards_hold(self):
        c = self.buf.download()
        return bool((c[0] == CANARY).all() and (c[-1] == CANARY).all())


def test_mpa_batch_exact_fit_rows():
    """Lmax = the longest path any school BUILDS over the oracle's run (phase and FADs candidates, accepted or not; pruning off, so
    every one is built).  With path_cap = Lmax the batch runs to the end and equals the oracle; with Lmax - 1 it raises the
    capacity overflow at the iteration in which the oracle first builds a path of Lmax cells, and not before it.  The candidate
    rows lie between guard rows: nothing is written outside them, and a one-cell overrun inside them lands in the next predator's
    row, which the comparison with the oracle reads."""
    import pathfit
    c, g = bc.FIT_MPA, bc.fig7()
    ref = bc.fit_mpa_reference()
    Lmax, at = bc.fit_lengths(ref)
    kw = dict(seeds=c["seeds"], **ends(c["pairs"]), **bc.MPA_KW, **bc.MPA_W)
    KN = len(c["seeds"]) * c["N"]
    e = pathfit.Engine(g)
    try:
        e.set_option("mpa_prune", 0)

        def framed(cap):
            b = pathfit.MPABatch(g, c["N"], c["iters"], engine=e, path_cap=cap, **kw)
            assert b.path_cap == cap
            frames = FramedRows(e, KN, cap), FramedRows(e, KN, cap)
            b.d_c1_cells, b.d_c2_cells = frames[0].view, frames[1].view
            return b, frames
        b, frames = framed(Lmax)
        mpa_run(b, ref, c["iters"], 20, "path_cap = Lmax")
        assert b.counters()[1] == 0 and all(f.guards_hold() for f in frames)
        b.close()
        b, frames = framed(Lmax - 1)
        mpa_run(b, ref, c["iters"], 20, "path_cap = Lmax - 1", upto=at - 1)     # every iteration before it fits, and equals the oracle
        with pytest.raises(RuntimeError, match=r"capacity overflow on \d+ predators \(path_cap=%d\)" % (Lmax - 1)):
            b.step(at)
        assert b.counters()[1] > 0 and all(f.guards_hold() for f in frames)
        b.close()
    finally:
        reset_and_close(e)
