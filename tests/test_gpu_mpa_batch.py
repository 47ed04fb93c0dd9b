"""MPABatch: K independent MPA schools in one batched sweep.  Every school must equal, bit for bit, a solo run with its seed, start
and target -- the oracle loop (oracle/pf_loops.py) on the 20 x 20 map, a solo pathfit.MPA on the bench maps -- in every predator's
path, length and fp64 stats, in the sorted order, in the best-so-far row after every iteration and in the convergence curve.
All comparisons are exact (== on cells, lengths and orders; bit patterns of the doubles); no school and no predator is left out."""
import collections
import ctypes as C

import numpy as np
import pytest

import golden_io as gio
from batch_edge_cases import free_pairs, moved, bits               # noqa: F401  (shared by the batch test files)

pytestmark = pytest.mark.gpu


def best_of(x):
    """the best-so-far row of a solo MPA or of a school, doubles as bit patterns"""
    return (list(x.best_path_overall), bits([x.best_path_length_overall, x.best_path_turns_overall, x.best_safety_penalty_overall,
                                              x.best_diag_penalty_overall, x.best_fitness_overall]).tolist())


def state_of_batch(b):
    """per school: (order, [cells of storage row r], stats bits [N][5]) -- the whole device state of the populations"""
    K, N = b.K, b.num_predators
    cells, lens, stats, order = b.d_cells.download(), b.d_len.download(), b.d_stats.download(), b.d_order.download()
    out = []
    for k in range(K):
        rows = range(k * N, (k + 1) * N)
        out.append((order[k * N:(k + 1) * N].tolist(), [cells[r, :lens[r]].tolist() for r in rows], bits(stats[k * N:(k + 1) * N])))
    return out


def state_of_solo(m):
    cells, lens, stats = m.d_cells.download(), m.d_len.download(), m.d_stats.download()
    return (m.order.tolist(), [cells[r, :lens[r]].tolist() for r in range(m.n_local)], bits(stats))


def same_state(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def run_batch_steps(b, iters):
    """step by step -> per iteration (states of all schools, bests of all schools); curves at the end"""
    log = []
    for it in range(1, iters + 1):
        b.step(it)
        log.append((state_of_batch(b), [best_of(b.school(k)) for k in range(b.K)]))
    return log, [list(b.school(k).convergence_curve_data) for k in range(b.K)]


def check_solo_steps(make_solo, k, iters, log, curves):
    """a solo MPA stepped alongside the batch's log of school k: population, order and best row after EVERY iteration"""
    m = make_solo()
    for it in range(1, iters + 1):
        m.step(it)
        assert same_state(state_of_solo(m), log[it - 1][0][k]), f"school {k}, iteration {it}: population / order differ from the solo run"
        assert best_of(m) == log[it - 1][1][k], f"school {k}, iteration {it}: best row differs from the solo run"
    assert list(m.convergence_curve_data) == curves[k]
    return m


KW = dict(FADs_rate=0.2, P_const=0.5, levy_beta=1.5)


# --------------------------------------------------------------------------- 1. against the oracle loop
def counting_oracle():
    """MpaOracle that also counts what a run exercised: accepted candidates per phase, FADs branches tried / taken."""
    import pf_loops

    class Counting(pf_loops.MpaOracle):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.events = collections.Counter()

        def phase_candidate(self, it, i, elite, CF):
            c = super().phase_candidate(it, i, elite, CF)
            if c[1][4] < self.pop[i][1][4]:                          # the memory step will take it (MPA.py:382)
                self.events["phase%d" % (1 if it <= self.K / 3 else (2 if it <= 2 * self.K / 3 else 3))] += 1
            return c

        def fads(self, it, i, ind, CF):
            out = super().fads(it, i, ind, CF)
            g = self.o.rng(self.seed, pf_loops.DOM_MPA_FADS, it, i)  # replay the two gating draws (MPA.py:389-390)
            if self.L.orc_rng_random(C.byref(g)) < self.fads_rate:
                kind = "detour" if self.L.orc_rng_random(C.byref(g)) < CF else "reinit"
                self.events[kind + "_tried"] += 1
                if out is not ind:
                    self.events[kind + "_taken"] += 1
            return out
    return Counting


def test_six_schools_match_the_oracle_loop_every_iteration():
    """fig7, K = 6 (distinct seeds, random free start / target pairs), N = 30, 12 iterations: 4 per phase, CF reaches 0.
    The pairs and seeds were picked with the oracle on the CPU so that the batch as a whole accepts a candidate in each phase and
    a FADs detour, and takes the FADs re-init branch.

    On the re-init branch (MPA.py:405-409): its candidate is the initial path, and every predator starts AS the initial path and
    is only ever replaced by something strictly fitter (:382, :402, :408), so `init fitness < predator fitness` can never hold:
    the branch produces its candidate and the comparison rejects it, in the reference as here.  The test therefore asserts that the
    branch RAN (237 times in this configuration) and that the oracle never accepted it -- an accepted re-init cannot exist."""
    import pathfit, pf_oracle as po
    g, _, _ = gio.grid("fig7")
    N, iters = 30, 12
    pairs = free_pairs(g, 6, seed=1)
    seeds = [100 + k for k in range(6)]
    b = pathfit.MPABatch(g, N, iters, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    orc, Counting = po.Oracle(g), counting_oracle()
    refs = [Counting(orc, s[0] * 20 + s[1], t[0] * 20 + t[1], N, iters, seed=seeds[k], **KW) for k, (s, t) in enumerate(pairs)]
    b.begin()
    for k, ref in enumerate(refs):
        ref._sort()
        ref.best = ref.pop[0]
        ref.curve.append(ref.best[1][4])
    for it in range(1, iters + 1):
        b.step(it)
        st = state_of_batch(b)
        for k, ref in enumerate(refs):
            ref.step(it)
            order, rows, sb = st[k]
            assert sorted(order) == list(range(N))
            assert [rows[slot] for slot in order] == [p[0].tolist() for p in ref.pop], f"school {k}, iteration {it}: paths"
            assert np.array_equal(sb[order], bits(np.array([p[1] for p in ref.pop]))), f"school {k}, iteration {it}: stats"
            sc = b.school(k)
            assert [r * 20 + c for r, c in sc.best_path_overall] == ref.best[0].tolist(), f"school {k}, iteration {it}: best path"
            assert best_of(sc)[1] == bits(ref.best[1]).tolist(), f"school {k}, iteration {it}: best row"
    ev = collections.Counter()
    for k, ref in enumerate(refs):
        assert b.school(k).convergence_curve_data == ref.curve
        ev += ref.events
    assert ev["phase1"] > 0 and ev["phase2"] > 0 and ev["phase3"] > 0, ev
    assert ev["detour_taken"] > 0, ev
    assert ev["reinit_tried"] > 0 and ev["reinit_taken"] == 0, ev
    # the batch's school view of population agrees with the raw rows (the read surface)
    pop = b.school(3).population
    assert [p["path"].cells.tolist() for p in pop] == [p[0].tolist() for p in refs[3].pop]
    assert [p["fitness"] for p in pop] == [float(p[1][4]) for p in refs[3].pop]


# --------------------------------------------------------------------------- 2. against solo MPA, pruning on and off
def test_eight_schools_match_solo_mpa_with_and_without_pruning():
    """bench_grid(128), K = 8, N = 256, 9 iterations (3 per phase): every school equals a solo MPA on the moved-marker grid after
    every iteration; with mpa_prune 1 the batch prunes rebuilds, with 0 it does not, and nothing else changes."""
    import pathfit
    from pathfit import env
    g = env.bench_grid(128)
    K, N, iters = 8, 256, 9
    pairs = free_pairs(g, K, seed=3)
    seeds = [40 + k for k in range(K)]
    eb, es = pathfit.Engine(g), pathfit.Engine(g)
    runs = []
    try:
        for prune in (1, 0):
            eb.set_option("mpa_prune", prune)
            b = pathfit.MPABatch(g, N, iters, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], engine=eb, **KW)
            pruned, log = 0, []
            for it in range(1, iters + 1):
                b.step(it)
                pruned += b.counters()[0]["pruned_rebuilds"]
                log.append((state_of_batch(b), [best_of(b.school(k)) for k in range(K)]))
            curves = [list(b.school(k).convergence_curve_data) for k in range(K)]
            runs.append((log, curves, pruned))
            b.close()
            if prune:
                for k, (s, t) in enumerate(pairs):
                    check_solo_steps(lambda: pathfit.MPA(moved(g, s, t), N, iters, seed=seeds[k], engine=es, **KW), k, iters, log, curves)
    finally:
        eb.set_option("mpa_prune", 1)
    assert runs[0][2] > 0 and runs[1][2] == 0
    for it in range(iters):
        for k in range(K):
            assert same_state(runs[0][0][it][0][k], runs[1][0][it][0][k]) and runs[0][0][it][1][k] == runs[1][0][it][1][k]
    assert runs[0][1] == runs[1][1]
    eb.close()
    es.close()


# --------------------------------------------------------------------------- 3. at a size the bench quotes
def test_four_schools_of_1024_on_512_match_solo_runs():
    """bench_grid(512), K = 4, N = 1024 -- the 4096 predators per sweep of the mpa512 bench row -- 3 iterations (one per phase),
    through solve_path_planning() on both sides: results, curves, whole populations and orders."""
    import pathfit
    from pathfit import env
    g = env.bench_grid(512)
    K, N, iters = 4, 1024, 3
    pairs = free_pairs(g, K, seed=5)
    seeds = [7, 7, 8, 9]                                              # (two schools share a seed: their cells differ)
    eb, es = pathfit.Engine(g), pathfit.Engine(g)
    b = pathfit.MPABatch(g, N, iters, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], engine=eb, **KW)
    res = b.solve_path_planning()
    st = state_of_batch(b)
    assert len(res) == K
    for k, (s, t) in enumerate(pairs):
        m = pathfit.MPA(moved(g, s, t), N, iters, seed=seeds[k], engine=es, **KW)
        want = m.solve_path_planning()
        assert res[k][0] == want[0] and bits(res[k][1:]).tolist() == bits(want[1:]).tolist(), f"school {k}: result"
        assert b.school(k).convergence_curve_data == m.convergence_curve_data
        assert best_of(b.school(k)) == best_of(m)
        assert same_state(state_of_solo(m), st[k]), f"school {k}: population / order"
    eb.close()
    es.close()


# --------------------------------------------------------------------------- 4. an unreachable target
def test_school_with_a_sealed_target_keeps_the_fallback_population():
    """One school's target sits in a sealed room: it keeps the reference's fallback population [start, target] (MPA.py:235-236)
    with the fitness the solo run reports; the other schools are what they are without it."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    g = np.array(g, dtype=int)
    room = (9, 9)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            g[room[0] + dr, room[1] + dc] = 0 if (dr, dc) == (0, 0) else 1   # (fig7's markers are in the corners)
    ring = {(room[0] + dr, room[1] + dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1)}
    pairs = [p for p in free_pairs(g, 12, seed=2) if not (set(p) & ring)][:3]
    pairs.insert(1, (pairs[0][0], room))                              # school 1: sealed target
    seeds, N, iters = [5, 6, 7, 8], 24, 6
    e1, e2 = pathfit.Engine(g), pathfit.Engine(g)
    b = pathfit.MPABatch(g, N, iters, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], engine=e1, **KW)
    log, curves = run_batch_steps(b, iters)
    solos = [check_solo_steps(lambda: pathfit.MPA(moved(g, s, t), N, iters, seed=seeds[k], engine=e2, **KW), k, iters, log, curves)
             for k, (s, t) in enumerate(pairs)]
    s, t = pairs[1]
    fallback = [s[0] * 20 + s[1], t[0] * 20 + t[1]]
    order, rows, sb = log[-1][0][1]
    assert all(r == fallback for r in rows)
    assert b.school(1).best_path_overall == [s, t] and b.school(1).best_fitness_overall == solos[1].best_fitness_overall
    # without the sealed school, the others are bit for bit the same
    keep = [0, 2, 3]
    b2 = pathfit.MPABatch(g, N, iters, seeds=[seeds[k] for k in keep], starts=[pairs[k][0] for k in keep],
                          targets=[pairs[k][1] for k in keep], engine=e1, **KW)
    log2, curves2 = run_batch_steps(b2, iters)
    for j, k in enumerate(keep):
        for it in range(iters):
            assert same_state(log2[it][0][j], log[it][0][k]) and log2[it][1][j] == log[it][1][k]
        assert curves2[j] == curves[k]
        assert len(b.school(k).best_path_overall) > 2 and b.school(k).best_path_overall[-1] == pairs[k][1]
    e1.close()
    e2.close()


# --------------------------------------------------------------------------- 5. independence
def test_changing_one_seed_changes_no_bit_of_the_other_schools():
    import pathfit
    from pathfit import env
    g = env.bench_grid(128)
    K, N, iters = 4, 64, 6
    pairs = free_pairs(g, K, seed=10)                                # (school 1's population depends on its seed: checked with the oracle)
    e = pathfit.Engine(g)
    logs = []
    for s1 in (21, 99):
        b = pathfit.MPABatch(g, N, iters, seeds=[20, s1, 22, 23], starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], engine=e, **KW)
        logs.append(run_batch_steps(b, iters))
        b.close()
    for it in range(iters):
        for k in (0, 2, 3):
            assert same_state(logs[0][0][it][0][k], logs[1][0][it][0][k]) and logs[0][0][it][1][k] == logs[1][0][it][1][k]
    assert all(logs[0][1][k] == logs[1][1][k] for k in (0, 2, 3))
    assert any(not same_state(logs[0][0][it][0][1], logs[1][0][it][0][1]) for it in range(iters))   # (the seed does matter)
    e.close()


# --------------------------------------------------------------------------- 6. the doubt route
def test_doubtful_proposals_resolve_against_their_own_school():
    """Margins widened so that every proposal is recomputed by the host's libm (mpa_resolve_doubts): each one must be resolved with
    its own school's elite, seed and rows, or a K = 3 batch would part from the solo runs."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    K, N, iters = 3, 20, 6
    pairs = free_pairs(g, K, seed=1)
    seeds = [31, 32, 33]
    e1, e2 = pathfit.Engine(g), pathfit.Engine(g)
    try:
        e1.set_option("mpa_doubt_round_e15", 600_000_000_000_000)     # 0.6 > any |frac - 0.5|
        e1.set_option("mpa_doubt_log_e15", 10 ** 18)
        before = e1.L.pf_mpa_doubts_resolved(e1.h)
        b = pathfit.MPABatch(g, N, iters, seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], engine=e1, **KW)
        log, curves = run_batch_steps(b, iters)
        resolved = e1.L.pf_mpa_doubts_resolved(e1.h) - before
        assert resolved > 0 and b.counters()[2] == resolved
    finally:
        e1.set_option("mpa_doubt_round_e15", -1)
        e1.set_option("mpa_doubt_log_e15", -1)
    for k, (s, t) in enumerate(pairs):                                # solo runs with the default margins (device arithmetic)
        check_solo_steps(lambda: pathfit.MPA(moved(g, s, t), N, iters, seed=seeds[k], engine=e2, **KW), k, iters, log, curves)
    e1.close()
    e2.close()


# --------------------------------------------------------------------------- 7. shared engine
def test_solo_mpa_and_batch_share_an_engine():
    """A solo MPA and an MPABatch on ONE Engine, stepped alternately, each equal to its own isolated run; after update_grid the
    batch refuses to step."""
    import pathfit
    from pathfit import PathfitError
    g, s0, t0 = gio.grid("fig7")
    K, N, iters = 3, 24, 6
    pairs = free_pairs(g, K, seed=4)
    seeds = [51, 52, 53]
    kwb = dict(seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    # isolated runs
    bi = pathfit.MPABatch(g, N, iters, **kwb)
    log_i, curves_i = run_batch_steps(bi, iters)
    mi = pathfit.MPA(g, 36, iters, seed=77, **KW)
    solo_i = []
    for it in range(1, iters + 1):
        mi.step(it)
        solo_i.append((state_of_solo(mi), best_of(mi)))
    # shared
    e = pathfit.Engine(g)
    m = pathfit.MPA(g, 36, iters, seed=77, engine=e, **KW)            # (solo set up first, batch created after it ...)
    b = pathfit.MPABatch(g, N, iters, engine=e, **kwb)
    for it in range(1, iters + 1):
        if it % 2:
            m.step(it); b.step(it)
        else:
            b.step(it); m.step(it)
        assert same_state(state_of_solo(m), solo_i[it - 1][0]) and best_of(m) == solo_i[it - 1][1], f"solo, iteration {it}"
        st = state_of_batch(b)
        for k in range(K):
            assert same_state(st[k], log_i[it - 1][0][k]) and best_of(b.school(k)) == log_i[it - 1][1][k], f"school {k}, iteration {it}"
    assert [list(b.school(k).convergence_curve_data) for k in range(K)] == curves_i
    assert list(m.convergence_curve_data) == list(mi.convergence_curve_data)
    e.update_grid(g)
    with pytest.raises(PathfitError, match="replaced grid"):
        b.step(1)
    b.close()
    e.close()


# --------------------------------------------------------------------------- 8. overflow
def test_path_cap_too_small_raises_and_returns_nothing_truncated():
    """Rows just long enough for the initial paths: the first rebuilt or detoured path that needs more is counted on the device
    (the engine's ordinary status 3 route) and step() raises instead of returning anything."""
    import pathfit
    g, _, _ = gio.grid("fig7")
    pairs = free_pairs(g, 6, seed=1)
    seeds = [100 + k for k in range(6)]
    kw = dict(seeds=seeds, starts=[p[0] for p in pairs], targets=[p[1] for p in pairs], **KW)
    e = pathfit.Engine(g)
    ref = pathfit.MPABatch(g, 30, 12, engine=e, **kw)
    cap = int(ref.d_len.download().max())                            # the longest initial path of the six schools
    ref.close()
    with pytest.raises(RuntimeError, match="capacity overflow"):
        pathfit.MPABatch(g, 30, 12, engine=e, path_cap=cap - 1, **kw)   # an initial path does not fit: refused at once
    small = pathfit.MPABatch(g, 30, 12, engine=e, path_cap=cap, **kw)
    assert small.path_cap == cap
    with pytest.raises(RuntimeError, match=r"capacity overflow on \d+ predators \(path_cap=%d\)" % cap):
        small.solve_path_planning()                                  # a FADs detour through a random cell needs more than that
    assert small.counters()[1] > 0 and small.counters()[0]["overflow_agents"] > 0
    e.close()


# --------------------------------------------------------------------------- 9. K = 1
def test_one_school_is_solo_mpa():
    import pathfit
    g, _, _ = gio.grid("fig7")
    b = pathfit.MPABatch(g, 40, 9, seeds=[13], **KW)                  # starts / targets default to the grid's markers
    m = pathfit.MPA(g, 40, 9, seed=13, **KW)
    res, want = b.solve_path_planning(), m.solve_path_planning()
    assert len(res) == 1 and res[0][0] == want[0] and bits(res[0][1:]).tolist() == bits(want[1:]).tolist()
    assert b.school(0).convergence_curve_data == m.convergence_curve_data
    assert same_state(state_of_solo(m), state_of_batch(b)[0])
    assert b.school(0).start_node == m.start_node and b.school(0).target_node == m.target_node
    assert b.school(0).order.tolist() == m.order.tolist()
    assert [(p["path"].cells.tolist(), p["turns"], bits([p["length"], p["safety_penalty"], p["diag_penalty"], p["fitness"]]).tolist())
            for p in b.school(0).population] == \
           [(p["path"].cells.tolist(), p["turns"], bits([p["length"], p["safety_penalty"], p["diag_penalty"], p["fitness"]]).tolist())
            for p in m.population]
