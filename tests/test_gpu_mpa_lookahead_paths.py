"""The rare paths of the MPA look-ahead on the device, held to the model of tests/lookahead_cases.py: levels of
another phase than their leader's, depth 16 and its truncation, D N that is no multiple of a block, N = 1, the single-level
route, doubtful proposals and an overflow in a level ahead, the contract of pf_mpa_ahead_take, two MPAs on one Engine.

Every run is compared step by step with the look-ahead-off run on the same library, its curve and result with the oracle, and
the machinery with the model EXACTLY: the four totals of mpa_ahead_stats(), the mpa_sweep launches per step, the acceptance
history with its STALE marks.  No tolerance anywhere: bit for bit, or integer equality."""
import numpy as np
import pytest

import lookahead_cases as lc
import test_gpu_mpa_lookahead as base

pytestmark = pytest.mark.gpu

TOTALS = ("merged_sweeps", "levels_ahead", "served", "stale")
WIDE = (("mpa_doubt_round_e15", 600_000_000_000_000), ("mpa_doubt_log_e15", 10 ** 18))   # every proposal is doubtful


def policy_kw(policy):
    ad, rs = lc.POLICIES[policy]
    return dict(allow_diagonal_moves=bool(ad), restrict_diagonal_near_obstacle=bool(rs), **lc.KW)


def new_mpa(eng, run, path_cap=None, N=None):
    import pathfit
    g, _, _ = lc.grid(run.map)
    m = pathfit.MPA(g, N or run.N, run.K, engine=eng, seed=run.seed, **policy_kw(run.policy))
    if path_cap is not None:                                 # shorter rows: the population is built again in them
        m.path_cap = int(path_cap)
        m._init_population()
        assert m.path_cap == path_cap
    return m


def start(m):
    m._sort()
    slot, s0 = m._best_row()
    m._take_first(s0, m._fetch(slot))


def totals(st):
    return {k: st[k] for k in TOTALS}


def run(r, option, path_cap=None, wide=False, prune=True):
    """A whole run, one step at a time -> dict(snaps after every step, curve, result, stats, history, mpa_sweep launches per
    step, doubtful proposals resolved on the host per step, overflow_agents reported per step, error = (iteration, message) of
    the step that raised)."""
    import pathfit
    g, _, _ = lc.grid(r.map)
    eng = pathfit.Engine(g)
    try:
        eng.set_option("mpa_lookahead", option)
        eng.set_option("mpa_lookahead_always", r.always if option else 0)
        for name, v in WIDE if wide else ():
            eng.set_option(name, v)
        eng.set_option("mpa_prune", int(prune))
        out = dict(snaps=[], launches=[], resolved=[], ovf=[], error=None, cap=eng.mpa_ahead_stats()["cap"])
        eng.klog = []
        m = new_mpa(eng, r, path_cap)
        start(m)
        for it in range(1, r.K + 1):
            n0, d0 = len(eng.klog), eng.L.pf_mpa_doubts_resolved(eng.h)
            try:
                m.step(it)
            except RuntimeError as e:
                out["error"] = (it, str(e))
                break
            out["launches"].append(sum(f == "mpa_sweep" for f, _, _ in eng.klog[n0:]))
            out["resolved"].append(eng.L.pf_mpa_doubts_resolved(eng.h) - d0)
            out["ovf"].append(eng.counters()["overflow_agents"])
            out["snaps"].append(base.snapshot(m, m.order))
        out.update(curve=list(m.convergence_curve_data), result=m.result(), stats=eng.mpa_ahead_stats(), history=list(m.accept_history))
        return out
    finally:
        eng.set_option("mpa_lookahead", -1)
        eng.set_option("mpa_lookahead_always", 0)
        for name, _ in WIDE:
            eng.set_option(name, -1)
        eng.set_option("mpa_prune", 1)
        eng.close()


_OFF = {}


def off_run(r, path_cap=None, wide=False, prune=True):
    key = (r.map, r.N, r.K, r.seed, r.policy, path_cap, wide, prune)
    if key not in _OFF:
        _OFF[key] = run(r, 0, path_cap, wide, prune)
        st = _OFF[key]
        assert totals(st["stats"]) == dict.fromkeys(TOTALS, 0) and st["history"] == [] and set(st["launches"]) == {1}
    return _OFF[key]


def assert_is_oracle(r, got):
    o = lc.run_oracle(r)
    cols = lc.grid(r.map)[0].shape[1]
    assert got["curve"] == o.curve
    assert [a * cols + b for a, b in got["result"][0]] == list(o.best[0])
    assert got["result"][1:] == (o.best[1][0], int(o.best[1][1]), o.best[1][2], o.best[1][3], o.best[1][4])


def assert_run_is_model(r, on, off, sched):
    """on == off step by step, == oracle, and the machinery did exactly what the model says."""
    from pathfit.mpa import STALE
    base.assert_same_steps(on["snaps"], off["snaps"])
    assert on["curve"] == off["curve"] and on["result"] == off["result"]
    assert_is_oracle(r, on)
    assert totals(on["stats"]) == sched.totals, (on["stats"], sched.totals)
    assert on["launches"] == sched.launches
    assert on["history"] == sched.history
    assert [a for a in on["history"] if a != STALE] == lc.run_oracle(r).acc


# --------------------------------------------------------------------------------------------------------------- a, b
def test_door_levels_of_another_phase_are_served_and_accept():
    """Case a: iteration 17 (phase 2) is a level of the sweep led by 9 (phase 1) and changes 6 predators; iteration 33 (phase 3)
    is a level of the sweep led by 32 (phase 2).  Whatever a level took from level 0's view shows here."""
    r = lc.RUNS["door16"]
    sched = lc.run_schedule(r)
    assert sched.steps[16] == "served" and sched.steps[32] == "served"
    assert lc.run_oracle(r).acc[16] == 6
    on = run(r, r.cap)
    assert_run_is_model(r, on, off_run(r), sched)


@pytest.mark.parametrize("policy", ["4", "cut"])
def test_door_under_the_other_move_policies(policy):
    """Case b: 4-connected moves, and corner cutting allowed.  Both runs have a quiet pair before K at seed 0 (pinned in
    tests/test_lookahead_cases.py), so no other seed had to be looked for."""
    r = lc.policy_run(policy)
    sched = lc.run_schedule(r)
    assert sched.totals["served"] > 0 and sched.totals["stale"] > 0
    on = run(r, r.cap)
    assert_run_is_model(r, on, off_run(r), sched)


# ------------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("name,option,cap", [("open65", 99, 16), ("open5", 99, 16), ("open1", 99, 16), ("open5", -1, 8),
                                             ("open5_cap2", 2, 2), ("open5_cap1", 1, 1)])
def test_open12_depth_16_truncation_and_the_option(name, option, cap):
    """Case c: nothing ever accepts, so every level is served and every sweep after the first step has full depth: 16 (the
    option's 99 clamped), truncated by the run's end; D N = 1040 / 80 / 16; the default; 2; and 1, where every step is
    pf_mpa_iter_ahead with one level."""
    r = lc.RUNS[name]
    o = lc.run_oracle(r)
    sched = lc.schedule(o.acc, cap, r.K)
    on = run(r, option)
    assert on["cap"] == cap                                  # the clamp (99 -> 16) and the default (-1 -> 8)
    assert_run_is_model(r, on, off_run(r), sched)
    assert on["stats"]["levels_ahead"] == on["stats"]["served"]          # no level beyond iteration K was swept
    if cap == 1:
        assert on["stats"]["merged_sweeps"] == 0 and on["stats"]["served"] == 0 and on["launches"] == [1] * r.K


# ------------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("name", ["fig7_s0_16", "fig7_s0_5", "fig7_s1_16", "fig7_s1_5"])
def test_fig7_looking_ahead_after_every_iteration(name):
    """Case d: "mpa_lookahead_always" -- most levels are discarded, and the totals are the model's."""
    r = lc.RUNS[name]
    sched = lc.run_schedule(r)
    on = run(r, r.cap)
    assert_run_is_model(r, on, off_run(r), sched)


# ------------------------------------------------------------------------------------------------------------------- e
def test_doubtful_proposals_in_levels_ahead_take_the_host_route():
    """Case e: with the doubt margins widened every proposal is recomputed on the host, those of the levels ahead too: a merged
    sweep resolves more than N of them (pf_mpa_doubts_resolved, the handle's counter, read around every step)."""
    r = lc.RUNS["door16"]
    sched = lc.run_schedule(r)
    on, off = run(r, r.cap, wide=True), off_run(r, wide=True)
    assert_run_is_model(r, on, off, sched)
    lead = [n for n, s in zip(on["resolved"], sched.steps) if "lead" in s]
    assert len(lead) == 6 and max(lead) > r.N, lead             # more than one level's worth: levels >= 1 were resolved too
    assert sum(on["resolved"]) >= sum(off["resolved"])         # (every iteration's proposals are resolved at least once)
    assert all(n == 0 for n, s in zip(on["resolved"], sched.steps) if s == "served")
    assert sum(off["resolved"]) > 0 and max(off["resolved"]) <= r.N


# ------------------------------------------------------------------------------------------------------------------- f
def test_overflow_in_a_level_ahead():
    """Case f: door, seed 0, rows of 36 cells.  Iteration 24 is level 1 of the sweep led by 23 and has a 37-cell row: the leader's
    step reports no overflow, the take of 24 finds the level stale, and the sweep of 24 on its own raises what the run without
    look-ahead raises.  Bound pruning is off in both runs ("mpa_prune" 0: it changes no result): the 37-cell row is a candidate the
    oracle computes and the pruning would skip, and a search that never runs cannot overflow."""
    f = lc.find_overflow_case()
    assert f is not None
    r = lc.Run(f.map, f.N, f.K, f.seed, f.cap, 0, "8")
    sched = lc.schedule(lc.run_oracle(r).acc, f.cap, f.K, overflow_at=f.at)
    on, off = run(r, f.cap, path_cap=f.path_cap, prune=False), off_run(r, path_cap=f.path_cap, prune=False)
    assert off["error"] is not None and off["error"][0] == f.at, off["error"]
    assert on["error"] == off["error"] and "overflow" in on["error"][1]
    assert len(on["snaps"]) == len(off["snaps"]) == f.at - 1
    base.assert_same_steps(on["snaps"], off["snaps"])
    assert on["curve"] == off["curve"] == lc.run_oracle(r).curve[:f.at]
    assert totals(on["stats"]) == sched.totals and sched.steps[-1] == "stale+overflow"
    # (the step that raises has swept and noted its acceptances before the overflow is looked at)
    assert on["launches"] == sched.launches[:-1] and on["history"][:-1] == sched.history and len(on["history"]) == len(sched.history) + 1
    assert on["ovf"] == [0] * (f.at - 1) and sched.steps[f.leader - 1] == "lead(16)"      # the leader's own step included


# ------------------------------------------------------------------------------------------------------------------- g
def _pop(m):
    return m.d_cells.download(), m.d_len.download(), m.d_stats.download(), m.d_order.download()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _lead(m, it, depth, phases=None):
    from pathfit.mpa import cf_and_phase
    e = m.engine
    m._sort()
    e.mpa_pick_elite(m.path_cap, m.d_cells, m.d_len, m.d_stats, m.d_order)
    lv = [(cf_and_phase(it + d, m.num_iterations)[1], cf_and_phase(it + d, m.num_iterations)[0], it + d) for d in range(depth)]
    if phases:
        lv = [(p, cf, i) for p, (_, cf, i) in zip(phases, lv)]
    return e.mpa_iter_ahead(lv, m.seed, m.n_local, m.path_cap, m.d_cells, m.d_len, m.d_stats, m.d_gidx, m.d_order, m._el_cells.ptr, -1,
                            m._el_stats.ptr, *m._own_rows)


def test_the_contract_of_take_and_the_argument_errors():
    """Case g on open12, through Engine.mpa_iter_ahead / mpa_ahead_take directly."""
    import pathfit
    from pathfit._lib import PathfitError
    r = lc.RUNS["open5"]
    g, _, _ = lc.grid(r.map)
    eng = pathfit.Engine(g)
    try:
        eng.set_option("mpa_lookahead", 16)
        m = new_mpa(eng, r)
        pop = (m.d_order, m.d_cells, m.d_len, m.d_stats)
        st = lambda: totals(eng.mpa_ahead_stats())
        assert _lead(m, 1, 4) == 0 and st() == dict(merged_sweeps=1, levels_ahead=3, served=0, stale=0)
        before = _pop(m)
        assert eng.mpa_ahead_take(3, *pop) == -1 and st()["stale"] == 1          # level 1 waits for iteration 2, not 3
        assert eng.mpa_ahead_take(2, *pop) == -1 and st()["stale"] == 1          # nothing is waiting any more
        assert _same(_pop(m), before)
        assert _lead(m, 2, 4) == 0 and st()["merged_sweeps"] == 2
        assert eng.mpa_ahead_take(3, *pop) == 0 and st()["served"] == 1          # (the right take is served)
        stale = 1
        for k, src in enumerate((3, 0, 1, 2)):                                   # another list / cells / lengths / stats buffer
            other = list(pop)
            other[k] = eng.put(before[src])
            assert _lead(m, 4, 4) == 0
            assert eng.mpa_ahead_take(5, *other) == -1 and st()["stale"] == stale + 1
            assert eng.mpa_ahead_take(5, *pop) == -1 and st()["stale"] == stale + 1
            stale += 1
        assert _lead(m, 4, 4) == 0
        eng.mpa_ahead_drop()
        assert eng.mpa_ahead_take(5, *pop) == -1 and st()["stale"] == stale      # dropped: nothing waiting, nothing counted
        assert _same(_pop(m), before) and st()["served"] == 1
        # argument errors come before any launch
        s0 = st()
        eng.klog = []
        for depth, phases in ((0, None), (17, None), (2, (0, 1)), (2, (1, 4))):
            with pytest.raises(PathfitError, match="bad arguments"):
                _lead(m, 6, depth, phases)
        assert st() == s0 and _same(_pop(m), before)
        assert [f for f, _, _ in eng.klog if f == "mpa_sweep"] == []
    finally:
        eng.set_option("mpa_lookahead", -1)
        eng.close()


def test_a_refused_take_leaves_a_level_that_would_have_accepted_unapplied():
    """Case g, sharpened: on door the level waiting for iteration 17 changes 6 predators when it is applied.  Asked for as
    iteration 18 it is refused, the population stays bit for bit what it was, and the run goes on as the run without look-ahead."""
    import pathfit
    r = lc.RUNS["door16"]
    off = off_run(r)
    g, _, _ = lc.grid(r.map)
    eng = pathfit.Engine(g)
    try:
        eng.set_option("mpa_lookahead", 16)
        m = new_mpa(eng, r)
        start(m)
        snaps = []
        for it in range(1, 17):
            m.step(it)
            snaps.append(base.snapshot(m, m.order))
        st = eng.mpa_ahead_stats()
        assert m._ahead_left == 8                                                # levels 17 .. 24 of the sweep led by 9
        before = _pop(m)
        assert eng.mpa_ahead_take(18, m.d_order, m.d_cells, m.d_len, m.d_stats) == -1
        assert eng.mpa_ahead_stats()["stale"] == st["stale"] + 1 and _same(_pop(m), before)
        for it in range(17, r.K + 1):
            m.step(it)
            snaps.append(base.snapshot(m, m.order))
        base.assert_same_steps(snaps, off["snaps"])
        assert list(m.convergence_curve_data) == off["curve"] and m.result() == off["result"]
    finally:
        eng.set_option("mpa_lookahead", -1)
        eng.close()


# ------------------------------------------------------------------------------------------------------------------- h
def _cand(m):
    """The candidate rows a caller may read between steps (what ShardedMPA and the tests do)."""
    cl = m.d_cand_len.download()
    cc = m.d_cand_cells.download()
    return (cl, m.d_cand_stats.download(), m.d_c2_len.download(), m.d_status.download()) + tuple(cc[i, :cl[i]].copy() for i in range(len(cl)))


def test_two_mpas_on_one_engine():
    """Case h: A (door, 20 predators) and B (door, 33 predators, rows of 200 cells) on one Engine, cap 8, three iterations
    each in turn.  The handle holds one MPA set-up and one set of level buffers: each instance sets itself up again when the
    other has stepped, which drops the levels (STALE in the history exactly where the model puts it) -- and B's merged sweeps
    reallocate the level buffers A's candidate rows were views into, so A's rows must have moved to A's own buffers by then.
    Then the map is set again (the same one), both are rebuilt on the Engine, and run to the end."""
    import pathfit
    rA = lc.Run("door", 20, 48, 0, 8, 0, "8")
    rB = rA._replace(N=33)
    PB = 200
    offA, offB = off_run(rA), off_run(rB, path_cap=PB)
    accA, accB = lc.run_oracle(rA).acc, lc.run_oracle(rB).acc
    g, _, _ = lc.grid("door")
    eng = pathfit.Engine(g)
    try:
        eng.set_option("mpa_lookahead", 8)
        eng.klog = []
        done = dict.fromkeys(TOTALS, 0)
        for upto in (24, 48):
            A, B = new_mpa(eng, rA), new_mpa(eng, rB, path_cap=PB)
            assert A.path_cap != B.path_cap
            ms = {"A": A, "B": B}
            start(A), start(B)
            order = [x for x in lc.interleave(48) if x[1] <= upto]
            h = lc.Handle(8)
            model = {"A": lc.Instance(h, accA, 48), "B": lc.Instance(h, accB, 48)}
            snaps, launches, held = {"A": [], "B": []}, {"A": [], "B": []}, {}
            for who, it in order:
                m, other = ms[who], ms["B" if who == "A" else "A"]
                n0 = len(eng.klog)
                m.step(it)
                model[who].step(it)
                launches[who].append(sum(f == "mpa_sweep" for f, _, _ in eng.klog[n0:]))
                snaps[who].append(base.snapshot(m, m.order))
                held[who] = _cand(m)
                if other is not m and ("B" if who == "A" else "A") in held:      # the other's rows are still what they were
                    assert _same(_cand(other), held["B" if who == "A" else "A"]), (who, it)
            for who, off in (("A", offA), ("B", offB)):
                base.assert_same_steps(snaps[who], off["snaps"][:upto])
                assert list(ms[who].convergence_curve_data) == off["curve"][:upto + 1]
                assert list(ms[who].accept_history) == model[who].hist
                assert launches[who] == model[who].launches
                assert "served" in model[who].steps and "stale+single" in model[who].steps
            now = totals(eng.mpa_ahead_stats())
            assert {k: now[k] - done[k] for k in TOTALS} == h.totals()
            done = now
            if upto == 24:
                eng.update_grid(g)                                               # mid-run: the set-up and the levels are gone
        assert ms["A"].result() == offA["result"] and ms["B"].result() == offB["result"]
    finally:
        eng.set_option("mpa_lookahead", -1)
        eng.close()
