"""The cases of tests/lookahead_cases.py are what tests/test_gpu_mpa_lookahead_paths.py needs them to be (no GPU): the
oracle's acceptance lists, the model's schedule for every row of the run table, and the property that makes each case worth
running on the device.  A change of the oracle, of bench.py's MPA parameters or of the look-ahead policy shows here first."""
import pytest

import lookahead_cases as lc

S, L16, SV, ST = "single", "lead(16)", "served", "stale+single"
DOOR_ACC = [0, 0, 0, 1, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 8, 2, 0, 1, 0, 0, 0, 0, 1, 8, 7, 3, 1] + [0] * 18
DOOR_STEPS = [S, L16, SV, SV, ST, L16, SV, ST, L16] + [SV] * 8 + [ST, S, S, L16, ST, L16, SV, SV, SV, ST, S, S, S, S, L16] + [SV] * 15 + [S]
OPEN48_STEPS = [S, L16] + [SV] * 15 + [L16] + [SV] * 15 + ["lead(15)"] + [SV] * 14
OPEN40_STEPS = [S, L16] + [SV] * 15 + [L16] + [SV] * 15 + ["lead(7)"] + [SV] * 6


def test_door_acceptance_and_hand_derivation():
    """The hand derivation of the issue (6 merged sweeps, 90 levels swept ahead, 29 served, 5 stale, leaders 2, 6, 9, 21, 23,
    32) and the model agree."""
    r = lc.RUNS["door16"]
    o = lc.run_oracle(r)
    assert o.acc == DOOR_ACC and len(DOOR_ACC) == r.K == 48
    s = lc.run_schedule(r)
    assert s.steps == DOOR_STEPS
    assert s.totals == dict(merged_sweeps=6, levels_ahead=90, served=29, stale=5)
    assert s.leaders == [2, 6, 9, 21, 23, 32]
    assert s.launches == [0 if x == SV else 1 for x in DOOR_STEPS]
    from pathfit.mpa import STALE
    assert [a for a in s.history if a != STALE] == DOOR_ACC
    assert [i + 1 - k for k, i in enumerate(j for j, a in enumerate(s.history) if a == STALE)] == [5, 8, 18, 22, 27]


def test_door_serves_levels_of_another_phase_that_accept():
    r = lc.RUNS["door16"]
    o, s = lc.run_oracle(r), lc.run_schedule(r)
    served = lc.served_iterations(s)
    assert 17 in served and 33 in served
    # iteration 17, the first of phase 2, is a level of the sweep led by 9 (phase 1) and accepts 6 predators
    assert (lc.leader_of(s, 17), lc.phase_of(9, 48), lc.phase_of(17, 48), o.acc[16]) == (9, 1, 2, 6)
    # iteration 33, the first of phase 3, is a level of the sweep led by 32 (phase 2)
    assert (lc.leader_of(s, 33), lc.phase_of(32, 48), lc.phase_of(33, 48)) == (32, 2, 3)
    assert any(o.acc[it - 1] > 0 and lc.phase_of(it, 48) != lc.phase_of(lc.leader_of(s, it), 48) for it in served)
    # a leader whose own level accepts: every level behind it is stale
    assert s.steps[20] == L16 and o.acc[20] == 1 and s.steps[21] == ST


@pytest.mark.parametrize("name,steps,totals", [
    ("open65", OPEN48_STEPS, (3, 44, 44, 0)), ("open5", OPEN48_STEPS, (3, 44, 44, 0)), ("open1", OPEN40_STEPS, (3, 36, 36, 0)),
    ("open5_cap2", [S] + ["lead(2)", SV] * 23 + [S], (23, 23, 23, 0)), ("open5_cap1", [S] * 48, (0, 0, 0, 0))])
def test_open12_schedules(name, steps, totals):
    r = lc.RUNS[name]
    o, s = lc.run_oracle(r), lc.run_schedule(r)
    assert o.acc == [0] * r.K                               # nothing ever accepts: every level is served
    assert s.steps == steps and len(steps) == r.K
    assert tuple(s.totals[k] for k in ("merged_sweeps", "levels_ahead", "served", "stale")) == totals
    assert s.totals["levels_ahead"] == s.totals["served"]   # no level beyond iteration K is ever swept
    if r.cap == 16:
        assert L16 in s.steps                               # a sweep of depth 16 ...
        last = [x for x in s.steps if x.startswith("lead")][-1]
        assert last == "lead(%d)" % (r.K - 33)              # ... and one truncated by the run's end (led by iteration 34)


def test_open12_shapes():
    r = lc.RUNS["open65"]
    assert (16 * r.N) % 256 != 0 and (16 * r.N) % 64 != 0 and r.N % 64 != 0
    assert lc.RUNS["open1"].N == 1
    # the option's clamp and default, as the model sees them
    assert lc.Handle(99).cap == 16 and lc.Handle(-1).cap == 8 and lc.Handle(2).cap == 2


def test_fig7_quiet_tails():
    assert lc.oracle_run("fig7", 70, 48, 0).acc[20:] == [0] * 28 and lc.oracle_run("fig7", 70, 48, 0).acc[19] > 0
    assert lc.oracle_run("fig7", 70, 48, 1).acc[21:] == [0] * 27 and lc.oracle_run("fig7", 70, 48, 1).acc[20] > 0
    assert lc.oracle_run("fig7", 70, 60, 2).acc[29:] == [0] * 31 and lc.oracle_run("fig7", 70, 60, 2).acc[28] > 0


@pytest.mark.parametrize("name,totals", [("fig7_s0_16", (12, 176, 26, 10)), ("fig7_s0_5", (16, 62, 22, 10)),
                                         ("fig7_s1_16", (12, 175, 26, 10)), ("fig7_s1_5", (16, 61, 22, 10))])
def test_fig7_always_discards_most_levels(name, totals):
    s = lc.run_schedule(lc.RUNS[name])
    assert tuple(s.totals[k] for k in ("merged_sweeps", "levels_ahead", "served", "stale")) == totals
    assert s.totals["levels_ahead"] > 2 * s.totals["served"] and s.steps[0].startswith("lead")
    assert sum(s.launches) == 48 - s.totals["served"]


@pytest.mark.parametrize("policy,seed,totals", [("4", 0, (8, 114, 25, 6)), ("cut", 0, (5, 69, 36, 3))])
def test_door_under_the_other_move_policies(policy, seed, totals):
    """Both policies' runs at seed 0 have a quiet pair before K, so seed 0 it is (the search is first_quiet_seed)."""
    assert lc.first_quiet_seed("door", 20, 48, policy) == seed == lc.POLICY_SEEDS[policy]
    r = lc.policy_run(policy)
    o, s = lc.run_oracle(r), lc.run_schedule(r)
    assert o.acc != DOOR_ACC and sum(o.acc) > 0
    assert tuple(s.totals[k] for k in ("merged_sweeps", "levels_ahead", "served", "stale")) == totals
    assert any(o.acc[it - 1] > 0 for it in lc.served_iterations(s))     # a served level accepts


def test_overflow_in_a_level_ahead_exists():
    """door, seed 0, rows of 36 cells: iteration 22's longest row is 36 cells, iteration 24's is 37, and the model serves 24
    from the sweep led by 23."""
    f = lc.find_overflow_case()
    assert f == lc.Overflow("door", 20, 48, 0, 16, 36, 24, 23)
    o = lc.oracle_run(f.map, f.N, f.K, f.seed)
    assert o.longest[0] <= f.path_cap and max(o.longest[1:f.at]) <= f.path_cap < o.longest[f.at]
    s = lc.schedule(o.acc, f.cap, f.K, overflow_at=f.at)
    assert s.steps[f.leader - 1] == L16 and s.steps[-1] == "stale+overflow" and len(s.steps) == f.at
    base = lc.schedule(o.acc, f.cap, f.K)
    assert s.steps[:-1] == base.steps[:f.at - 1]
    assert s.totals["stale"] == sum(x.startswith("stale") for x in s.steps)


def test_two_instances_on_one_handle():
    """A (door, 20 predators) and B (door, 33 predators), cap 8, three iterations each in turn: a level survives only inside a
    burst, and the first step of a burst that still had levels waiting finds them gone."""
    a, b = lc.oracle_run("door", 20, 48, 0), lc.oracle_run("door", 33, 48, 0)
    A, B, totals = lc.schedule_two(a.acc, b.acc, 8, 48)
    assert len(A.steps) == len(B.steps) == 48
    for m in (A, B):
        assert "served" in m.steps and "stale+single" in m.steps
        # a stale mark only on the first iteration of a burst, or after an accepting level inside one
        for it, x in enumerate(m.steps, 1):
            if x.startswith("stale") and (it - 1) % 3 != 0:
                assert m.acc[it - 2] > 0, it
    # the other instance's set-up takes the levels away without counting a stale level: fewer counted than marked
    from pathfit.mpa import STALE
    assert totals["stale"] < A.hist.count(STALE) + B.hist.count(STALE)
    assert totals["served"] == A.steps.count("served") + B.steps.count("served")
