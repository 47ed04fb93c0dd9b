"""The MPA look-ahead (pf_mpa_iter_ahead / pf_mpa_ahead_take) is exact: a run with it computes, step by step,
what a run without it computes, whether the levels swept ahead are served or have to be thrown away."""
import os
import sys

import numpy as np
import pytest

import golden_io as gio

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

pytestmark = pytest.mark.gpu

# fig7 (20 x 20), 70 predators (more than one wavefront of them), 30 iterations, bench.py's MPA parameters.  The oracle's
# acceptance counts (chosen on the CPU with scripts/probe_mpa_acceptance.py):
#   seed 0: ... 4, 0, 0, 1, 24, 20, 17, 5, 1, 0, 0, ...   a quiet pair inside phase 1 whose look-ahead ends in a stale level, then
#           the quiet tail from iteration 16;
#   seed 1: ... 2, 0, 27, ... 7, 0, 1, 0, 0, ...          single quiet iterations whose first level ahead is stale, tail from 22.
GRID, N, K = "fig7", 70, 30
KW = dict(FADs_rate=0.2, P_const=0.5, levy_beta=2.0, turn_penalty_factor=0.1, safety_penalty_factor=0.8, min_safe_distance=1.8,
          diagonal_obstacle_penalty=100.0)
OKW = dict(FADs_rate=0.2, P_const=0.5, levy_beta=2.0, w_turn=0.1, w_safe=0.8, min_safe=1.8, diag_pen=100.0)
SEEDS = (0, 1)
_REF = {}


def oracle_run(seed):
    """(acceptance counts per iteration, curve, best (cells, stats)) of the oracle's run -- computed once per seed."""
    if seed not in _REF:
        import pf_loops
        import pf_oracle as po
        from probe_mpa_acceptance import acceptance_rows
        g, s, t = gio.grid(GRID)
        ref = pf_loops.MpaOracle(po.Oracle(g), s, t, N, K, seed=seed, **OKW)
        rows = acceptance_rows(ref)
        _REF[seed] = ([r[2] for r in rows], list(ref.curve), ref.best)
    return _REF[seed]


def snapshot(m, order):
    cells, lens = m.d_cells.download(), m.d_len.download()
    return dict(lens=lens, stats=m.d_stats.download(), order=np.asarray(order).copy(), rows=[cells[i, :lens[i]].copy() for i in range(len(lens))],
                best=(list(m.best_path_overall), m.best_path_length_overall, m.best_path_turns_overall, m.best_safety_penalty_overall,
                      m.best_diag_penalty_overall, m.best_fitness_overall))


def run(seed, lookahead, always=0, sharded=False):
    """A whole run, one step at a time -> (snapshots after every step, curve, result, look-ahead statistics, acceptance history,
    mpa_sweep launches logged per step)."""
    import pathfit
    from pathfit.dist import Comm, ShardedMPA
    g, _, _ = gio.grid(GRID)
    eng = pathfit.Engine(g)
    try:
        eng.set_option("mpa_lookahead", lookahead)
        eng.set_option("mpa_lookahead_always", always)
        snaps, launches = [], []
        eng.klog = []
        if sharded:
            sm = ShardedMPA(Comm(None), lambda n: pathfit.MPA(g, N, K, engine=eng, seed=seed, n_local=n, **KW), N)
            m = sm.local
            sm._resort()
            _, r, slot, s = sm._best_row()
            m._take_first(s, sm._fetch(r, slot))
            for it in range(1, K + 1):
                n0 = len(eng.klog)
                sm.step(it)
                _, r, slot, s = sm._best_row()
                m._take(s, sm._fetch(r, slot))
                launches.append(sum(f == "mpa_sweep" for f, _, _ in eng.klog[n0:]))
                snaps.append(snapshot(m, sm.gorder))
        else:
            m = pathfit.MPA(g, N, K, engine=eng, seed=seed, **KW)
            m._sort()
            slot, s0 = m._best_row()
            m._take_first(s0, m._fetch(slot))
            for it in range(1, K + 1):
                n0 = len(eng.klog)
                m.step(it)
                launches.append(sum(f == "mpa_sweep" for f, _, _ in eng.klog[n0:]))
                snaps.append(snapshot(m, m.order))
        return snaps, list(m.convergence_curve_data), m.result(), eng.mpa_ahead_stats(), list(m.accept_history), launches
    finally:
        eng.set_option("mpa_lookahead", -1)
        eng.set_option("mpa_lookahead_always", 0)
        eng.close()


_OFF = {}


def off_run(seed):
    if seed not in _OFF:
        _OFF[seed] = run(seed, 0)
    return _OFF[seed]


def assert_same_steps(a, b):
    assert len(a) == len(b)
    for it, (x, y) in enumerate(zip(a, b), 1):
        assert np.array_equal(x["lens"], y["lens"]), it
        assert np.array_equal(x["stats"], y["stats"]), it
        assert np.array_equal(x["order"], y["order"]), it
        assert all(np.array_equal(p, q) for p, q in zip(x["rows"], y["rows"])), it
        assert x["best"] == y["best"], it


def assert_is_oracle(seed, curve, result):
    _, ref_curve, best = oracle_run(seed)
    assert curve == ref_curve
    assert [r * 20 + c for r, c in result[0]] == list(best[0])
    assert result[1:] == (best[1][0], int(best[1][1]), best[1][2], best[1][3], best[1][4])


def quiet_pair_before_end(acc):
    return any(acc[i] == 0 and acc[i + 1] == 0 for i in range(len(acc) - 2))


@pytest.mark.parametrize("seed", SEEDS)
def test_lookahead_on_equals_off_and_oracle(seed):
    acc, _, _ = oracle_run(seed)
    assert quiet_pair_before_end(acc), acc                # the run does reach quiet iterations before K
    off = off_run(seed)
    on = run(seed, 8)
    assert_same_steps(on[0], off[0])
    assert on[1] == off[1] and on[2] == off[2]
    assert_is_oracle(seed, on[1], on[2])
    from pathfit.mpa import STALE
    assert [a for a in on[4] if a != STALE] == acc         # the device's acceptance counts are the oracle's
    st, st0 = on[3], off[3]
    assert st["served"] >= 1 and st["merged_sweeps"] >= 1 and st["levels_ahead"] >= st["served"]
    assert st0["served"] == 0 and st0["merged_sweeps"] == 0 and off[5] == [1] * K and off[4] == []
    assert sum(on[5]) == K - st["served"] and set(on[5]) <= {0, 1}   # a served step logs no sweep
    assert st["stale"] >= 1                                 # (both seeds have a quiet iteration followed by an accepting one)


@pytest.mark.parametrize("seed", SEEDS)
def test_lookahead_discard_path(seed):
    """Looking ahead after every iteration: most levels are thrown away, and nothing changes."""
    off = off_run(seed)
    on = run(seed, 3, always=1)
    assert_same_steps(on[0], off[0])
    assert on[1] == off[1] and on[2] == off[2]
    st = on[3]
    assert st["stale"] >= 3 and st["served"] >= 1, st
    assert st["levels_ahead"] > st["served"]


def test_lookahead_through_sharded_mpa_world_1():
    seed = SEEDS[0]
    off = off_run(seed)
    on = run(seed, 8, sharded=True)
    assert_same_steps(on[0], off[0])
    assert on[1] == off[1] and on[2] == off[2]
    assert on[3]["served"] >= 1
    assert_is_oracle(seed, on[1], on[2])


def test_lookahead_candidate_rows_and_drop():
    """After a served step m.d_cand_* / m.d_c2_* / m.d_status are that iteration's rows (as after a plain sweep), and dropping the
    look-ahead between steps (what a re-initialisation does) only costs the levels."""
    import pathfit
    seed = SEEDS[0]
    acc, _, _ = oracle_run(seed)
    g, _, _ = gio.grid(GRID)
    rows = {}
    for la in (0, 8):
        eng = pathfit.Engine(g)
        try:
            eng.set_option("mpa_lookahead", la)
            m = pathfit.MPA(g, N, K, engine=eng, seed=seed, **KW)
            out = []
            for it in range(1, K + 1):
                m.step(it)
                if la and it == 20:
                    m.drop_lookahead()
                cl = m.d_cand_len.download()
                cc = m.d_cand_cells.download()
                out.append((cl, [cc[i, :cl[i]].copy() for i in range(N)], m.d_cand_stats.download(), m.d_c2_len.download(),
                            m.d_status.download(), m.d_stats.download()))
            rows[la] = out
            if la:
                assert eng.mpa_ahead_stats()["served"] >= 2
        finally:
            eng.set_option("mpa_lookahead", -1)
            eng.close()
    for it, (x, y) in enumerate(zip(rows[0], rows[8]), 1):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]), it
        assert np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5]), it
        assert all(np.array_equal(p, q) for p, q in zip(x[1], y[1])), it
