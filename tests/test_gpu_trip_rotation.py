"""The rotated trip of the sorted-window pop loop (pf_astar_sw.h) changes nothing: a trip that sends no push to the
window and is followed by no refill issues the next trip's record load behind its own record stores and appends to the pool in
that load's shadow.  Every search below is compared with oracle/pf_oracle bit for bit -- cells, length, status and the pop / push /
examined counters -- on maps chosen for the ways rotated and unrotated trips follow each other:

  blocks48 / blocks64  seeded random blocks, a quarter of the cells: the everyday mixture;
  empty64              plateaus of equal f: full windows, window inserts in consecutive trips -- rotated and unrotated trips alternate
                       (run on the plain and on the plateau kernels);
  serpentine64         corridors one cell wide: one or two heads a trip and a refill nearly every trip -- a rotated issue is followed
                       at once by a trip that starts at the top;
  fans                 one start, every sixth reachable cell as a target: the target is popped at every place of the pop sequence,
                       so also in the trip right after a rotated one;
  step caps            a rotated trip is by construction not the last one, so a cap ends the search in the trip that FOLLOWS one
                       (whose records were requested a trip early) or in a trip from the top: caps of many residues.

The closed-set variants run on the sequential loop (astar_settle 0): its counters are the reference's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NPAIRS = 200


def blocks(n, seed):
    rnd = np.random.default_rng(seed)
    g = np.zeros((n, n), np.uint8)
    while (g == 1).mean() < 0.25:
        r, c = (int(v) for v in rnd.integers(0, n, 2))
        h, w = (int(v) for v in rnd.integers(1, 5, 2))
        g[r:r + h, c:c + w] = 1
    return g


def serpentine(n):
    g = np.zeros((n, n), np.uint8)
    for k, r in enumerate(range(1, n, 2)):
        g[r, :] = 1
        g[r, n - 1 if k % 2 == 0 else 0] = 0
    return g


MAPS = {"blocks48": lambda: blocks(48, 48), "blocks64": lambda: blocks(64, 64), "empty64": lambda: np.zeros((64, 64), np.uint8),
        "serpentine64": lambda: serpentine(64)}
_WORLD = {}


def world(name):
    """(engine, oracle, map) -- one per map for the whole module."""
    if name not in _WORLD:
        from pathfit.engine import Engine
        import pf_oracle as po
        g = MAPS[name]()
        _WORLD[name] = (Engine(g), po.Oracle(g), g)
    return _WORLD[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e, _, _ in _WORLD.values():
        e.set_option("astar_settle", -1); e.set_option("plateau_kernels", -1); e.set_option("astar_step_cap", 0)
        e.close()
    _WORLD.clear()


def pairs_with_a_path(o, g, variant, n, seed):
    """n seeded pairs of free cells that the oracle connects by a path of at least two cells, with its answers."""
    rnd = np.random.default_rng(seed)
    free = np.flatnonzero(g.reshape(-1) != 1)
    S, T, want = [], [], []
    while len(S) < n:
        s, t = (int(v) for v in rnd.choice(free, 2))
        w = o.astar(s, t, None, variant)
        if len(w[0]) > 1:
            S.append(s); T.append(t); want.append(w)
    return S, T, want


def assert_searches(e, variant, S, T, want, where, cap=None):
    paths, st, cnt = e.astar_host(variant, S, T, None, path_cap=e.R * e.C, want_counters=True)
    assert len(paths) == len(want)
    for i, (wp, ost) in enumerate(want):
        tag = (where, variant, i, S[i], T[i])
        assert st[i] == ost[5], (tag, st[i], ost[5])
        assert len(paths[i]) == len(wp) and np.array_equal(paths[i], wp), tag
        assert (cnt[i, 0], cnt[i, 1], cnt[i, 3]) == (ost[0], ost[1], ost[4]), (tag, cnt[i], ost)
        if cap is not None and ost[5] == 2:
            assert cnt[i, 0] == cap and len(wp) == 0, tag


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", ["blocks48", "blocks64", "serpentine64"])
def test_searches_equal_oracle(name, variant):
    e, o, g = world(name)
    e.set_option("astar_settle", 0)
    S, T, want = pairs_with_a_path(o, g, variant, NPAIRS, 100 + variant)
    assert max(len(w[0]) for w in want) > g.shape[0]
    assert_searches(e, variant, S, T, want, name)


@pytest.mark.parametrize("plateau", [0, 1])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_empty_map_equals_oracle(variant, plateau):
    e, o, g = world("empty64")
    e.set_option("astar_settle", 0)
    e.set_option("plateau_kernels", plateau)
    S, T, want = pairs_with_a_path(o, g, variant, NPAIRS, 200 + variant)
    assert_searches(e, variant, S, T, want, ("empty64", plateau))


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", ["blocks64", "empty64"])
def test_target_fans_equal_oracle(name, variant):
    """One start, every sixth reachable cell (in cell order) as the target: the search stops at every place of one pop sequence."""
    e, o, g = world(name)
    e.set_option("astar_settle", 0)
    e.set_option("plateau_kernels", -1)
    free = np.flatnonzero(g.reshape(-1) != 1)
    s = int(free[len(free) // 3])
    S, T, want = [], [], []
    for t in free[variant::6]:
        w = o.astar(s, int(t), None, variant)
        if len(w[0]) > 1:
            S.append(s); T.append(int(t)); want.append(w)
    assert len(S) >= NPAIRS
    assert_searches(e, variant, S, T, want, ("fan", name))


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_step_caps_equal_oracle(variant):
    """24 connected pairs under fourteen caps: the capped searches stop with the reference's status and counters (pops == cap),
    the others return the reference's path."""
    import pf_oracle as po
    e, o, g = world("blocks64")
    e.set_option("astar_settle", 0)
    S, T, _ = pairs_with_a_path(o, g, variant, 24, 300 + variant)
    capped = 0
    try:
        for cap in (1, 6, 7, 8, 13, 20, 27, 34, 41, 55, 101, 250, 333, 1001):
            e.set_option("astar_step_cap", cap); po.set_step_cap(cap)
            want = [o.astar(s, t, None, variant) for s, t in zip(S, T)]
            capped += sum(int(w[1][5] == 2) for w in want)
            assert_searches(e, variant, S, T, want, ("cap", cap), cap=cap)
    finally:
        e.set_option("astar_step_cap", 0); po.set_step_cap(0)
    assert capped >= 100


def test_decode_batch_equals_oracle():
    """pf_decode_batch, W = 5, 64 agents on blocks64: chained searches of the closed-set variant, scored."""
    from pathfit.engine import score_params
    e, o, g = world("blocks64")
    e.set_option("astar_settle", 0)
    sp = score_params(0, True, 0.3, 0.8, 1.8, 100.0)
    rnd = np.random.default_rng(5)
    free = np.flatnonzero(g.reshape(-1) != 1)
    s, t = pairs_with_a_path(o, g, 0, 1, 400)[:2]
    s, t = s[0], t[0]
    WP, want = [], []
    while len(WP) < 64:
        wp = rnd.choice(free, 5).astype(np.int32)
        w = o.decode(s, t, wp)
        if len(w[0]) > 1:
            WP.append(wp); want.append(w)
    paths, st, stats = e.decode_host(s, t, wp_cells=np.stack(WP), sp=sp, path_cap=g.size + 6)
    c = e.counters()
    for a, (wp_, ost) in enumerate(want):
        assert st[a] == 0 and len(paths[a]) == len(wp_) and np.array_equal(paths[a], wp_), a
        assert np.array_equal(stats[a].view(np.uint64), o.score(wp_, 0, 0.3, 0.8, 1.8, True, 100.0).view(np.uint64)), a
    assert (c["pops"], c["pushes"], c["nbr_examined"]) == tuple(int(sum(w[1][k] for w in want)) for k in (0, 1, 4)), c


def test_mpa_run_equals_oracle():
    """70 predators x 6 iterations on fig7 (bench.py's MPA parameters): convergence curve and best path of MpaOracle."""
    import golden_io as gio
    import pathfit
    import pf_loops
    import pf_oracle as po
    g, s, t = gio.grid("fig7")
    N, K = 70, 6
    ref = pf_loops.MpaOracle(po.Oracle(g), s, t, N, K, seed=0, FADs_rate=0.2, P_const=0.5, levy_beta=2.0, w_turn=0.1, w_safe=0.8,
                             min_safe=1.8, diag_pen=100.0)
    best = ref.solve()
    eng = pathfit.Engine(g)
    try:
        m = pathfit.MPA(g, N, K, engine=eng, seed=0, FADs_rate=0.2, P_const=0.5, levy_beta=2.0, turn_penalty_factor=0.1,
                        safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty=100.0)
        m._sort()
        slot, s0 = m._best_row()
        m._take_first(s0, m._fetch(slot))
        for it in range(1, K + 1):
            m.step(it)
        result = m.result()
        assert list(m.convergence_curve_data) == list(ref.curve)
        assert [r * g.shape[1] + c for r, c in result[0]] == list(best[0])
        assert result[1:] == (best[1][0], int(best[1][1]), best[1][2], best[1][3], best[1][4])
    finally:
        eng.close()
