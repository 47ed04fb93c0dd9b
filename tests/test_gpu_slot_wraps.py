"""The search slots' records are epoch stamped and never cleared; a slot is wiped only when one of its counters is about to
wrap: the 14-bit avoid epoch at 0x3FF0 and the 24-bit solve tag at 0xFFFFFF - 2 * 0x8000 (slot_begin_eval), the label epoch
of the parallel settling engine at 127 (pf_settle.h).  A long-lived engine reaches all three; these tests get there with the
test hooks "astar_slot_avoid_epoch" / "astar_slot_tag" (forward only) and, for the label epoch, by running enough searches,
and compare every result with the CPU oracle and with the same call made on fresh counters.  pf_selftest_slot_state reads the
counters back, so a hook that did nothing could not pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AVOID_LIMIT = 0x3FF0
TAG_LIMIT = 0xFFFFFF - 2 * 0x8000
N = 48


def wrap_map():
    """48 x 48, 6 % obstacles, start (0, 0), target (47, 47)."""
    rnd = np.random.default_rng(48)
    g = (rnd.random((N, N)) < 0.06).astype(np.uint8)
    g[0, 0], g[N - 1, N - 1] = 2, 3
    return g


def search_batch(n, seed, short=False):
    """n (start, target, avoid list or None) triples on the wrap map."""
    g = wrap_map()
    rnd = np.random.default_rng(seed)
    free = np.flatnonzero(g.reshape(-1) != 1)
    starts = rnd.choice(free, n)
    if short:                                                    # a target a few cells away
        r = np.clip(starts // N + rnd.integers(-4, 5, n), 0, N - 1); c = np.clip(starts % N + rnd.integers(-4, 5, n), 0, N - 1)
        targets = (r * N + c).astype(np.int64)
    else:
        targets = rnd.choice(free, n)
    avoid = [rnd.choice(free, int(rnd.integers(1, 40))).astype(np.int32) if i % 3 else None for i in range(n)]
    return starts.astype(np.int32), targets.astype(np.int32), avoid


def chain_waypoints(W):
    """W free waypoints that run down the diagonal of the wrap map, so that the chained decode stays feasible to its end."""
    g = wrap_map()
    wp, c = [], 0
    for r in range(1, W + 1):
        c = max(c, r)
        while g[r, c] == 1:
            c += 1
        wp.append(r * N + c)
    return np.array(wp, np.int32)


def decode_inputs(n, W, seed):
    g = wrap_map()
    rnd = np.random.default_rng(seed)
    free = np.flatnonzero(g.reshape(-1) != 1)
    near = free[(free // N < 24) & (free % N < 24)]
    wp = np.stack([np.sort(rnd.choice(near if a % 2 else free, W)) for a in range(n)]).astype(np.int32)
    wp[0] = chain_waypoints(W)
    return wp


MPA_KW = dict(FADs_rate=0.5, P_const=0.5, levy_beta=1.5, turn_penalty_factor=0.1, safety_penalty_factor=0.8, min_safe_distance=1.8,
              diagonal_obstacle_penalty=100.0)


@pytest.fixture(scope="module")
def ref():
    """The oracle's answers, computed once: 120 searches x 3 variants, 24 decodes + scores, three MPA iterations of 32 predators,
    8192 short searches x 3 variants, the W = 40 chain."""
    import pf_oracle as po, pf_loops
    g = wrap_map()
    o = po.Oracle(g)
    d = {"g": g, "o": o}
    d["batch"] = search_batch(120, 1)
    d["batch_paths"] = [[o.astar(int(s), int(t), a, v)[0] for s, t, a in zip(*d["batch"])] for v in range(3)]
    d["wp"] = decode_inputs(24, 5, 2)
    d["dec_paths"] = [o.decode(0, N * N - 1, w)[0] for w in d["wp"]]
    d["dec_stats"] = np.array([o.score(p, 0, 0.3, 0.8, 1.8, True, 100.0) for p in d["dec_paths"]])
    mk = dict(FADs_rate=0.5, P_const=0.5, levy_beta=1.5, w_turn=0.1, w_safe=0.8, min_safe=1.8, diag_pen=100.0, seed=9)
    m = pf_loops.MpaOracle(o, 0, N * N - 1, 32, 6, **mk)
    m.solve()
    d["mpa"] = ([p for p, _ in m.pop], [s[4] for _, s in m.pop], list(m.curve))
    m = pf_loops.MpaOracle(o, 0, N * N - 1, 32, 6, **mk)       # the candidates of iteration 1 (MPA.py:339-377), predator by predator
    m._sort()
    d["mpa_cand"] = [m.phase_candidate(1, i, m.pop[0], (1.0 - 1 / 6) ** (2.0 / 6)) for i in range(32)]
    assert sum(len(c[0]) != len(m.pop[0][0]) or not np.array_equal(c[0], m.pop[0][0]) for c in d["mpa_cand"]) >= 4   # rebuilt paths among them
    d["big"] = search_batch(8192, 3, short=True)
    d["big_paths"] = [[o.astar(int(s), int(t), a, v)[0] for s, t, a in zip(*d["big"])] for v in range(3)]
    d["chain"] = chain_waypoints(40)[None, :]
    d["chain_path"] = o.decode(0, N * N - 1, d["chain"][0])[0]
    assert len(d["chain_path"]) > 40 and sum(len(p) > 0 for p in d["dec_paths"]) >= 4
    return d


def run_searches(e, ref, v, key="batch"):
    s, t, av = ref[key]
    paths, st = e.astar_host(v, s, t, av)
    for i, want in enumerate(ref[key + "_paths"][v]):
        assert st[i] != 3 and (st[i] == 0) == (len(want) > 0) and np.array_equal(paths[i], want), (key, v, i, st[i])
    return [p.tolist() for p in paths], st.tolist()


def run_decodes(e, ref):
    from pathfit.engine import score_params
    paths, st, stats = e.decode_host(0, N * N - 1, wp_cells=ref["wp"], sp=score_params(0, True, 0.3, 0.8, 1.8, 100.0))
    for i, want in enumerate(ref["dec_paths"]):
        assert st[i] == (0 if len(want) else 1) and np.array_equal(paths[i], want), (i, st[i])
    assert np.array_equal(stats, ref["dec_stats"])
    return [p.tolist() for p in paths], st.tolist(), stats.tolist()


def run_mpa(e, ref, fused):
    import pathfit
    m = pathfit.MPA(ref["g"], 32, 6, seed=9, fused=fused, engine=e, **MPA_KW)
    m.solve_path_planning()
    pop = m.population
    want_paths, want_fit, want_curve = ref["mpa"]
    assert [p["fitness"] for p in pop] == want_fit and m.convergence_curve_data == want_curve, fused
    for a, b in zip(pop, want_paths):
        assert np.array_equal(a["path"].cells, b), fused
    rows = []
    if not fused:                                                # the phase kernel's candidate rows of iteration 1 == the oracle's
        m = pathfit.MPA(ref["g"], 32, 6, seed=9, fused=False, engine=e, **MPA_KW)
        m.step(1)
        cells, lens, stats, st = m.d_cand_cells.download(), m.d_cand_len.download(), m.d_cand_stats.download(), m.d_status.download()
        for a, (wp, ws) in enumerate(ref["mpa_cand"]):
            assert np.array_equal(cells[a, :lens[a]], wp) and np.array_equal(stats[a], ws), a
        rows += [lens.tolist(), stats.tolist(), st.tolist()]
    return [list(p["path"].cells) for p in pop], want_fit, rows


def calls(ref):
    return [lambda e: run_searches(e, ref, 0), lambda e: run_searches(e, ref, 1), lambda e: run_searches(e, ref, 2),
            lambda e: run_decodes(e, ref), lambda e: run_mpa(e, ref, True), lambda e: run_mpa(e, ref, False)]


def reset_options(e):
    for name in ("astar_slot_avoid_epoch", "astar_slot_tag", "astar_settle"):
        e.set_option(name, -1)


@pytest.mark.parametrize("settle", [0, -1])
def test_avoid_epoch_wipe_in_every_search_kernel(ref, settle):
    """Every slot's avoid epoch starts two evaluations below the wipe; the A* batch (three variants), the decode and the MPA
    sweeps (fused: k_mpa_search; unfused: the phase and the FADs kernels) then each meet the wipe in the middle of a batch -- four
    runs on fresh engines, each starting the sequence at another call, so that each kernel is the first to cross.  With
    "astar_settle" 0 every search runs the sequential pop loop, which reads the avoid stamps; by default (-1) the Dijkstra
    searches and the decodes of a small batch go through the settling engine first."""
    from pathfit.engine import Engine
    seq = calls(ref)
    e = Engine(ref["g"])
    try:
        e.set_option("astar_settle", settle)
        before = [f(e) for f in seq]                             # fresh counters: == the oracle (asserted inside)
        assert e.slot_state(0)[1] < 64
    finally:
        e.close()
    for first in (0, 3, 4, 5):
        e = Engine(ref["g"])
        try:
            e.set_option("astar_settle", settle)
            e.set_option("astar_slot_avoid_epoch", AVOID_LIMIT - 2)
            paths, st = e.astar_host(0, [0], [N * N - 1])        # one search lands on slot 0: the hook is applied in front of it
            assert st[0] == 0 and np.array_equal(paths[0], ref["o"].astar(0, N * N - 1, None, 0)[0])
            assert e.slot_state(0)[1] == AVOID_LIMIT - 1         # near the limit: the next evaluation of slot 0 wipes it
            for k in range(len(seq)):
                i = (first + k) % len(seq)
                assert seq[i](e) == before[i], (first, i)
            e.astar_host(0, [0], [N * N - 1])
            assert 1 <= e.slot_state(0)[1] < 64 and e.slot_state(0)[0] < 1 << 16
        finally:
            reset_options(e)
            e.close()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_avoid_epoch_wipe_in_mid_batch(ref, variant):
    """8192 short searches on 2048 slots: every slot evaluates several, and is wiped at its second."""
    from pathfit.engine import Engine
    e = Engine(ref["g"])
    try:
        e.set_option("astar_slot_avoid_epoch", AVOID_LIMIT - 2)
        run_searches(e, ref, variant, "big")
        assert e.counters()["overflow_agents"] == 0
        e.astar_host(0, [0], [N * N - 1])
        assert 1 <= e.slot_state(0)[1] < 64
    finally:
        reset_options(e)
        e.close()


def test_forward_only_hook_refuses_a_step_back(ref):
    import pathfit
    from pathfit.engine import Engine
    e = Engine(ref["g"])
    try:
        e.set_option("astar_slot_avoid_epoch", 100)
        e.astar_host(0, [0], [N * N - 1])
        assert e.slot_state(0)[1] == 101
        e.set_option("astar_slot_avoid_epoch", 50)
        with pytest.raises(pathfit.PathfitError, match="forward"):
            e.astar_host(0, [0], [N * N - 1])
        assert e.slot_state(0)[1] == 101
        paths, st = e.astar_host(0, [0], [N * N - 1])            # one-shot: the refused value is gone
        assert st[0] == 0 and e.slot_state(0)[1] == 102
        with pytest.raises(pathfit.PathfitError):
            e.set_option("astar_slot_tag", 1 << 24)
    finally:
        reset_options(e)
        e.close()


def test_tag_wipe_after_a_long_chain(ref):
    """The tag starts a few searches below its limit: a decode of 40 waypoints (41 searches, each with a fresh tag) starts below
    it, runs past it without a wipe inside the chain, and the next evaluation of the slot wipes it."""
    from pathfit.engine import Engine, score_params
    seq = calls(ref)
    e = Engine(ref["g"])
    try:
        e.set_option("astar_settle", 0)                          # only a search of the sequential loop takes a tag
        before = [f(e) for f in seq]
        e.set_option("astar_slot_tag", TAG_LIMIT - 20)
        paths, st, _ = e.decode_host(0, N * N - 1, wp_cells=ref["chain"], sp=score_params(0, True, 0.3, 0.8, 1.8, 100.0))
        assert st[0] == 0 and np.array_equal(paths[0], ref["chain_path"])
        tag = e.slot_state(0)[0]
        assert TAG_LIMIT <= tag < TAG_LIMIT + 2 * 0x8000, tag    # past the limit, not wiped inside the chain, no wrap
        for i in (3, 0, 1, 2, 4, 5):                             # the decode batch first: its 24 chains start on near-limit tags
            assert seq[i](e) == before[i], i
        e.astar_host(0, [0], [N * N - 1])
        assert e.slot_state(0)[0] < 1 << 16
    finally:
        reset_options(e)
        e.close()


@pytest.mark.parametrize("first", [0, 4, 5])
def test_tag_wipe_in_every_search_kernel(ref, first):
    """Every slot's tag starts one search below the limit, and one search takes slot 0 past it.  Each slot's first evaluation
    after that begins below the limit and ends past it; its next one is wiped, in whichever kernel runs it: the A* batch
    (first = 0: the slots that variant 0 took past the limit are wiped by variants 1 and 2), k_mpa_search (4) and the phase and
    FADs kernels (5), where a slot evaluates several items of one sweep, and the decode after them."""
    from pathfit.engine import Engine
    seq = calls(ref)
    e = Engine(ref["g"])
    try:
        e.set_option("astar_settle", 0)
        before = [f(e) for f in seq]
    finally:
        reset_options(e)
        e.close()
    e = Engine(ref["g"])
    try:
        e.set_option("astar_settle", 0)
        e.set_option("astar_slot_tag", TAG_LIMIT - 1)
        paths, st = e.astar_host(0, [0], [N * N - 1])
        assert st[0] == 0 and np.array_equal(paths[0], ref["o"].astar(0, N * N - 1, None, 0)[0])
        assert TAG_LIMIT <= e.slot_state(0)[0] < TAG_LIMIT + 2 * 0x8000      # slot 0 is past the limit, every other slot one below
        for k in range(len(seq)):
            i = (first + k) % len(seq)
            assert seq[i](e) == before[i], (first, i)
        e.astar_host(0, [0], [N * N - 1])
        assert e.slot_state(0)[0] < 1 << 16
    finally:
        reset_options(e)
        e.close()


@pytest.mark.parametrize("variant,settle", [(2, -1), (0, 1)])
def test_settle_label_epoch_wipe(ref, variant, settle):
    """140 one-search batches in a row (n = 1 lands on slot 0), with and without an avoid list: the settling engine's label epoch
    climbs to 126, its label array is wiped and the epoch starts again at 1 -- once on the way."""
    from pathfit.engine import Engine
    s, t, av = ref["batch"]
    want = ref["batch_paths"][variant]
    o = ref["o"]
    real = [i for i in range(120) if av[i] is not None and len(want[i]) > 1 and len(o.astar(int(s[i]), int(t[i]), None, variant)[0]) > 1]
    assert len(real) >= 40                                       # searches that do reach the engine, with and without their avoid list
    e = Engine(ref["g"])
    try:
        e.set_option("astar_settle", settle)
        epochs = []
        for k in range(140):
            i = real[k % len(real)]
            paths, st = e.astar_host(variant, [s[i]], [t[i]], [av[i]] if k % 2 and av[i] is not None else None)
            exp = want[i] if k % 2 and av[i] is not None else ref["o"].astar(int(s[i]), int(t[i]), None, variant)[0]
            assert st[0] == (0 if len(exp) else 1) and np.array_equal(paths[0], exp), (k, i)
            epochs.append(e.slot_state(0)[2])
        falls = [k for k in range(1, 140) if epochs[k] < epochs[k - 1]]
        assert len(falls) == 1 and epochs[falls[0]] == 1 and epochs[falls[0] - 1] == 126, epochs
        assert max(epochs) == 126
    finally:
        reset_options(e)
        e.close()
