"""HIP kernels under the move policies other than the default: 4-connected searches (allow_diag = 0, with either corner
rule) and corner cutting allowed (restrict = 0).  Connectors, decodes, scoring, MPA rebuilds and whole MPA runs, the
facades, dynamic maps and policy switches on one engine are compared with the CPU oracle (itself pinned to the
unmodified reference by tests/test_oracle_policies.py) and with the reference's goldens in policy_cases.npz."""
import math
import time

import numpy as np
import pytest

import golden_io as gio

pytestmark = pytest.mark.gpu

POLICIES = ((1, 1), (1, 0), (0, 1), (0, 0))          # (allow_diag, restrict_corner); the policy index is 2 * ad + rs
_eng = {}
_orc = {}
_ans = {}              # oracle answers, shared by both engine modes
SEQ = True             # see closed_set_engine


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    """Every engine holds gigabytes of search scratch: free this module's before the next module runs."""
    yield
    for e in _eng.values():
        e[0].close()
    _eng.clear()


@pytest.fixture(autouse=True, params=["sequential", "settle"])
def closed_set_engine(request):
    """Every test runs with the closed-set searches on the sequential pop loop (paths, statuses and the reference's pop /
    push counts are compared) and with the label-settling engine in front of it (variants 0 and 2: paths and statuses;
    variant 1 keeps its counts)."""
    global SEQ
    SEQ = request.param == "sequential"
    e = eng("fig7")[0]
    e.set_option("astar_settle", 0 if SEQ else 1)
    yield
    e.set_option("astar_settle", -1)
    SEQ = True


def counts_apply(variant):
    return SEQ or variant == 1


def grid_of(name):
    if name.startswith("up"):          # "up2:g256" -> np.kron upsample, S = 0, T = last cell
        k, base = name[2:].split(":")
        g = gio.upsample(gio.grid(base)[0], int(k))
        return g, 0, g.size - 1
    if name == "open1024":
        g = np.zeros((1024, 1024), np.uint8)
        return g, 0, g.size - 1
    if name == "open":
        R, C = (int(v) for v in gio.load("policy_cases")["open_map_shape"])
        g = np.zeros((R, C), np.uint8)
        g[0, 0], g[-1, -1] = 2, 3
        return g, 0, R * C - 1
    return gio.grid(name)


def eng(name):
    from pathfit.engine import Engine
    if name not in _eng:
        g, s, t = grid_of(name)
        _eng[name] = (Engine(g), s, t, g)
    return _eng[name]


def orc(name, ad, rs):
    import pf_oracle as po
    key = (name, ad, rs)
    if key not in _orc:
        _orc[key] = po.Oracle(grid_of(name)[0], ad, rs)
    return _orc[key]


def oracle_astar(name, ad, rs, s, t, avoid, variant, tag=None):
    """Oracle answer (path, stats), computed once per search."""
    key = (name, ad, rs, int(s), int(t), variant, tag)
    if key not in _ans:
        _ans[key] = orc(name, ad, rs).astar(int(s), int(t), avoid, variant)
    return _ans[key]


def check_batch(name, ad, rs, variant, starts, targets, avoid, path_cap=8192, tag=None, e=None):
    """One astar_host batch against the oracle: path, status, pops / pushes -> device counters."""
    e = e or eng(name)[0]
    paths, st, cnt = e.astar_host(variant, starts, targets, avoid, path_cap=path_cap, allow_diag=ad, restrict_corner=rs,
                                  want_counters=True)
    for i in range(len(starts)):
        av = avoid[i] if avoid is not None else None
        want, ost = oracle_astar(name, ad, rs, starts[i], targets[i], av, variant, (tag, i) if av is not None else tag)
        assert np.array_equal(paths[i], want), (name, ad, rs, variant, i)
        assert st[i] == ost[5], (name, ad, rs, variant, i, st[i], ost[5])
        if len(want) > 1 and counts_apply(variant):
            assert cnt[i, 0] == ost[0] and cnt[i, 1] == ost[1], (name, ad, rs, variant, i, cnt[i], ost[:2])
    return paths, st, cnt


def test_connector_goldens():
    """AStarSolver.solve / MPA._a_star / DijkstraSolver.solve of the reference under (1, 0), (0, 1), (0, 0)."""
    z = gio.load("policy_cases")
    names = [str(s) for s in z["grid_names"]]
    for pi, (ad, rs) in enumerate(z["policies"]):
        ad, rs = int(ad), int(rs)
        for gid, gname in enumerate(names):
            e = eng(gname)[0]
            for variant in (0, 1, 2):
                idx = np.flatnonzero((z["as_policy"] == pi) & (z["as_grid"] == gid) & (z["as_variant"] == variant))
                avoid = [gio.csr_get(z["as_avoid_off"], z["as_avoid"], i) if z["as_has_avoid"][i] else None for i in idx]
                paths, st, cnt = e.astar_host(variant, z["as_start"][idx], z["as_target"][idx], avoid, allow_diag=ad,
                                              restrict_corner=rs, want_counters=True)
                for j, i in enumerate(idx):
                    want = gio.csr_get(z["as_path_off"], z["as_path"], i)
                    assert st[j] == (1 if len(want) == 0 else 0), (gname, ad, rs, variant, i, st[j])
                    assert np.array_equal(paths[j], want), (gname, ad, rs, variant, i)
                    if len(want) > 1 and counts_apply(variant):
                        assert tuple(cnt[j, :2]) == tuple(z["as_counts"][i]), (gname, ad, rs, variant, i, cnt[j], z["as_counts"][i])


def test_astar_random_512_vs_oracle():
    """48 random pairs + corner to corner on the 512^2 bench grid, avoid sets on half, all policies and variants."""
    name = "up2:g256"
    _, s, t, g = eng(name)
    rnd = np.random.default_rng(15)
    free = np.flatnonzero(g.reshape(-1) != 1)
    n = 49
    starts = rnd.choice(free, n); targets = rnd.choice(free, n)
    starts[0], targets[0] = s, t
    avoid = [rnd.choice(free, 200) if i % 2 else None for i in range(n)]
    for ad, rs in POLICIES:
        for variant in (0, 1, 2):
            _, st, cnt = check_batch(name, ad, rs, variant, starts, targets, avoid, tag="r512")
            assert (st != 3).all()
            if not ad and variant != 2 and counts_apply(variant):
                assert cnt[0, 0] == 165746, (ad, rs, variant, cnt[0])          # (8-connected: 91 044, test_gpu_parity.py)


@pytest.mark.parametrize("plateau_kernels", [1, 0])
def test_astar_open_map_4_connected_vs_oracle(plateau_kernels):
    """The empty 1024 x 1024 map under 4-connectivity: unit steps make g an integer, so exact (f, g) ties are the normal
    case, and the corner-to-corner search floods the whole map (1 048 576 pops).  Nothing may overflow, and every search
    must equal the oracle: path, status, pops."""
    from pathfit.engine import Engine, ST_OVERFLOW
    name = "open1024"
    g = grid_of(name)[0]
    e = Engine(g)                          # (not kept: the search scratch of a 1024^2 engine is large)
    e.set_option("plateau_kernels", plateau_kernels)
    rnd = np.random.default_rng(21)
    n = 24
    starts = rnd.integers(0, g.size, n).astype(np.int32); targets = rnd.integers(0, g.size, n).astype(np.int32)
    starts[:4] = [0, 0, g.size - 1, 1023]; targets[:4] = [g.size - 1, 1023 * 1024 + 511, 0, 1023 * 1024]
    try:
        for variant in (0, 1):
            t0 = time.perf_counter()
            _, st, cnt = check_batch(name, 0, 1, variant, starts, targets, None, path_cap=4096, e=e)
            print(f"open 1024^2 4-connected: variant {variant}, plateau {plateau_kernels}, settle {int(not SEQ)}: "
                  f"{n} searches in {e.last_kernel_ms():.1f} ms kernel, {time.perf_counter() - t0:.2f} s with the oracle checks")
            assert (st != ST_OVERFLOW).all() and (st == 0).all()
            if counts_apply(variant):
                assert cnt[0, 0] == 1048576 and cnt[1, 0] == 524288 and cnt[2, 0] == 1048576, cnt[:3]
    finally:
        e.set_option("plateau_kernels", -1)
        e.close()


def test_sealed_rooms_4_connected_then_door_opened():
    """The sealed-room map of test_gpu_parity.py under 4-connectivity (the second room's diagonal leak is closed), then
    pf_update_grid opens a one-cell door into the first room: component labels and the records' move masks of every
    policy must be rebuilt (stale labels answer "no path", stale masks give other paths)."""
    from pathfit.engine import Engine
    import pf_oracle as po
    rnd = np.random.default_rng(9)
    g = (rnd.random((96, 96)) < 0.08).astype(np.uint8)
    g[20:62, 30] = 1; g[20:62, 71] = 1; g[20, 30:72] = 1; g[61, 30:72] = 1          # sealed 40x40 room
    g[70:90, 5:8] = 1; g[70, 5:30] = 1; g[89, 5:30] = 1; g[70:90, 29] = 1             # second room, diagonal leak at a corner
    g[89, 29] = 0; g[88, 29] = 1; g[89, 28] = 1
    e = Engine(g)
    free = np.flatnonzero(g.reshape(-1) != 1)
    inside = np.array([c for c in free if 20 < c // 96 < 61 and 30 < c % 96 < 71])
    room2 = np.array([c for c in free if 70 < c // 96 < 89 and 7 < c % 96 < 29])
    n = 40
    starts = np.concatenate([rnd.choice(inside, 10), rnd.choice(free, 10), rnd.choice(room2, 10), rnd.choice(free, 10)])
    targets = np.concatenate([rnd.choice(free, 10), rnd.choice(inside, 10), rnd.choice(free, 10), rnd.choice(room2, 10)])
    avoid = [rnd.choice(free, 60) if i % 3 == 0 else None for i in range(n)]

    def run(grid, policies):
        fails = {}
        for ad, rs in policies:
            o = po.Oracle(grid, ad, rs)
            for variant in (0, 1, 2):
                paths, st, cnt = e.astar_host(variant, starts, targets, avoid, path_cap=4096, allow_diag=ad, restrict_corner=rs,
                                              want_counters=True)
                for i in range(n):
                    want, ost = o.astar(int(starts[i]), int(targets[i]), avoid[i], variant)
                    assert np.array_equal(paths[i], want) and st[i] == ost[5], (ad, rs, variant, i)
                    if len(want) > 1 and counts_apply(variant):
                        assert cnt[i, 0] == ost[0] and cnt[i, 1] == ost[1], (ad, rs, variant, i)
                fails[(ad, rs, variant)] = [len(p) == 0 for p in paths]
        return fails

    before = run(g, POLICIES)
    # the second room leaks only diagonally between two obstacles: without corner cutting its pairs fail
    assert sum(before[(0, 1, 0)][20:40]) > sum(before[(1, 0, 0)][20:40])
    assert all(sum(before[(ad, rs, 0)][:20]) >= 15 for ad, rs in POLICIES)
    g2 = g.copy()
    g2[40, 29:32] = 0                                       # a door in the first room's west wall
    e.update_grid(g2)
    try:
        after = run(g2, ((0, 0), (1, 1), (0, 1), (1, 0)))
    finally:
        e.close()
    for ad, rs in POLICIES:
        assert sum(after[(ad, rs, 0)][:20]) < sum(before[(ad, rs, 0)][:20]) - 5, (ad, rs)


def _switch_batch(e, name, pol, rnd_seed):
    """One astar_host batch of each variant and one decode batch, as plain arrays for comparison."""
    from pathfit.engine import score_params
    ad, rs = pol >> 1, pol & 1
    _, s, t, g = eng(name)
    rnd = np.random.default_rng(rnd_seed)
    free = np.flatnonzero(g.reshape(-1) != 1)
    starts, targets = rnd.choice(free, 32), rnd.choice(free, 32)
    avoid = [rnd.choice(free, 40) if i % 2 else None for i in range(32)]
    out = []
    for variant in (0, 1, 2):
        paths, st, cnt = e.astar_host(variant, starts, targets, avoid, allow_diag=ad, restrict_corner=rs, want_counters=True)
        out.append((paths, st, cnt if counts_apply(variant) else None))
    wp = rnd.choice(free, (24, 3)).astype(np.int32)
    paths, st, stats = e.decode_host(s, t, wp_cells=wp, sp=score_params(0, rs, 0.3, 0.8, 1.8, 100.0), allow_diag=ad,
                                     restrict_corner=rs)
    out.append((paths, st, stats))
    return out


def _same(a, b):
    for (pa, sa, ca), (pb, sb, cb) in zip(a, b):
        assert np.array_equal(sa, sb) and len(pa) == len(pb)
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        assert (ca is None) == (cb is None) and (ca is None or np.array_equal(ca, cb))


def test_policy_switching_on_one_engine():
    """Batches on one Engine in the policy order 3, 0, 3, 1, 2, 0 (policy = 2 * allow_diag + restrict): each equals the same
    batch on a fresh engine that only ever ran that policy (the records' move masks are rebuilt on every switch)."""
    from pathfit.engine import Engine
    name = "g128crop"
    g = eng(name)[3]
    shared = Engine(g)
    fresh = {}
    try:
        for k, pol in enumerate((3, 0, 3, 1, 2, 0)):
            got = _switch_batch(shared, name, pol, 100 + pol)
            if pol not in fresh:
                fresh[pol] = Engine(g)
            _same(got, _switch_batch(fresh[pol], name, pol, 100 + pol))
            ad, rs = pol >> 1, pol & 1
            paths = got[0][0]
            assert any(len(p) > 1 for p in paths)
            for p in paths:
                if len(p) > 1 and not ad:
                    assert (np.abs(np.diff(p // 128)) + np.abs(np.diff(p % 128)) == 1).all(), (k, pol)
    finally:
        shared.close()
        for f in fresh.values():
            f.close()


def test_step_cap_4_connected_vs_oracle():
    """The step cap (astar.py:58 / MPA.py:118) lowered on both sides, under 4-connectivity: same status, same pop count, no
    path -- including caps that fall in the middle of a seven-head trip."""
    import pf_oracle as po
    name = "up2:g256"
    e, s, t, g = eng(name)
    o = orc(name, 0, 1)
    rnd = np.random.default_rng(19)
    free = np.flatnonzero(g.reshape(-1) != 1)
    n = 24
    starts = rnd.choice(free, n); targets = rnd.choice(free, n)
    starts[0], targets[0] = s, t
    try:
        for cap in (1, 7, 8, 1000):
            e.set_option("astar_step_cap", cap); po.set_step_cap(cap)
            capped = 0
            for variant in (0, 1, 2):
                paths, st, cnt = e.astar_host(variant, starts, targets, None, path_cap=8192, allow_diag=0, restrict_corner=1,
                                              want_counters=True)
                for i in range(n):
                    want, ost = o.astar(int(starts[i]), int(targets[i]), None, variant)
                    assert np.array_equal(paths[i], want), (cap, variant, i)
                    if st[i] == 1 and ost[5] == 2:
                        po.set_step_cap(0)             # proved "no path" without searching: the uncapped oracle agrees
                        assert len(o.astar(int(starts[i]), int(targets[i]), None, variant)[0]) == 0
                        po.set_step_cap(cap)
                        continue
                    assert st[i] == ost[5], (cap, variant, i, st[i], ost[5])
                    if ost[5] == 2:
                        assert cnt[i, 0] == cap and len(want) == 0
                        capped += 1
            assert capped > 0
    finally:
        e.set_option("astar_step_cap", 0); po.set_step_cap(0)


def test_decode_and_score_goldens():
    """GA chromosome and PSO position decodes + helper stats of the reference under the three non-default policies."""
    from pathfit.engine import score_params
    z = gio.load("policy_cases")
    names = [str(s) for s in z["grid_names"]]
    done = 0
    for pi, (ad, rs) in enumerate(z["policies"]):
        ad, rs = int(ad), int(rs)
        for gid, gname in enumerate(names):
            e, s, t, _ = eng(gname)
            for wi, w in enumerate((z["main_w"], z["def_w"])):
                sp = score_params(0, rs, w[0], w[1], w[2], w[3])
                for kind in (0, 1):
                    idx = np.flatnonzero((z["dec_policy"] == pi) & (z["dec_grid"] == gid) & (z["dec_w"] == wi) &
                                         (z["dec_kind"] == kind))
                    byW = {}
                    for i in idx:
                        L = len(gio.csr_get(z["dec_wp_off"], z["dec_wp"], i))
                        byW.setdefault(L if kind == 0 else L // 2, []).append(i)
                    for W, ids in byW.items():
                        wp = np.array([gio.csr_get(z["dec_wp_off"], z["dec_wp"], i) for i in ids])
                        if kind == 0:
                            paths, st, stats = e.decode_host(s, t, wp_cells=wp.astype(np.int32), sp=sp, allow_diag=ad,
                                                             restrict_corner=rs)
                        else:
                            paths, st, stats = e.decode_host(s, t, wp_pos=wp.reshape(len(ids), W, 2), sp=sp, allow_diag=ad,
                                                             restrict_corner=rs)
                        for j, i in enumerate(ids):
                            want = gio.csr_get(z["dec_path_off"], z["dec_path"], i)
                            assert st[j] != 3 and np.array_equal(paths[j], want), (gname, ad, rs, kind, i)
                            assert np.array_equal(stats[j], z["dec_stats"][i]), (gname, ad, rs, i, stats[j], z["dec_stats"][i])
                            done += 1
    assert done == len(z["dec_kind"])


def test_decode_random_512_vs_oracle():
    from pathfit.engine import score_params
    name = "up2:g256"
    e, s, t, g = eng(name)
    rnd = np.random.default_rng(23)
    free = np.flatnonzero(g.reshape(-1) != 1)
    n, W = 24, 5
    wp = rnd.choice(free, (n, W)).astype(np.int32)
    for ad, rs in POLICIES:
        o = orc(name, ad, rs)
        sp = score_params(0, rs, 0.3, 0.8, 1.8, 100.0)
        paths, st, stats = e.decode_host(s, t, wp_cells=wp, sp=sp, path_cap=16384, allow_diag=ad, restrict_corner=rs)
        feas = 0
        for i in range(n):
            want, _ = o.decode(s, t, wp[i])
            assert st[i] != 3 and np.array_equal(paths[i], want), (ad, rs, i)
            assert np.array_equal(stats[i], o.score(want, 0, 0.3, 0.8, 1.8, rs, 100.0)), (ad, rs, i)
            feas += len(want) > 0
        assert feas >= 3, (ad, rs)


def test_score_batch_hand_built_goldens():
    """pf_score_batch alone on the reference's scores of hand-built paths (1 .. 130 cells, turns and corner cuts on the
    64-cell chunk boundaries, steps of any length, an obstacle-free map), both variants, restrict_policy 1 and 0."""
    from pathfit.engine import score_params
    z = gio.load("policy_cases")
    names = [str(s) for s in z["sc_grid_names"]]
    done = 0
    for gid, gname in enumerate(names):
        e = eng(gname)[0]
        for variant in (0, 1):
            for rs in (1, 0):
                for wi, (wt, ws, ms, dp) in enumerate(z["sc_weights"]):
                    idx = np.flatnonzero((z["sc_grid"] == gid) & (z["sc_variant"] == variant) & (z["sc_restrict"] == rs) &
                                         (z["sc_w"] == wi))
                    if not len(idx):
                        continue
                    got = e.score_host([gio.csr_get(z["sc_path_off"], z["sc_path"], i) for i in idx],
                                       score_params(variant, rs, wt, ws, ms, dp))
                    for j, i in enumerate(idx):
                        assert np.array_equal(got[j], z["sc_stats"][i]), (gname, variant, rs, i, got[j], z["sc_stats"][i])
                        done += 1
    assert done == len(z["sc_variant"])


def test_score_batch_on_corner_cutting_paths():
    """Paths of the restrict = 0 connector on the 512^2 grid cut corners: pf_score_batch with restrict_policy 1 must charge
    them (bit for bit with the oracle), with 0 it must not."""
    from pathfit.engine import score_params
    name = "up2:g256"
    e, s, t, g = eng(name)
    o = orc(name, 1, 0)
    rnd = np.random.default_rng(29)
    free = np.flatnonzero(g.reshape(-1) != 1)
    n = 48
    starts, targets = rnd.choice(free, n), rnd.choice(free, n)
    paths, st = e.astar_host(0, starts, targets, None, path_cap=8192, allow_diag=1, restrict_corner=0)
    paths = [p for p in paths if len(p) > 1]
    assert len(paths) >= 30
    for variant in (0, 1):
        for rs in (1, 0):
            got = e.score_host(paths, score_params(variant, rs, 0.3, 0.8, 1.8, 100.0))
            for i, p in enumerate(paths):
                assert np.array_equal(got[i], o.score(p, variant, 0.3, 0.8, 1.8, rs, 100.0)), (variant, rs, i)
            if rs:
                assert (got[:, 3] > 0).sum() >= len(paths) // 3, (variant, (got[:, 3] > 0).sum())
            else:
                assert (got[:, 3] == 0).all()


def test_mpa_rebuild_goldens():
    """MPA._reconstruct_path_segment of the reference through pf_mpa_rebuild_batch: path, status, stats."""
    from pathfit._lib import MpaParams
    from pathfit.engine import score_params
    z = gio.load("policy_cases")
    names = [str(s) for s in z["grid_names"]]
    seed, it = (int(v) for v in z["reb_seed_it"])
    done = 0
    for pi, (ad, rs) in enumerate(z["policies"]):
        ad, rs = int(ad), int(rs)
        for gid, gname in enumerate(names):
            e, s, t, _ = eng(gname)
            o = orc(gname, ad, rs)
            for bi, beta in enumerate((1.5, 2.0)):
                ids = np.flatnonzero((z["reb_policy"] == pi) & (z["reb_grid"] == gid) & (z["reb_beta"] == beta))
                if not len(ids):
                    continue
                e.mpa_setup(MpaParams(0.5, beta, float(z["reb_sigma"][bi]), 0.2, len(ids), s, t, ad, rs),
                            score_params(1, rs, 0.1, 0.05, 1.5, 1000.0))
                groups = {}
                for i in ids:
                    groups.setdefault(gio.csr_get(z["reb_el_off"], z["reb_el"], i).tobytes(), []).append(i)
                for gi in groups.values():
                    n = len(gi)
                    cap = 4 * (e.R + e.C) + 64 if e.R > 20 else 400
                    pop = np.zeros((n, cap), np.int32); plen = np.zeros(n, np.int32)
                    for j, i in enumerate(gi):
                        p = gio.csr_get(z["reb_in_off"], z["reb_in"], i)
                        pop[j, :len(p)] = p; plen[j] = len(p)
                    el = gio.csr_get(z["reb_el_off"], z["reb_el"], gi[0])
                    pstats = np.array([o.score(pop[j, :plen[j]], 1, 0.1, 0.05, 1.5, rs, 1000.0) for j in range(n)])
                    dpop, dlen, dstats, del_ = e.put(pop), e.put(plen), e.put(pstats), e.put(el)
                    oc, ol, os_, ost = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf((n, 5), np.float64), e.buf(n, np.int32)
                    d_idx, d_lv = e.put(z["reb_idx"][gi], np.int32), e.put(z["reb_is_levy"][gi], np.int32)
                    d_sc, d_ag = e.put(z["reb_scale"][gi], np.float64), e.put(z["reb_agent"][gi], np.int32)
                    e._ck(e.L.pf_mpa_rebuild_batch(e.h, it, seed, n, cap, dpop.ptr, dlen.ptr, dstats.ptr, del_.ptr, len(el),
                                                   d_idx.ptr, d_lv.ptr, d_sc.ptr, d_ag.ptr, oc.ptr, ol.ptr, os_.ptr, ost.ptr))
                    cells, lens, stats, st = oc.download(), ol.download(), os_.download(), ost.download()
                    for j, i in enumerate(gi):
                        want = gio.csr_get(z["reb_out_off"], z["reb_out"], i)
                        assert st[j] != 3 and np.array_equal(cells[j, :lens[j]], want), (gname, ad, rs, beta, i, st[j])
                        assert np.array_equal(stats[j], z["reb_stats"][i]), (gname, ad, rs, beta, i)
                        done += 1
    assert done == len(z["reb_idx"])


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("gname", ["fig7", "img1"])
@pytest.mark.parametrize("ad,rs", [(0, 1), (1, 0)])
def test_mpa_runs_vs_oracle_loop(ad, rs, gname, fused):
    """pathfit.MPA with allow_diagonal_moves=False, or restrict_diagonal_near_obstacle=False: best path, stats, curve and
    the whole population after 20 iterations of 30 predators equal the oracle-driven loop."""
    import pathfit, pf_oracle as po, pf_loops
    g, s, t = gio.grid(gname)
    m = pathfit.MPA(g, 30, 20, seed=7, fused=fused, allow_diagonal_moves=bool(ad), restrict_diagonal_near_obstacle=bool(rs))
    got = m.solve_path_planning()
    ref = pf_loops.MpaOracle(po.Oracle(g, ad, rs), s, t, 30, 20, restrict=rs, seed=7)
    best = ref.solve()
    assert [r * 20 + c for r, c in got[0]] == list(best[0])
    assert (got[1], got[2], got[3], got[4], got[5]) == (best[1][0], int(best[1][1]), best[1][2], best[1][3], best[1][4])
    assert m.convergence_curve_data == ref.curve
    pop = m.population
    assert len(pop) == len(ref.pop)
    for a, b in zip(pop, ref.pop):
        assert np.array_equal(a["path"].cells, b[0]) and a["fitness"] == b[1][4]
    if not ad:
        cells = np.asarray(best[0])
        assert (np.abs(np.diff(cells // 20)) + np.abs(np.diff(cells % 20)) == 1).all()
    m.engine.close()


def test_mpa_bound_pruning_4_connected_changes_nothing():
    """The MPA pruning bounds are built from the policy's move mask: under 4-connectivity they are 4-connected distances.
    Pruning must fire and must leave every predator, the curve and the counters of the kept work exactly as without it."""
    import pathfit
    g, s, t = gio.grid("g256")
    kw = dict(FADs_rate=0.2, P_const=0.5, levy_beta=1.5, turn_penalty_factor=0.1, safety_penalty_factor=0.8,
              min_safe_distance=1.8, diagonal_obstacle_penalty=100.0, allow_diagonal_moves=False)
    runs = []
    for prune in (1, 0):
        m = pathfit.MPA(g, 64, 9, seed=11, **kw)
        m.engine.set_option("mpa_prune", prune)
        pruned = 0
        for it in range(1, 10):
            m.step(it)
            pruned += m.engine.counters()["pruned_rebuilds"]
        pop = m.population
        runs.append(([list(p["path"].cells) for p in pop], [p["fitness"] for p in pop], list(m.convergence_curve_data), pruned))
        m.engine.set_option("mpa_prune", 1)
        m.engine.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    assert runs[0][3] > 0 and runs[1][3] == 0


def test_ga_and_pso_facades_4_connected():
    """GASolver and synchronous PSOSolver with allow_diagonal_moves=False == the same facades with decode + score from the
    oracle."""
    import pathfit, pf_oracle as po
    from test_gpu_solvers import _oracle_backed
    g, s, t = gio.grid("fig7")
    orc4 = po.Oracle(g, 0, 1)
    kw = dict(num_generations=6, population_size=24, num_waypoints_per_chromosome=5, mutation_rate=0.1, crossover_rate=0.8,
              tournament_size=3, turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8,
              diagonal_obstacle_penalty_value=100.0, seed=4, allow_diagonal_moves=False)
    a = pathfit.GASolver(g, **kw)
    ra = a.solve()
    rb = _oracle_backed(pathfit.GASolver, orc4)(g, engine=a.engine, **kw).solve()
    assert ra == rb and ra[0][0] == (0, 0) and ra[0][-1] == (19, 19)
    kw = dict(num_iterations=8, num_particles=32, num_waypoints_per_particle=5, w=0.7, c1=1.5, c2=1.5,
              turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0,
              seed=6, asynchronous=False, allow_diagonal_moves=False)
    a = pathfit.PSOSolver(g, **kw)
    ra = a.solve()
    b = _oracle_backed(pathfit.PSOSolver, orc4)(g, engine=a.engine, **kw)      # same init, then the synchronous sweeps
    assert b._initialize_particles()
    pos, vel, pb, pbf = b._pos.copy(), b._vel.copy(), b._pbest.copy(), b._pbest_fit.copy()
    gb, gfit, gpath = np.array(b.gbest_particle_data["position"]), b.gbest_particle_data["fitness"], b.gbest_particle_data["path"]
    curve = [gfit]
    for it in range(8):
        pos, vel = orc4.pso_update(pos, vel, pb, gb, 0.7, 1.5, 1.5, b.max_vel, 6, it, 0)
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
    cells = np.array([r * 20 + c for r, c in ra[0]])
    assert len(cells) > 1 and (np.abs(np.diff(cells // 20)) + np.abs(np.diff(cells % 20)) == 1).all()


@pytest.mark.parametrize("ad,rs", [(0, 1), (0, 0), (1, 0)])
def test_astar_and_dijkstra_solver_single_queries(ad, rs):
    """AStarSolver / DijkstraSolver.solve return the reference's 6-tuple under the policy they were built with."""
    import pathfit, pf_oracle as po
    g, s, t = gio.grid("fig7")
    o = po.Oracle(g, ad, rs)
    for cls, variant in ((pathfit.AStarSolver, 0), (pathfit.DijkstraSolver, 2)):
        a = cls(g, 0.3, 0.8, 1.8, bool(ad), bool(rs), 100.0)
        for start, target in ((None, None), ((2, 2), (17, 5)), ((0, 4), (3, 3)), ((2, 2), (2, 2))):
            res = a.solve() if start is None else a.solve(start, target)
            sc, tc = (s, t) if start is None else (start[0] * 20 + start[1], target[0] * 20 + target[1])
            want, _ = o.astar(sc, tc, None, variant)
            assert [r * 20 + c for r, c in res[0]] == list(want), (cls.__name__, start, target)
            ws = o.score(want, 0, 0.3, 0.8, 1.8, rs, 100.0)
            assert all(a_ == b_ or (math.isinf(a_) and math.isinf(b_)) for a_, b_ in zip(res[1:], ws)), (cls.__name__, res[1:], ws)


def test_ga_and_mpa_solves_match_reference_4_connected():
    """GASolver.solve and MPA.solve_path_planning of the unmodified reference on fig7 with allow_diagonal_moves=False."""
    import pathfit
    from test_e2e_golden import GA_KW, curve_eq
    z = gio.load("policy_cases")
    g, s, t = gio.grid("fig7")
    ga = pathfit.GASolver(g, seed=4, allow_diagonal_moves=False, **GA_KW)
    res = ga.solve()
    assert [r * 20 + c for r, c in res[0]] == list(z["ga_path"]) and np.array_equal(np.array(res[1:], float), z["ga_stats"])
    assert np.array_equal(np.array(ga.convergence_curve), z["ga_curve"])
    assert np.array_equal([p["fitness"] for p in ga.population], z["ga_pop_fitness"])
    m = pathfit.MPA(g, 30, 20, seed=2, allow_diagonal_moves=False)
    res = m.solve_path_planning()
    assert [r * 20 + c for r, c in res[0]] == list(z["mpa_path"])
    assert np.array_equal(np.array(res[1:], float), z["mpa_stats"]) and curve_eq(m.convergence_curve_data, z["mpa_curve"])
    assert np.array_equal([p["fitness"] for p in m.population], z["mpa_pop_fitness"])
    assert np.array_equal([len(p["path"]) for p in m.population], z["mpa_pop_len"])
