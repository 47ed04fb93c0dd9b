"""Distance fields (pf_dist_field_batch, Engine.dist_fields_host, pathfit.DistanceField, DijkstraSolver.distance_field): exact
one-to-all path lengths, bit for bit.  Two CPU checkers of this file's own decide: `heap_field`, a plain heap Dijkstra over move
masks computed here from the grid and the policy, and `fixed_point_ok`, a vectorised test that a table is THE fixed point of
D[src] = 0, D[v] = min over legal moves of D[u] + w (unique, the weights being >= 1), which checks a megacell map in milliseconds.
Every comparison is np.array_equal on the doubles: there are no tolerances."""
import heapq
import math

import numpy as np
import pytest

import golden_io as gio
import thin_maps

pytestmark = pytest.mark.gpu

INF = float("inf")
SQRT2 = math.sqrt(2.0)
DR = (0, 0, 1, -1, 1, 1, -1, -1)          # helper.py:30-36 move order
DC = (1, -1, 0, 0, 1, -1, 1, -1)
POLICIES = ((1, 1), (1, 0), (0, 1), (0, 0))


def shifted(a, dr, dc, fill):
    """out[r, c] = a[r + dr, c + dc], `fill` outside."""
    R, C = a.shape
    out = np.full_like(a, fill)
    out[max(0, -dr):R - max(0, dr), max(0, -dc):C - max(0, dc)] = a[max(0, dr):R - max(0, -dr), max(0, dc):C - max(0, -dc)]
    return out


def move_masks(grid, ad, rs):
    """bit k of [r, c]: move k from (r, c) is legal -- target inside and free, the cell itself free; a diagonal needs
    allow_diag and, under restrict_corner, both orthogonal neighbours free."""
    free = np.asarray(grid) != 1
    mm = np.zeros(free.shape, np.uint8)
    for k in range(8 if ad else 4):
        ok = free & shifted(free, DR[k], DC[k], False)
        if k >= 4 and rs:
            ok &= shifted(free, DR[k], 0, False) & shifted(free, 0, DC[k], False)
        mm |= ok.astype(np.uint8) << k
    return mm


def heap_field(grid, mm, src):
    R, C = mm.shape
    dist = [INF] * (R * C)
    if np.asarray(grid).reshape(-1)[src] == 1:
        return np.array(dist).reshape(R, C)
    m = mm.reshape(-1).tolist()
    step = [DR[k] * C + DC[k] for k in range(8)]
    w = [1.0] * 4 + [SQRT2] * 4
    dist[src] = 0.0
    pq = [(0.0, src)]
    while pq:
        d, u = heapq.heappop(pq)
        if d > dist[u]:
            continue
        mu = m[u]
        for k in range(8):
            if (mu >> k) & 1:
                t, v = d + w[k], u + step[k]
                if t < dist[v]:
                    dist[v] = t
                    heapq.heappush(pq, (t, v))
    return np.array(dist).reshape(R, C)


def fixed_point_ok(grid, mm, src, field):
    """field is the fixed point: 0 at the source, inf on obstacles, every other free cell the minimum of neighbour + w over its
    own mask (the graph is symmetric: v's mask lists the moves INTO v reversed)."""
    g = np.asarray(grid)
    R, C = g.shape
    if field.shape != (R, C) or np.isnan(field).any():
        return False
    if g.reshape(-1)[src] == 1:
        return bool(np.all(np.isinf(field)))
    best = np.full((R, C), INF)
    for k in range(8):
        cand = shifted(field, DR[k], DC[k], INF) + (1.0 if k < 4 else SQRT2)
        best = np.where((mm >> k) & 1 == 1, np.minimum(best, cand), best)
    best.reshape(-1)[src] = 0.0
    best[g == 1] = INF
    return bool(np.array_equal(field, best) and field.reshape(-1)[src] == 0.0)


def test_checkers_on_the_cpu():
    """The checkers themselves: the fixed-point test accepts heap_field's table and rejects a one-ulp bump of one entry."""
    g, s, _ = gio.grid("fig7")
    for ad, rs in POLICIES:
        mm = move_masks(g, ad, rs)
        f = heap_field(g, mm, s)
        assert fixed_point_ok(g, mm, s, f)
        bad = f.copy()
        i = np.flatnonzero(np.isfinite(f.reshape(-1)) & (f.reshape(-1) > 0))[7]
        bad.reshape(-1)[i] = np.nextafter(bad.reshape(-1)[i], INF)
        assert not fixed_point_ok(g, mm, s, bad)


def sealed_rooms():
    """The 96 x 96 map of test_gpu_move_policies.py: a sealed 40 x 40 room and a second room that leaks diagonally at a corner."""
    rnd = np.random.default_rng(9)
    g = (rnd.random((96, 96)) < 0.08).astype(np.uint8)
    g[20:62, 30] = 1; g[20:62, 71] = 1; g[20, 30:72] = 1; g[61, 30:72] = 1
    g[70:90, 5:8] = 1; g[70, 5:30] = 1; g[89, 5:30] = 1; g[70:90, 29] = 1
    g[89, 29] = 0; g[88, 29] = 1; g[89, 28] = 1
    return g


def check_against_heap(e, g, sources, ad, rs):
    mm = move_masks(g, ad, rs)
    got, info = e.dist_fields_host(sources, ad, rs, want_info=True)
    for k, s in enumerate(sources):
        want = heap_field(g, mm, int(s))
        assert np.array_equal(got[k], want), (ad, rs, k, int(s))
        assert info[k, 1] == np.isfinite(want).sum(), (ad, rs, k, info[k])
    return got, info


# ---- 1. every cell of fig7 as a source: K = 400 is above the CU count, so the persistent loop and the slot reuse run
@pytest.mark.parametrize("ad, rs", POLICIES)
def test_every_cell_of_fig7(ad, rs):
    from pathfit.engine import Engine
    g, _, _ = gio.grid("fig7")
    e = Engine(g)
    try:
        got, _ = check_against_heap(e, g, np.arange(g.size), ad, rs)
        for s in np.flatnonzero(g.reshape(-1) == 1):
            assert np.all(np.isinf(got[s])), s
    finally:
        e.close()


# ---- 1b. the one level kernel behind both entry points: single sources are sets of one
def wall_and_pocket():
    """9 x 11: a wall across the map with a one-cell gap, and a sealed one-cell pocket."""
    g = np.zeros((9, 11), np.uint8)
    g[4, :] = 1
    g[4, 7] = 0
    g[0:3, 0:3] = 1
    g[1, 1] = 0
    return g


@pytest.fixture(scope="module")
def compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count.  torch brings a HIP runtime of its own, and it finds no GPU once
    the library's runtime has started in this process (whichever test ran first decides), so then a child process asks torch."""
    import subprocess
    import sys
    ask = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except RuntimeError:
        return int(subprocess.run([sys.executable, "-c", ask], check=True, capture_output=True, text=True, timeout=120).stdout.split()[-1])


@pytest.mark.parametrize("ad, rs", [(1, 1), (0, 0)])
def test_more_sources_than_workgroups(compute_units, ad, rs):
    """K = 2 CUs + 3 single sources: every workgroup loops at least twice and the control block {error word, off[K + 1], ids}
    outgrows its first allocation of 64 words.  The sources cycle through all 99 cells: obstacle cells and repeats are among them."""
    from pathfit.engine import Engine
    g = wall_and_pocket()
    K = 2 * compute_units + 3
    sources = np.arange(K) % g.size
    assert K > g.size and (g.reshape(-1)[sources] == 1).any()
    e = Engine(g)
    try:
        got, info = check_against_heap(e, g, sources, ad, rs)
        for k in np.flatnonzero(g.reshape(-1)[sources] == 1):
            assert np.all(np.isinf(got[k])), k
            assert info[k].tolist() == [0, 0, 0, 0], (k, info[k])
    finally:
        e.close()


def test_unit_sets_equal_the_batch():
    """pf_dist_field_merged with K sets of one source each against pf_dist_field_batch with the same K sources: the fields bytewise,
    the schedule-independent info words (levels, cells reached, offers) exactly; a cell is appended at most twice."""
    from pathfit.engine import Engine
    g = wall_and_pocket()
    C = g.shape[1]
    sources = np.array([0 * C + 5, 1 * C + 1, 4 * C + 7, 4 * C + 2, 8 * C + 10, 0 * C + 5, 6 * C + 3], np.int32)   # the pocket, the gap, a wall cell, a repeat
    assert len(sources) == 7 and g.reshape(-1)[sources[3]] == 1 and sources[5] == sources[0]
    e = Engine(g)
    try:
        for ad, rs in POLICIES:
            batch, binfo = e.dist_fields_host(sources, ad, rs, want_info=True)
            out, dinfo = e.buf((7, g.size), np.float64), e.buf((7, 4), np.int64)
            try:
                e.dist_field_merged(np.arange(8), sources, out, ad, rs, dinfo)
                merged, minfo = out.download(), dinfo.download()
            finally:
                out.free()
                dinfo.free()
            assert merged.tobytes() == batch.tobytes(), (ad, rs)
            assert np.array_equal(minfo[:, :3], binfo[:, :3]), (ad, rs, minfo, binfo)
            for info in (minfo, binfo):
                assert np.all(info[:, 1] <= info[:, 3]) and np.all(info[:, 3] <= 2 * info[:, 1]), (ad, rs, info)
            assert binfo[3].tolist() == [0, 0, 0, 0] and np.all(np.isinf(batch[3]))
    finally:
        e.close()


# ---- 2. thin maps
@pytest.mark.parametrize("R, C", [(1, 1), (1, 4095), (4095, 1), (2, 300), (3, 300)])
def test_thin_maps(R, C):
    from pathfit.engine import Engine
    g, _, _ = thin_maps.thin_map(R, C, obstacles=thin_maps.has_obstacle_version(R, C))
    flat = g.reshape(-1)
    sources = sorted({0, g.size - 1, g.size // 2, (g.size // 2 + C // 3) % g.size})
    obst = np.flatnonzero(flat == 1)
    if obst.size:
        sources += [int(obst[0]), int(obst[-1])]
        assert any(flat[s] != 1 for s in sources)
    e = Engine(g)
    try:
        for ad, rs in POLICIES:
            got, _ = check_against_heap(e, g, sources, ad, rs)
            for k, s in enumerate(sources):
                if flat[s] == 1:
                    assert np.all(np.isinf(got[k]))
    finally:
        e.close()


# ---- 3. g128crop and the sealed rooms, 16 sources inside and outside the rooms
@pytest.mark.parametrize("ad, rs", POLICIES)
def test_g128crop(ad, rs):
    from pathfit.engine import Engine
    g, s, t = gio.grid("g128crop")
    free = np.flatnonzero(g.reshape(-1) != 1)
    sources = np.concatenate([[s, t], np.random.default_rng(5).choice(free, 14, replace=False)])
    e = Engine(g)
    try:
        check_against_heap(e, g, sources, ad, rs)
    finally:
        e.close()


@pytest.mark.parametrize("ad, rs", POLICIES)
def test_sealed_rooms(ad, rs):
    from pathfit.engine import Engine
    g = sealed_rooms()
    rnd = np.random.default_rng(11)
    free = np.flatnonzero(g.reshape(-1) != 1)
    rr, cc = free // 96, free % 96
    inside = free[(20 < rr) & (rr < 61) & (30 < cc) & (cc < 71)]
    room2 = free[(70 < rr) & (rr < 89) & (7 < cc) & (cc < 29)]
    outside = np.setdiff1d(free, np.concatenate([inside, room2]))
    sources = np.concatenate([rnd.choice(inside, 5, replace=False), rnd.choice(room2, 5, replace=False), rnd.choice(outside, 6, replace=False)])
    e = Engine(g)
    try:
        got, _ = check_against_heap(e, g, sources, ad, rs)
    finally:
        e.close()
    room = np.zeros(g.shape, bool)
    room[21:61, 31:71] = True
    room &= g != 1
    for k in range(5):                                                # a source inside the sealed room reaches its room and nothing else
        assert np.array_equal(np.isfinite(got[k]), room), (ad, rs, k)  # (on this map no free room cell is walled in, 4-connected included)
    leak = np.isfinite(got[5:10])[:, outside // 96, outside % 96].any()
    assert leak == bool(ad and not rs), (ad, rs)                      # the second room leaks only by cutting its corner


# ---- 4. bucket boundaries and list capacity: an open 1400 x 1400 map (more than five times the workgroup size on a side)
def test_open_map_bucket_edges_and_list_capacity():
    from pathfit.engine import Engine
    n = 1400
    g = np.zeros((n, n), np.uint8)
    centre, corner = (n // 2) * n + n // 2, 0
    e = Engine(g)
    try:
        rr, cc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        for ad, rs in ((0, 1), (1, 1)):
            got, info = e.dist_fields_host([centre, corner], ad, rs, want_info=True)
            mm = move_masks(g, ad, rs)
            for k, s in enumerate((centre, corner)):
                f = got[k]
                if not ad:                                            # every label is an integer: exactly on a bucket edge
                    assert np.array_equal(f, (np.abs(rr - s // n) + np.abs(cc - s % n)).astype(np.float64)), (ad, k)
                else:
                    assert fixed_point_ok(g, mm, s, f), (ad, k)
                levels, settled, offered, appends = (int(v) for v in info[k])
                print(f"open {n}^2 policy ({ad}, {rs}) source {s}: levels {levels} settled {settled} offered {offered} appends {appends}")
                assert settled == np.isfinite(f).sum() == n * n
                assert settled - 1 <= appends <= 2 * settled
                assert levels <= math.floor(f[np.isfinite(f)].max()) + 1
                assert offered >= settled - 1
    finally:
        e.close()


# ---- 5. bench-size maps
def bench_map(k):
    return gio.upsample(gio.grid("g256")[0], k)


@pytest.fixture(scope="module")
def e512():
    from pathfit.engine import Engine
    g = bench_map(2)
    e = Engine(g)
    yield e, g
    e.close()


@pytest.mark.parametrize("ad, rs", [(1, 1), (0, 1)])
def test_bench_512_fixed_point(e512, ad, rs):
    e, g = e512
    free = np.flatnonzero(g.reshape(-1) != 1)
    sources = [0, g.size - 1] + [int(c) for c in np.random.default_rng(21).choice(free, 2, replace=False)]
    got, info = e.dist_fields_host(sources, ad, rs, want_info=True)
    mm = move_masks(g, ad, rs)
    for k, s in enumerate(sources):
        assert fixed_point_ok(g, mm, s, got[k]), (ad, rs, k)
        assert info[k, 1] == np.isfinite(got[k]).sum()
    print(f"512^2 ({ad}, {rs}): kernel {e.last_kernel_ms():.3f} ms, levels {info[:, 0].tolist()}")


@pytest.mark.parametrize("ad, rs", [(1, 1), (0, 1)])
def test_bench_1024_fixed_point(ad, rs):
    from pathfit.engine import Engine
    g = bench_map(4)
    e = Engine(g)
    try:
        got, info = e.dist_fields_host([0], ad, rs, want_info=True)
        assert fixed_point_ok(g, move_masks(g, ad, rs), 0, got[0])
        print(f"1024^2 ({ad}, {rs}): kernel {e.last_kernel_ms():.3f} ms, levels {int(info[0, 0])}")
    finally:
        e.close()


def test_bench_512_lengths_of_dijkstra_paths(e512):
    """field[S][t] is the length of DijkstraSolver's path S -> t: the engine's own search scored by the engine, and the oracle's
    (pinned to the reference) scored by the oracle; an empty path is inf."""
    import pf_oracle as po
    from pathfit.engine import score_params
    e, g = e512
    S = 0
    free = np.flatnonzero(g.reshape(-1) != 1)
    targets = np.random.default_rng(22).choice(free, 48, replace=False)
    field = e.dist_fields_host([S], 1, 1)[0].reshape(-1)
    paths, st = e.astar_host(2, [S] * 48, targets, path_cap=g.size)
    stats = e.score_host(paths, score_params(0))
    o = po.Oracle(g)
    for i, t in enumerate(targets):
        assert st[i] != 3
        assert field[t] == stats[i, 0], (i, int(t), field[t], stats[i, 0])
        want, _ = o.astar(S, int(t), None, 2)
        assert field[t] == o.score(want)[0], (i, int(t))
        assert (len(want) == 0) == math.isinf(field[t])


# ---- 6 / 7. the reference's goldens
def test_reference_dijkstra_goldens():
    from pathfit.engine import Engine
    z = gio.load("dijkstra_cases")
    idx = np.flatnonzero(~z["has_avoid"])
    assert len(idx) == 38 and np.isinf(z["stats"][idx, 0]).sum() == 7
    for gid, name in enumerate(str(s) for s in z["grid_names"]):
        mine = [i for i in idx if z["grid_id"][i] == gid]
        if not mine:
            continue
        g, _, _ = gio.grid(name)
        e = Engine(g)
        try:
            starts = sorted({int(z["start"][i]) for i in mine})
            f = e.dist_fields_host(starts, 1, 1).reshape(len(starts), -1)
            for i in mine:
                got = f[starts.index(int(z["start"][i])), int(z["target"][i])]
                assert got == z["stats"][i, 0], (name, i, got, z["stats"][i, 0])
        finally:
            e.close()


def test_reference_policy_goldens():
    """Variant 2 (DijkstraSolver) cases without an avoid set under (1, 0), (0, 1), (0, 0): the expected length is the
    left-to-right fp64 sum over the golden path's steps."""
    from pathfit.engine import Engine
    z = gio.load("policy_cases")
    names = [str(s) for s in z["grid_names"]]
    checked = 0
    for gid, name in enumerate(names):
        g, _, _ = gio.grid(name)
        C = g.shape[1]
        e = Engine(g)
        try:
            for pi, (ad, rs) in enumerate(z["policies"]):
                idx = np.flatnonzero((z["as_policy"] == pi) & (z["as_grid"] == gid) & (z["as_variant"] == 2) & ~z["as_has_avoid"])
                if not len(idx):
                    continue
                starts = sorted({int(z["as_start"][i]) for i in idx})
                f = e.dist_fields_host(starts, int(ad), int(rs)).reshape(len(starts), -1)
                for i in idx:
                    p = gio.csr_get(z["as_path_off"], z["as_path"], i)
                    want = INF
                    if len(p):
                        want = 0.0
                        for a, b in zip(p[:-1], p[1:]):
                            want += 1.0 if (a // C == b // C or a % C == b % C) else SQRT2
                    got = f[starts.index(int(z["as_start"][i])), int(z["as_target"][i])]
                    assert got == want, (name, int(ad), int(rs), i, got, want)
                    checked += 1
        finally:
            e.close()
    assert checked >= 30


# ---- 8. Engine.update_grid
def test_update_grid_opens_a_door():
    from pathfit.engine import Engine
    g = sealed_rooms()
    inside, outside = 40 * 96 + 50, 5 * 96 + 5
    assert g[40, 50] != 1 and g[5, 5] != 1
    e = Engine(g)
    try:
        before, _ = check_against_heap(e, g, [inside, outside], 1, 1)
        assert np.isinf(before[0, 5, 5]) and np.isinf(before[1, 40, 50])
        g2 = g.copy()
        g2[40, 29:32] = 0
        e.update_grid(g2)
        after, _ = check_against_heap(e, g2, [inside, outside], 1, 1)
        assert np.isfinite(after[0, 5, 5]) and np.isfinite(after[1, 40, 50])
        assert not np.array_equal(before, after)
    finally:
        e.close()


# ---- 9. call sequences, argument errors, the facades
def test_call_sequence_and_argument_errors():
    import pathfit
    from pathfit.engine import Engine
    g, s, t = gio.grid("g128crop")
    free = np.flatnonzero(g.reshape(-1) != 1)
    rnd = np.random.default_rng(31)
    calls = [([s], 1, 1), (rnd.choice(free, 300, replace=False), 0, 1), ([t, s], 1, 0), ([t], 0, 0)]
    e = Engine(g)
    try:
        for src, ad, rs in calls:
            got = e.dist_fields_host(src, ad, rs)
            fresh = Engine(g)
            try:
                assert np.array_equal(got, fresh.dist_fields_host(src, ad, rs)), (len(src), ad, rs)
            finally:
                fresh.close()
        out = e.buf((1, g.size), np.float64)
        ms = e.last_kernel_ms()
        for bad in ([], [g.size], [-1], [s, g.size]):
            with pytest.raises(pathfit.PathfitError, match="pf_dist_field_batch"):
                e.dist_field_batch(bad, out)
        assert e.last_kernel_ms() == ms                               # nothing was launched
        with pytest.raises(pathfit.PathfitError):
            e._ck(e.L.pf_dist_field_batch(e.h, 1, 1, 1, np.array([s], np.int32).ctypes.data, None, None))
        out.free()
    finally:
        e.close()


def test_facades_return_the_same_arrays():
    import pathfit
    g, s, t = gio.grid("fig13")
    C = g.shape[1]
    e = pathfit.Engine(g)
    try:
        for ad, rs in POLICIES:
            want = e.dist_fields_host([t, s], ad, rs)
            d = pathfit.DistanceField(g, [(t // C, t % C), (s // C, s % C)], allow_diagonal_moves=ad, restrict_diagonal_near_obstacle=rs, engine=e)
            assert d.length(1, (t // C, t % C)) == want[1].reshape(-1)[t]          # (one entry, before the download)
            assert np.array_equal(d.fields, want) and d.fields is d.fields
            assert np.array_equal(d.reachable(0), np.isfinite(want[0]))
            assert d.length(0, (s // C, s % C)) == want[0].reshape(-1)[s]
            assert np.array_equal(d.buf.download(), want)
            d.close()
            assert e.h                                                # a borrowed engine stays open
            sol = pathfit.DijkstraSolver(g, allow_diagonal_moves=bool(ad), restrict_diagonal_near_obstacle_policy=bool(rs), engine=e)
            assert np.array_equal(sol.distance_field(), want[1])
            assert np.array_equal(sol.distance_field((t // C, t % C)), want[0])
        d = pathfit.DistanceField(g)                                  # the target marker, an engine of its own
        assert d.sources == [(t // C, t % C)] and np.array_equal(d.fields[0], e.dist_fields_host([t])[0])
        own = d.engine
        d.close()
        assert not own.h
        with pytest.raises(pathfit.PathfitError, match="closed"):
            d.length(0, (0, 0)) if d._fields is None else d._check_open()
    finally:
        e.close()


# ---- 10. the MPA opt-in: bound tables from the device
KW = dict(turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty=100.0)


def _pop_rows(pop):
    return [(p["path"].cells.tolist(), p["turns"], np.array([p["length"], p["safety_penalty"], p["diag_penalty"], p["fitness"]]).view(np.uint64).tolist())
            for p in pop]


def test_mpa_bounds_from_the_device():
    import pathfit
    g, s, t = gio.grid("g256")
    C = g.shape[1]
    free = np.flatnonzero(g.reshape(-1) != 1)
    rnd = np.random.default_rng(41)
    rc = lambda c: (int(c) // C, int(c) % C)
    a, b_, c_ = (rc(v) for v in rnd.choice(free, 3, replace=False))
    starts, targets = [rc(s), a, rc(s), c_], [rc(t), rc(t), b_, a]     # mixed: shared and distinct endpoints
    seeds, N, iters = [5, 6, 7, 8], 24, 9
    runs = {}
    e = pathfit.Engine(g)
    try:
        for dev in (1, 0):
            e.set_option("mpa_bounds_device", dev)
            m = pathfit.MPA(g, N, iters, seed=3, engine=e, **KW)
            m._sort()
            slot, s0 = m._best_row()
            m._take_first(s0, m._fetch(slot))
            pruned = 0
            for it in range(1, iters + 1):
                m.step(it)
                pruned += e.counters()["pruned_rebuilds"]
            solo = (_pop_rows(m.population), list(m.convergence_curve_data), pruned)
            b = pathfit.MPABatch(g, N, iters, seeds=seeds, starts=starts, targets=targets, engine=e, **KW)
            b.begin()
            bpruned = 0
            for it in range(1, iters + 1):
                b.step(it)
                bpruned += b.counters()[0]["pruned_rebuilds"]
            batch = ([_pop_rows(b.school(k).population) for k in range(4)], [list(b.school(k).convergence_curve_data) for k in range(4)], bpruned)
            b.close()
            runs[dev] = (solo, batch)
            assert pruned > 0 and bpruned > 0, (dev, pruned, bpruned)
    finally:
        e.set_option("mpa_bounds_device", 0)
        e.close()
    assert runs[1] == runs[0]
