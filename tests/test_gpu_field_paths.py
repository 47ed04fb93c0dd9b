"""Routing trees (pf_dist_field_parents, pf_dist_field_paths, DistanceField.parents / next_hop / paths, DijkstraSolver.solve_many):
the parent maps and the traced paths are DijkstraSolver.solve()'s, cell for cell.  Three things decide: the CPU checkers of
tests/field_checkers.py (a reference-shaped Dijkstra and the field-only rule, pinned against each other by
tests/test_field_parent_rule.py), the variant-2 search batch (Engine.astar_host, an independent device algorithm) and the reference's
goldens.  Every comparison is exact equality of cell arrays, lengths, statuses and fp64 stats."""
import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import thin_maps

pytestmark = pytest.mark.gpu

CANARY = -77


def run(e, sources, ad, rs, kidx, targets, reverse=False, cap=None, want_chosen=False):
    """Raw Engine calls: fields -> parent maps -> one trace -> (parents uint8 [K, R, C], paths, status, lens[, chosen])."""
    K, RC, n = len(sources), e.R * e.C, len(targets)
    cap = int(cap or RC)
    f, p = e.buf((K, RC), np.float64), e.buf((K, RC), np.uint8)
    e.dist_field_batch(sources, f, ad, rs)
    e.dist_field_parents(K, f, p, ad, rs)
    dt = e.put(np.asarray(targets, np.int32))
    dk = e.put(np.asarray(kidx, np.int32)) if kidx is not None else None
    dc, dl, ds, dch = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
    e.dist_field_paths(K, p, dt, n, cap, dc, dl, ds, dk, f, reverse, dch)
    cells, lens, st, ch = dc.download(), dl.download(), ds.download(), dch.download()
    par = p.download().reshape(K, e.R, e.C)
    for b in (f, p, dt, dc, dl, ds, dch) + ((dk,) if dk is not None else ()):
        b.free()
    paths = [cells[i, :lens[i]].copy() for i in range(n)]
    return (par, paths, st, lens, ch) if want_chosen else (par, paths, st, lens)


def same_paths(got, want):
    return len(got) == len(want) and all(np.array_equal(a, np.asarray(b, np.int32)) for a, b in zip(got, want))


def check_all_targets(e, g, sources, ad, rs):
    """Every cell as a target from every source: parent maps, paths, statuses against the checker and the variant-2 batch."""
    mm = fc.move_masks(g, ad, rs)
    RC = g.size
    kidx = np.repeat(np.arange(len(sources)), RC)
    targets = np.tile(np.arange(RC), len(sources))
    par, paths, st, lens = run(e, sources, ad, rs, kidx, targets)
    want = []
    for k, s in enumerate(sources):
        dist, code = fc.reference_dijkstra(g, mm, int(s))
        assert np.array_equal(par[k], code), (ad, rs, k, int(s))
        assert np.array_equal(par[k], fc.rule_parents(dist, mm))
        want += [fc.trace(code, t) for t in range(RC)]
    assert same_paths(paths, want), (ad, rs)
    assert np.array_equal(st, np.array([0 if p else 1 for p in want])) and np.array_equal(lens, [len(p) for p in want])
    spaths, sst = e.astar_host(2, np.asarray(sources, np.int32)[kidx], targets, path_cap=RC, allow_diag=ad, restrict_corner=rs)
    assert same_paths(paths, spaths) and np.array_equal(st, sst), (ad, rs)


# ---- 1. fig7: 32 sources x every cell, the four policies
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_fig7_every_target(ad, rs):
    from pathfit.engine import Engine
    g, _, _ = gio.grid("fig7")
    free = np.flatnonzero(g.reshape(-1) != 1)
    sources = np.random.default_rng(51).choice(free, 32, replace=False)
    e = Engine(g)
    try:
        check_all_targets(e, g, sources, ad, rs)
    finally:
        e.close()


# ---- 2. the reference's goldens
def test_reference_dijkstra_goldens():
    import pathfit
    z = gio.load("dijkstra_cases")
    idx = np.flatnonzero(~z["has_avoid"])
    assert len(idx) == 38 and np.isinf(z["stats"][idx, 0]).sum() == 7
    for gid, name in enumerate(str(s) for s in z["grid_names"]):
        mine = [int(i) for i in idx if z["grid_id"][i] == gid]
        if not mine:
            continue
        g, _, _ = gio.grid(name)
        C = g.shape[1]
        e = pathfit.Engine(g)
        try:
            starts = sorted({int(z["start"][i]) for i in mine})
            kidx = [starts.index(int(z["start"][i])) for i in mine]
            _, paths, st, _ = run(e, starts, 1, 1, kidx, [int(z["target"][i]) for i in mine])
            for j, i in enumerate(mine):
                want = gio.csr_get(z["path_off"], z["path"], i)
                assert np.array_equal(paths[j], want) and st[j] == (0 if len(want) else 1), (name, i)
            sol = pathfit.DijkstraSolver(g, engine=e)
            for s in starts:
                grp = [i for i in mine if int(z["start"][i]) == s]
                res = sol.solve_many([(int(z["target"][i]) // C, int(z["target"][i]) % C) for i in grp], (s // C, s % C))
                for i, r in zip(grp, res):
                    assert [a * C + b for a, b in r[0]] == list(gio.csr_get(z["path_off"], z["path"], i)), (name, i)
                    assert list(r[1:6]) == list(z["stats"][i]), (name, i, r[1:], z["stats"][i])
        finally:
            e.close()


def test_reference_policy_goldens():
    from pathfit.engine import Engine
    z = gio.load("policy_cases")
    checked = 0
    for gid, name in enumerate(str(s) for s in z["grid_names"]):
        g, _, _ = gio.grid(name)
        e = Engine(g)
        try:
            for pi, (ad, rs) in enumerate(z["policies"]):
                idx = np.flatnonzero((z["as_policy"] == pi) & (z["as_grid"] == gid) & (z["as_variant"] == 2) & ~z["as_has_avoid"])
                if not len(idx):
                    continue
                starts = sorted({int(z["as_start"][i]) for i in idx})
                kidx = [starts.index(int(z["as_start"][i])) for i in idx]
                _, paths, st, _ = run(e, starts, int(ad), int(rs), kidx, z["as_target"][idx])
                for j, i in enumerate(idx):
                    want = gio.csr_get(z["as_path_off"], z["as_path"], i)
                    assert np.array_equal(paths[j], want) and st[j] == (0 if len(want) else 1), (name, int(ad), int(rs), int(i))
                    checked += 1
        finally:
            e.close()
    assert checked >= 30


# ---- 3. ties: open maps, a corner and a centre source
@pytest.mark.parametrize("R, C", [(33, 33), (9, 11)])
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_open_map_ties(R, C, ad, rs):
    from pathfit.engine import Engine
    g = np.zeros((R, C), np.uint8)
    e = Engine(g)
    try:
        check_all_targets(e, g, [0, (R // 2) * C + C // 2], ad, rs)
    finally:
        e.close()


# ---- 4. thin maps: a path of ~4096 cells in a row of exactly that many cells, and of one fewer
@pytest.mark.parametrize("R, C", [(1, 4096), (4096, 1), (2, 4096), (4096, 2), (3, 4096), (4096, 3)])
def test_thin_maps_exact_fit(R, C):
    from pathfit.engine import Engine, _View
    g, s, t = thin_maps.thin_map(R, C)
    mm = fc.move_masks(g, 1, 1)
    _, code = fc.reference_dijkstra(g, mm, s)
    want = np.array(fc.trace(code, t), np.int32)
    L = len(want)
    assert L >= 4096 and want[0] == s and want[-1] == t
    e = Engine(g)
    try:
        f, p = e.buf((1, g.size), np.float64), e.buf((1, g.size), np.uint8)
        e.dist_field_batch([s], f, 1, 1)
        e.dist_field_parents(1, f, p, 1, 1)
        assert np.array_equal(p.download().reshape(g.shape), code)
        dt, dk = e.put(np.array([t], np.int32)), e.put(np.zeros(1, np.int32))
        for cap, reverse in ((L, 0), (L, 1), (L - 1, 0), (L - 1, 1)):
            rows = e.put(np.full(3 * L, CANARY, np.int32))            # the query's row lies between two canary rows
            small = [e.put(np.full(3, CANARY, np.int32)) for _ in range(3)]
            row = _View(e, rows.at(L), cap, np.int32)
            dl, ds, dch = (_View(e, b.at(1), 1, np.int32) for b in small)
            e.dist_field_paths(1, p, dt, 1, cap, row, dl, ds, dk, None, reverse, dch)
            got = rows.download()
            ln, st, ch = (b.download() for b in small)
            for b in (ln, st, ch):
                assert b[0] == CANARY and b[2] == CANARY
            assert np.all(got[:L] == CANARY) and np.all(got[2 * L:] == CANARY), (cap, reverse)
            if cap == L:
                assert st[1] == 0 and ln[1] == L and ch[1] == 0
                assert np.array_equal(got[L:2 * L], want[::-1] if reverse else want), (cap, reverse)
            else:
                assert st[1] == 3 and ln[1] == 0 and ch[1] == 0
                assert np.all(got[L:2 * L] == CANARY), (cap, reverse)   # an overflowing query writes nothing
            for b in [rows] + small:
                b.free()
    finally:
        e.close()


# ---- 5. degenerate queries
def room_map():
    g = np.zeros((14, 15), np.uint8)
    g[3, 4:11] = 1; g[9, 4:11] = 1; g[3:10, 4] = 1; g[3:10, 10] = 1   # a sealed 5 x 5 room
    g[12, 1] = 1
    return g


@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_degenerate_queries(ad, rs):
    import pathfit
    from pathfit.engine import Engine
    g = room_map()
    C = g.shape[1]
    outside, inside, wall = 0 * C + 0, 6 * C + 7, 3 * C + 5
    e = Engine(g)
    try:
        # a sealed room (both ways), a target on an obstacle, target == source
        par, paths, st, lens = run(e, [outside, inside], ad, rs, [0, 1, 0, 0, 1, 1], [inside, outside, wall, outside, inside, inside + 1])
        assert st.tolist() == [1, 1, 1, 0, 0, 0] and lens.tolist() == [0, 0, 0, 1, 1, 2]
        assert paths[3].tolist() == [outside] and paths[4].tolist() == [inside] and paths[5].tolist() == [inside, inside + 1]
        assert par[0].reshape(-1)[outside] == 8 and par[1].reshape(-1)[inside] == 8 and (par == 8).sum() == 2
        room = np.zeros(g.shape, bool); room[4:9, 5:10] = True
        assert np.array_equal(par[1] != 255, room) and np.array_equal(par[0] != 255, (g != 1) & ~room)
        # a source on an obstacle: every query is infeasible
        par, paths, st, lens = run(e, [wall], ad, rs, np.zeros(g.size, np.int32), np.arange(g.size))
        assert np.all(par == 255) and np.all(st == 1) and np.all(lens == 0)
        # a field index / a target id out of range: status 1, nothing written; the field each query used
        f, p = e.buf((2, g.size), np.float64), e.buf((2, g.size), np.uint8)
        e.dist_field_batch([outside, inside], f, ad, rs)
        e.dist_field_parents(2, f, p, ad, rs)
        tg = np.array([5, g.size, -1, 5, 5, 2 ** 31 - 1, -2 ** 31, 5], np.int32)
        ki = np.array([0, 0, 1, 2, -1, 0, 0, 2 ** 31 - 1], np.int32)
        n, cap = len(tg), 8
        dt, dk = e.put(tg), e.put(ki)
        dc, dl, ds, dch = (e.put(np.full(s, CANARY, np.int32)) for s in ((n, cap), n, n, n))
        e.dist_field_paths(2, p, dt, n, cap, dc, dl, ds, dk, None, False, dch)
        cells = dc.download()
        assert ds.download().tolist() == [0, 1, 1, 1, 1, 1, 1, 1] and dl.download().tolist() == [6] + [0] * 7
        assert dch.download().tolist() == [0, -1, -1, -1, -1, -1, -1, -1]
        assert cells[0, :6].tolist() == list(range(6)) and np.all(cells[0, 6:] == CANARY) and np.all(cells[1:] == CANARY)
        # the nearest source with out-of-range ids
        e.dist_field_paths(2, p, dt, n, cap, dc.upload(np.full((n, cap), CANARY, np.int32)), dl, ds, None, f, True, dch)
        assert ds.download().tolist() == [0, 1, 1, 0, 0, 1, 1, 0] and dch.download().tolist() == [0, -1, -1, 0, 0, -1, -1, 0]
        assert dc.download()[0, :6].tolist() == list(range(5, -1, -1))
        # n = 0: nothing is launched, nothing is written
        ms = e.last_kernel_ms()
        dc.upload(np.full((n, cap), CANARY, np.int32))
        e.dist_field_paths(2, p, dt, 0, cap, dc, dl, ds, dk, None, False, dch)
        assert e.last_kernel_ms() == ms and np.all(dc.download() == CANARY)
        # argument errors: found on the host, nothing launched
        for bad in (dict(K=0), dict(n=-1), dict(cap=0), dict(p=None), dict(dt=None), dict(dc=None), dict(dl=None), dict(ds=None), dict(dk=None)):
            a = dict(K=2, p=p, dt=dt, n=n, cap=cap, dc=dc, dl=dl, ds=ds, dk=dk)
            a.update(bad)
            with pytest.raises(pathfit.PathfitError, match="pf_dist_field_paths"):
                e.dist_field_paths(a["K"], a["p"], a["dt"], a["n"], a["cap"], a["dc"], a["dl"], a["ds"], a["dk"], None, False, None)
        for K_, f_, p_ in ((0, f, p), (2, None, p), (2, f, None)):
            with pytest.raises(pathfit.PathfitError, match="pf_dist_field_parents"):
                e.dist_field_parents(K_, f_, p_, ad, rs)
        assert e.last_kernel_ms() == ms
        # fields of ANOTHER policy are no fixed point of this one: a message, not a wrong tree
        if (ad, rs) == (0, 1):
            e.dist_field_batch([outside, inside], f, 1, 1)
            with pytest.raises(pathfit.PathfitError, match="no fixed point"):
                e.dist_field_parents(2, f, p, 0, 1)
    finally:
        e.close()


def test_corrupt_map_ends():
    """A parent map that is no tree (a two-cell cycle, a code outside 0..8, a step off the grid): PF_ST_OVERFLOW, never a hang or an
    access out of range."""
    from pathfit.engine import Engine
    g = np.zeros((6, 7), np.uint8)
    e = Engine(g)
    try:
        par = np.full(g.size, 255, np.uint8)
        par[10], par[11] = 1, 0            # 10's parent is 11, 11's parent is 10
        par[20] = 9                        # no move
        par[3] = 2                         # parent = one row up from row 0: cell -4
        par[41] = 3                        # parent = one row down from the last row: cell 48
        par[30], par[29] = 0, 8            # a sound two-cell chain
        p, dt, dk = e.put(par), e.put(np.array([10, 20, 3, 41, 30, 0], np.int32)), e.put(np.zeros(6, np.int32))
        dc, dl, ds = e.put(np.full((6, 50), CANARY, np.int32)), e.buf(6, np.int32), e.buf(6, np.int32)
        e.dist_field_paths(1, p, dt, 6, 50, dc, dl, ds, dk)
        assert ds.download().tolist() == [3, 3, 3, 3, 0, 1] and dl.download().tolist() == [0, 0, 0, 0, 2, 0]
        cells = dc.download()
        assert cells[4, :2].tolist() == [29, 30] and (cells != CANARY).sum() == 2
    finally:
        e.close()


# ---- 6. divergent lanes: one ~2000-cell chain beside one-step chains in the same wavefront
def test_serpentine_divergent_lanes():
    from pathfit.engine import Engine
    g = fc.serpentine(64)
    mm = fc.move_masks(g, 1, 1)
    dist, code = fc.reference_dijkstra(g, mm, 0)
    far = int(np.argmax(np.where(np.isfinite(dist), dist, -1.0)))
    chain = fc.trace(code, far)
    assert len(chain) > 2000 and len(chain) == (g != 1).sum()
    targets = [chain[i] for i in np.linspace(1, len(chain) - 1, 64).astype(int)]
    e = Engine(g)
    try:
        for reverse in (False, True):
            par, paths, st, lens = run(e, [0], 1, 1, np.zeros(64, np.int32), targets, reverse=reverse)
            assert np.array_equal(par[0], code) and np.all(st == 0)
            assert lens[0] == 2 and lens[-1] == len(chain)
            assert same_paths(paths, [fc.trace(code, t)[::-1 if reverse else 1] for t in targets])
    finally:
        e.close()


# ---- 7. the nearest source
@pytest.mark.parametrize("name", ["fig7", "seeded18x23"])
def test_nearest_source(name):
    import pathfit
    g = (gio.grid("fig7")[0] == 1).astype(np.uint8) if name == "fig7" else fc.seeded_map()
    R, C = g.shape
    free = np.flatnonzero(g.reshape(-1) != 1)
    src = [(int(c) // C, int(c) % C) for c in np.random.default_rng(61).choice(free, 5, replace=False)]
    every = [(r, c) for r in range(R) for c in range(C)]
    d = pathfit.DistanceField(g, src)
    try:
        got = d.paths(every)
        chosen = d.chosen.copy()
        fields = d.fields.reshape(5, -1)
        assert np.array_equal(chosen, np.argmin(fields, axis=0))
        assert len(set(chosen.tolist())) > 1
        assert [p.cells.tolist() for p in got] == [p.cells.tolist() for p in d.paths(every, k=chosen.tolist())]
        assert np.array_equal(d.chosen, chosen)
        none = np.isinf(fields).all(axis=0)
        assert none.any() and np.array_equal(d.status, none.astype(np.int32))
        assert all((len(p) == 0) == bool(none[i]) for i, p in enumerate(got))
        mm = fc.move_masks(g, 1, 1)
        codes = [fc.reference_dijkstra(g, mm, r * C + c)[1] for r, c in src]
        assert np.array_equal(d.parents, np.stack(codes)) and d.parents is d.parents
        assert [p.cells.tolist() for p in got] == [fc.trace(codes[chosen[t]], t) for t in range(R * C)]
        back = d.paths(every, reverse=True)
        assert [p.cells.tolist() for p in back] == [p.cells.tolist()[::-1] for p in got]
        # next_hop: the cell before this one on the way from the source; None at the source and where no route ends
        for t in range(R * C):
            k = int(chosen[t])
            p = got[t].tolist()
            assert d.next_hop(k, every[t]) == (p[-2] if len(p) > 1 else None), (t, k)
    finally:
        d.close()


# ---- 8. bench-sized maps
def test_bench_512_against_the_search_batch():
    from pathfit.engine import Engine
    g = gio.upsample(gio.grid("g256")[0], 2)
    free = np.flatnonzero(g.reshape(-1) != 1)
    rnd = np.random.default_rng(71)
    sources = [0, int(rnd.choice(free))]
    targets = np.concatenate([rnd.choice(free, 2048, replace=False) for _ in sources]).astype(np.int32)
    kidx = np.repeat(np.arange(2), 2048)
    e = Engine(g)
    try:
        cap = e.default_path_cap()
        _, paths, st, _ = run(e, sources, 1, 1, kidx, targets, cap=cap)
        spaths, sst = e.astar_host(2, np.asarray(sources, np.int32)[kidx], targets, path_cap=cap)
        assert not (sst == 3).any() and (sst == 0).sum() > 2048
        assert np.array_equal(st, sst) and same_paths(paths, spaths)
    finally:
        e.close()


def test_open_1024_parent_map_obeys_the_rule():
    from pathfit.engine import Engine
    n = 1024
    g = np.zeros((n, n), np.uint8)
    g[300:700, 511] = 1                                               # (a wall, so that some labels go round a corner)
    sources = [0, (n // 2) * n + n // 3, n * n - 1]
    mm = fc.move_masks(g, 1, 1)
    e = Engine(g)
    try:
        f, p = e.buf((3, n * n), np.float64), e.buf((3, n * n), np.uint8)
        e.dist_field_batch(sources, f, 1, 1)
        e.dist_field_parents(3, f, p, 1, 1)
        print(f"1024^2, K = 3: parent map kernel {e.last_kernel_ms():.3f} ms")
        fields, par = f.download().reshape(3, n, n), p.download().reshape(3, n, n)
    finally:
        e.close()
    ids = np.arange(n * n).reshape(n, n)
    for k, s in enumerate(sources):
        D, code = fields[k], par[k]
        assert np.array_equal(code == 255, np.isinf(D)) and np.array_equal(code == 8, ids == s) and D.reshape(-1)[s] == 0.0
        assert np.array_equal(code, fc.rule_parents(D, mm)), k       # no candidate with a smaller (D[u], u)
        for m in range(8):                                            # and, spelt out: D[parent] + w == D[v] across a legal move
            sel = code == m
            assert np.all(((mm >> fc.OPP[m]) & 1)[sel] == 1)
            assert np.array_equal((fc.shifted(D, -fc.DR[m], -fc.DC[m], np.inf) + fc.W[m])[sel], D[sel]), (k, m)


# ---- 9. DijkstraSolver.solve_many
@pytest.mark.parametrize("weights", [dict(turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8, diagonal_obstacle_penalty_value=100.0), {}])
def test_solve_many_is_a_list_of_solves(weights):
    import pathfit
    g, s, _ = gio.grid("fig7")
    R, C = g.shape
    start = (s // C, s % C)
    targets = [(r, c) for r in range(R) for c in range(C)] + [(R, 0), start, None]
    e = pathfit.Engine(g)
    try:
        one, many = pathfit.DijkstraSolver(g, engine=e, **weights), pathfit.DijkstraSolver(g, engine=e, **weights)
        want = [one.solve(start, t) for t in targets]
        got = many.solve_many(targets, start)
        assert len(got) == len(want)
        for t, a, b in zip(targets, got, want):
            assert type(a) is tuple and a == b, (t, a, b)
        assert many.convergence_curve == one.convergence_curve and len(one.convergence_curve) > 100
        other = (R - 1, C - 1)                                        # another start, and the default one
        assert many.solve_many(targets[:60], other) == [one.solve(other, t) for t in targets[:60]]
        assert many.solve_many([None, (0, 0)]) == [one.solve(), one.solve(None, (0, 0))]
        assert many.convergence_curve == one.convergence_curve
    finally:
        e.close()


# ---- 10. lifecycle
def test_lifecycle():
    import pathfit
    g, s, t = gio.grid("fig13")
    R, C = g.shape
    mm = fc.move_masks(g, 1, 1)
    e = pathfit.Engine(g)
    try:
        a = pathfit.DistanceField(g, [(s // C, s % C)], engine=e)
        b = pathfit.DistanceField(g, [(t // C, t % C), (s // C, s % C)], engine=e)
        pa = a.paths([(t // C, t % C)], k=0)[0]                       # a's map is computed, then b's, then a's is read
        pb = b.paths([(s // C, s % C)] * 2, k=[0, 1])
        code_s, code_t = fc.reference_dijkstra(g, mm, s)[1], fc.reference_dijkstra(g, mm, t)[1]
        assert np.array_equal(a.parents[0], code_s) and np.array_equal(b.parents, np.stack([code_t, code_s]))
        assert pa.cells.tolist() == fc.trace(code_s, t) and pb[0].cells.tolist() == fc.trace(code_t, s) and pb[1].cells.tolist() == [s]
        assert a.paths([(t // C, t % C)], k=0, path_cap=len(pa))[0] == pa
        with pytest.raises(pathfit.PathfitError, match="more than path_cap"):
            a.paths([(t // C, t % C)], k=0, path_cap=len(pa) - 1)
        b.close()
        assert e.h and np.array_equal(a.pbuf.download()[0], code_s)   # a borrowed engine stays open, a's map is untouched
        assert a.paths([(t // C, t % C)], k=0)[0] == pa
        a.close()
        assert a.pbuf is None and a.buf is None
        fresh = pathfit.DistanceField(g, [(s // C, s % C)], engine=e)
        fresh.close()
        with pytest.raises(pathfit.PathfitError, match="closed"):
            fresh.parents
        with pytest.raises(pathfit.PathfitError, match="closed"):
            fresh.paths([(0, 0)], k=0)
    finally:
        e.close()
