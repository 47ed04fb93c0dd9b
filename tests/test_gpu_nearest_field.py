"""Nearest-source fields (pf_dist_field_merged, pf_dist_field_owners, pathfit.NearestSourceField): the merged field, the parent maps,
the owner of every cell, the territory sizes and the traced paths against the CPU checkers of tests/nearest_checkers.py (a
reference-shaped Dijkstra seeded with the whole set and an owner tracer, pinned by tests/test_nearest_owner_rule.py), against the
elementwise minimum of pf_dist_field_batch's rows and against pf_score_batch.  Every comparison is exact equality; every output
buffer lies between two canary rows."""
import numpy as np
import pytest

import field_checkers as fc
import golden_io as gio
import nearest_checkers as nc
import thin_maps

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 16                                                             # canary words in front of and behind the counts / the info block


def run(e, sets, ad, rs, with_info=True):
    """Raw Engine calls, every output between canaries: merged fields -> parent maps -> owners and counts
    -> dict(fields [B, R, C], parents, owners, counts [N], info [B, 4], bufs to free)."""
    from pathfit.engine import _View
    B, RC = len(sets), e.R * e.C
    off, ids = nc.csr(sets)
    N = len(ids)
    f = e.put(np.full((B + 2, RC), float(CANARY)))
    p = e.put(np.full((B + 2, RC), 0x5A, np.uint8))
    o = e.put(np.full((B + 2, RC), CANARY, np.int32))
    c = e.put(np.full(N + 2 * PAD, CANARY, np.int64))
    i = e.put(np.full(4 * B + 2 * PAD, CANARY, np.int64))
    fv, pv, ov = (_View(e, b.at(RC), B * RC, b.dtype) for b in (f, p, o))
    cv, iv = _View(e, c.at(PAD), N, np.int64), _View(e, i.at(PAD), 4 * B, np.int64)
    e.dist_field_merged(off, ids, fv, ad, rs, iv)
    ms = [e.last_kernel_ms()]
    e.dist_field_parents(B, fv, pv, ad, rs)
    ms.append(e.last_kernel_ms())
    e.dist_field_owners(off, ids, pv, ov, iv if with_info else None, cv)
    ms.append(e.last_kernel_ms())
    out = {}
    for name, b, fill in (("fields", f, float(CANARY)), ("parents", p, 0x5A), ("owners", o, CANARY)):
        a = b.download()
        assert np.all(a[0] == fill) and np.all(a[-1] == fill), name
        out[name] = a[1:-1].reshape(B, e.R, e.C)
    for name, b in (("counts", c), ("info", i)):
        a = b.download()
        assert np.all(a[:PAD] == CANARY) and np.all(a[-PAD:] == CANARY), name
        out[name] = a[PAD:-PAD]
    out["info"] = out["info"].reshape(B, 4)
    out.update(off=off, ids=ids, ms=ms, views=(fv, pv, ov), bufs=(f, p, o, c, i))
    return out


def free(res):
    for b in res["bufs"]:
        b.free()


def want_of(g, mm, sources):
    merged, code = nc.multi_dijkstra(g, mm, sources)
    own, count = nc.owners_of(code, sources)
    return merged, code, own, count


def check(g, sets, ad, rs, res, wants=None):
    """Fields, parents, owners, counts and the info block of every set against the checkers -> the checkers' answers."""
    mm = fc.move_masks(g, ad, rs)
    wants = wants or [want_of(g, mm, s) for s in sets]
    for b, (merged, code, own, count) in enumerate(wants):
        tag = (ad, rs, b)
        assert np.array_equal(res["fields"][b], merged), tag
        assert np.array_equal(res["parents"][b], code), tag
        assert np.array_equal(res["owners"][b], own), tag
        assert np.array_equal(res["counts"][res["off"][b]:res["off"][b + 1]], count), tag
        finite = merged[np.isfinite(merged)]
        levels, reached, offers, appends = res["info"][b]
        assert levels == len(np.unique(np.floor(finite))) and reached == finite.size, tag
        assert reached <= appends <= 2 * max(reached, 1) and offers == sum(int(((mm >> k) & 1)[np.isfinite(merged)].sum()) for k in range(8)), tag
    return wants


def trace_all(e, res, B, targets, kidx, cap, reverse=False):
    """pf_dist_field_paths through the merged parent maps -> (paths, status)."""
    fv, pv, _ = res["views"]
    n = len(targets)
    dt, dk = e.put(np.asarray(targets, np.int32)), e.put(np.asarray(kidx, np.int32))
    dc, dl, ds = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
    e.dist_field_paths(B, pv, dt, n, cap, dc, dl, ds, dk, None, reverse, None)
    cells, lens, st = dc.download(), dl.download(), ds.download()
    for b in (dt, dk, dc, dl, ds):
        b.free()
    return [cells[q, :lens[q]] for q in range(n)], st


# ---- 1. fig7: 300 sets in one launch (more sets than CUs), the four policies, every cell a target
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_fig7_many_sets(ad, rs):
    from pathfit.engine import Engine
    g = (gio.grid("fig7")[0] == 1).astype(np.uint8)
    RC = g.size
    walls = [int(v) for v in np.flatnonzero(g.reshape(-1) == 1)]
    rnd = np.random.default_rng(91)
    sets = nc.seeded_sets(g, rnd.integers(1, 7, 300), seed=92)
    sets[3] = sets[3] + [sets[3][0]]                                  # a source listed twice
    sets[7] = [sets[7][0], walls[5]] + sets[7][1:]                    # an obstacle cell among the sources
    sets[11] = walls[:3]                                              # obstacle cells only
    assert {len(s) for s in sets} >= {1, 2, 3, 4, 5, 6}
    e = Engine(g)
    try:
        res = run(e, sets, ad, rs)
        wants = check(g, sets, ad, rs, res)
        assert np.all(np.isinf(res["fields"][11])) and np.all(res["owners"][11] == -1) and np.all(res["counts"][res["off"][11]:res["off"][12]] == 0)
        assert res["counts"][res["off"][3] + len(sets[3]) - 1] == 0 and res["counts"][res["off"][7] + 1] == 0
        # the elementwise minimum of the single-source rows, and the owner's own row
        single = e.dist_fields_host(res["ids"], ad, rs).reshape(len(res["ids"]), RC)
        for b in range(len(sets)):
            rows = single[res["off"][b]:res["off"][b + 1]]
            merged, own = res["fields"][b].reshape(-1), res["owners"][b].reshape(-1)
            assert np.array_equal(merged, rows.min(axis=0)), (ad, rs, b)
            reach = own >= 0
            assert np.array_equal(rows[own[reach], np.flatnonzero(reach)], merged[reach]), (ad, rs, b)
        # every cell a target of every set
        want_paths = [fc.trace(code, t) for _, code, _, _ in wants for t in range(RC)]
        cap = max(len(p) for p in want_paths)
        paths, st = trace_all(e, res, len(sets), np.tile(np.arange(RC), len(sets)), np.repeat(np.arange(len(sets)), RC), cap)
        assert np.array_equal(st, [0 if p else 1 for p in want_paths])
        assert all(np.array_equal(a, b) for a, b in zip(paths, want_paths)), (ad, rs)
        free(res)
    finally:
        e.close()


# ---- 2. every free cell a source
def test_fig7_every_free_cell_a_source():
    from pathfit.engine import Engine
    g = (gio.grid("fig7")[0] == 1).astype(np.uint8)
    cells = [int(v) for v in np.flatnonzero(g.reshape(-1) != 1)]
    e = Engine(g)
    try:
        res = run(e, [cells], 1, 1)
        check(g, [cells], 1, 1, res)
        assert np.array_equal(res["fields"][0], np.where(g == 1, np.inf, 0.0))
        assert np.array_equal(res["owners"][0].reshape(-1)[cells], np.arange(len(cells))) and np.all(res["counts"] == 1)
        assert res["info"][0].tolist()[:2] == [1, len(cells)] and res["info"][0][3] == len(cells)
        free(res)
    finally:
        e.close()


# ---- 3. more seeds than threads, more than one pass of 128 entries, adjacent seeds, ties between owners
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_open_40_many_seeds(ad, rs):
    from pathfit.engine import Engine
    g = np.zeros((40, 40), np.uint8)
    sources = nc.seeded_sets(g, [1300], seed=93)[0]
    sources += [sources[i] for i in np.random.default_rng(94).choice(1300, 50, replace=False)]
    e = Engine(g)
    try:
        res = run(e, [sources], ad, rs)
        (merged, _, own, count), = check(g, [sources], ad, rs, res)
        assert (count[1300:] == 0).all() and (count > 1).any() and merged.max() >= 1.0
        free(res)
    finally:
        e.close()


# ---- 4. thin maps: sources at the ends and in the middle
@pytest.mark.parametrize("R, C", [(1, 64), (64, 1), (2, 200), (3, 200)])
def test_thin_maps(R, C):
    from pathfit.engine import Engine
    g, _, _ = thin_maps.thin_map(R, C, obstacles=R > 1)
    g = (g == 1).astype(np.uint8)
    sets = [[0, R * C - 1, (R // 2) * C + C // 2], [R * C - 1], [(R // 2) * C + C // 2, 0]]
    e = Engine(g)
    try:
        for ad, rs in fc.POLICIES:
            res = run(e, sets, ad, rs)
            wants = check(g, sets, ad, rs, res)
            targets = np.arange(R * C)
            paths, st = trace_all(e, res, len(sets), targets, np.zeros(R * C, np.int32), R * C, reverse=True)
            want = [fc.trace(wants[0][1], int(t))[::-1] for t in targets]
            assert np.array_equal(st, [0 if p else 1 for p in want]) and all(np.array_equal(a, b) for a, b in zip(paths, want)), (ad, rs)
            free(res)
    finally:
        e.close()


# ---- 5. sealed rooms
def rooms_map():
    g = np.zeros((14, 27), np.uint8)
    for c0 in (3, 15):                                                # two sealed 5 x 5 rooms
        g[3, c0:c0 + 7] = 1; g[9, c0:c0 + 7] = 1; g[3:10, c0] = 1; g[3:10, c0 + 6] = 1
    return g


@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_sealed_rooms(ad, rs):
    from pathfit.engine import Engine
    g = rooms_map()
    C = g.shape[1]
    outside, in_a, in_b, wall = 0, 6 * C + 6, 6 * C + 18, 3 * C + 4
    sets = [[outside, in_a, wall], [in_b]]
    e = Engine(g)
    try:
        res = run(e, sets, ad, rs)
        check(g, sets, ad, rs, res)
        room_a = np.zeros(g.shape, bool); room_a[4:9, 4:9] = True
        room_b = np.zeros(g.shape, bool); room_b[4:9, 16:21] = True
        f, p, o = res["fields"], res["parents"], res["owners"]
        assert np.all(np.isinf(f[0][room_b])) and np.all(p[0][room_b] == 255) and np.all(o[0][room_b] == -1)     # the room without a source
        assert np.all(o[0][room_a] == 1) and res["counts"].tolist()[:3] == [int(((g != 1) & ~room_a & ~room_b).sum()), 25, 0]
        assert np.array_equal(o[1] == 0, room_b) and res["counts"][3] == 25
        paths, st = trace_all(e, res, 2, [in_b, in_b + 1, in_a + 1, wall, in_b + 1], [0, 0, 0, 0, 1], g.size)
        assert st.tolist() == [1, 1, 0, 1, 0] and [len(q) for q in paths] == [0, 0, 2, 0, 2]
        assert paths[2].tolist() == [in_a, in_a + 1] and paths[4].tolist() == [in_b, in_b + 1]
        free(res)
    finally:
        e.close()


# ---- 6. serpentine 32 x 32: chains of about 500 cells stress the round count of the doubling
def test_serpentine_rounds():
    from pathfit.engine import Engine
    g = fc.serpentine(32)
    free_cells = np.flatnonzero(g.reshape(-1) != 1)
    mm = fc.move_masks(g, 1, 1)
    dist, _ = fc.reference_dijkstra(g, mm, 0)
    order = free_cells[np.argsort(dist.reshape(-1)[free_cells])]      # the corridor, end to end
    assert len(order) > 500
    three = [int(order[0]), int(order[101]), int(order[314])]         # chains of unequal, odd lengths
    e = Engine(g)
    try:
        for sets in ([[0]], [three], [[0], three, [int(order[-1])]]):
            res = run(e, sets, 1, 1, with_info=True)
            wants = check(g, sets, 1, 1, res)
            again = run(e, sets, 1, 1, with_info=False)               # RC as the bound on a chain: more rounds, the same owners
            assert np.array_equal(again["owners"], res["owners"]) and np.array_equal(again["counts"], res["counts"])
            free(res); free(again)
        lens = sorted(np.bincount(wants[1][2][wants[1][2] >= 0]).tolist())
        assert len(set(lens)) == 3 and max(lens) > 150
    finally:
        e.close()


def test_owner_map_errors():
    """Parent maps that are no forest of the sets: a message, every word written, nothing out of range."""
    import pathfit
    from pathfit.engine import Engine, _View
    g = np.zeros((6, 7), np.uint8)
    e = Engine(g)
    try:
        off, ids = nc.csr([[29]])
        sound = np.full(g.size, 255, np.uint8)
        sound[30], sound[29] = 0, 8
        for name, (cell, code), msg in (("cycle", (10, 1), "chain"), ("code", (20, 9), "code outside"), ("edge", (3, 2), "code outside"),
                                        ("edge", (41, 3), "code outside"), ("wrap", (7, 0), "code outside"), ("root", (5, 8), "no source of its set")):
            par = sound.copy()
            par[cell] = code
            if name == "cycle":
                par[11] = 0                                           # 10's parent is 11, 11's parent is 10
            p, o = e.put(par), e.put(np.full(3 * g.size, CANARY, np.int32))
            with pytest.raises(pathfit.PathfitError, match=msg):
                e.dist_field_owners(off, ids, p, _View(e, o.at(g.size), g.size, np.int32))
            got = o.download()
            assert np.all(got[:g.size] == CANARY) and np.all(got[2 * g.size:] == CANARY) and not np.any(got[g.size:2 * g.size] == CANARY), name
            assert got[g.size + 29] == 0 and got[g.size + 30] == 0, name
            p.free(); o.free()
    finally:
        e.close()


# ---- 7. a bench-sized map
def test_bench_512_64_sources():
    import pathfit
    g = gio.upsample(gio.grid("g256")[0], 2)
    g = (g == 1).astype(np.uint8)
    R, C = g.shape
    free_cells = np.flatnonzero(g.reshape(-1) != 1)
    sources = nc.seeded_sets(g, [64], seed=95)[0]
    targets = np.random.default_rng(96).choice(free_cells, 2000, replace=False)
    mm = fc.move_masks(g, 1, 1)
    e = pathfit.Engine(g)
    try:
        res = run(e, [sources], 1, 1)
        (merged, code, own, count), = check(g, [sources], 1, 1, res, [want_of(g, mm, sources)])
        print(f"512^2, 64 sources: merged field {res['ms'][0]:.3f} ms, parents {res['ms'][1]:.3f} ms, owners {res['ms'][2]:.3f} ms, "
              f"{res['info'][0][0]} levels")
        free(res)
        pairs = [(int(t) // C, int(t) % C) for t in targets]
        n = pathfit.NearestSourceField(g, [[(s // C, s % C) for s in sources]], engine=e)
        d = pathfit.DistanceField(g, [(s // C, s % C) for s in sources], engine=e)
        sp = pathfit.score_params()
        fwd, back = n.paths(pairs), n.paths(pairs, reverse=True)
        assert np.array_equal(n.chosen, own.reshape(-1)[targets]) and np.array_equal(n.owners[0], own)
        assert np.array_equal(n.territory_sizes(0), count) and np.array_equal(n.fields[0], merged)
        label = merged.reshape(-1)[targets]
        assert np.isfinite(label).sum() > 1000
        step = {fc.DR[k] * C + fc.DC[k]: k for k in range(8)}
        for t, a, b, o in zip(targets, fwd, back, n.chosen):
            a, b = a.cells, b.cells
            assert np.array_equal(a[::-1], b)
            if o < 0:
                assert len(a) == 0
                continue
            assert a[0] == sources[o] and a[-1] == t
            ks = [step[int(v)] for v in np.diff(a)]
            assert all((mm.reshape(-1)[u] >> k) & 1 for u, k in zip(a[:-1], ks))
        assert np.array_equal(e.score_host([p.cells for p in fwd], sp)[:, 0], label)                     # pf_score_batch: bit for bit the label
        # the route that existed before: K = 64 fields and paths(k=None).  The same lengths, not always the same cells or sources
        old = d.paths(pairs)
        assert np.array_equal(e.score_host([p.cells for p in old], sp)[:, 0], label)
        assert np.array_equal(e.score_host([p.cells[::-1] for p in d.paths(pairs, reverse=True)], sp)[:, 0], label)
        assert np.array_equal(d.fields.reshape(64, -1).min(axis=0), merged.reshape(-1))
        assert [len(p) == 0 for p in old] == [len(p) == 0 for p in fwd]
        n.close(); d.close()
    finally:
        e.close()


# ---- 8. argument errors: found on the host, nothing launched
def test_argument_errors():
    import pathfit
    from pathfit.engine import Engine, _View
    g = (gio.grid("fig7")[0] == 1).astype(np.uint8)
    RC = g.size
    e = Engine(g)
    try:
        f = e.put(np.full((4, RC), float(CANARY)))
        o = e.put(np.full((4, RC), CANARY, np.int32))
        p = e.put(np.full((2, RC), 255, np.uint8))
        fv, ov = _View(e, f.at(RC), 2 * RC, np.float64), _View(e, o.at(RC), 2 * RC, np.int32)
        e.dist_field_merged([0, 1], [0], _View(e, f.at(RC), RC, np.float64))
        ms = e.last_kernel_ms()
        f.upload(np.full((4, RC), float(CANARY)))
        cases = [([0], [0], r"B = 0"), ([1, 2, 3], [0, 1, 2], r"set_off\[0\] = 1.*start at 0"), ([0, 2, 1], [0, 1], r"set 1: set_off\[2\] = 1 lies below"),
                 ([0, 1, 1], [0], r"set 1 is empty"), ([0, 0, 1], [0], r"set 0 is empty"), ([0, 2, 4], [0, 1, 2, RC], rf"set 1, source 1 \(index 3\) = {RC} lies outside"),
                 ([0, 2, 4], [0, -1, 2, 3], r"set 0, source 1 \(index 1\) = -1 lies outside")]
        for off, ids, msg in cases:
            with pytest.raises(pathfit.PathfitError, match="pf_dist_field_merged: .*" + msg):
                e.dist_field_merged(off, ids, fv)
            with pytest.raises(pathfit.PathfitError, match="pf_dist_field_owners: .*" + msg):
                e.dist_field_owners(off, ids, p, ov)
        a, b = (int(v) for v in np.flatnonzero(g.reshape(-1) != 1)[[0, -1]])
        off, ids = nc.csr([[a], [b]])
        po, pi = off.ctypes.data, ids.ctypes.data
        for args in ((None, pi, fv.ptr), (po, None, fv.ptr), (po, pi, None)):
            assert e.L.pf_dist_field_merged(e.h, 1, 1, 2, args[0], args[1], args[2], None) == -1
            assert "pf_dist_field_merged: bad arguments" in e.L.pf_last_error(e.h).decode()
        for args in ((None, po, pi, ov.ptr), (p.ptr, None, pi, ov.ptr), (p.ptr, po, None, ov.ptr), (p.ptr, po, pi, None)):
            assert e.L.pf_dist_field_owners(e.h, 2, args[0], args[1], args[2], None, args[3], None) == -1
            assert "pf_dist_field_owners: bad arguments" in e.L.pf_last_error(e.h).decode()
        assert e.L.pf_dist_field_merged(None, 1, 1, 2, po, pi, fv.ptr, None) == -2
        assert e.last_kernel_ms() == ms
        assert np.all(f.download() == CANARY) and np.all(o.download() == CANARY)
        e.dist_field_merged(off, ids, fv)                             # the handle still works
        got = f.download()
        assert np.all(got[0] == CANARY) and np.all(got[3] == CANARY) and got[1, a] == 0.0 and got[2, b] == 0.0 and (got[1:3] == 0.0).sum() == 2
    finally:
        e.close()


# ---- 9. NearestSourceField end to end, sharing an engine with a DijkstraSolver
def test_nearest_source_field_end_to_end():
    import pathfit
    g, s, t = gio.grid("fig13")
    R, C = g.shape
    z = gio.load("dijkstra_cases")
    gid = [str(v) for v in z["grid_names"]].index("fig13")
    mine = [int(i) for i in np.flatnonzero(~z["has_avoid"] & (z["grid_id"] == gid))]
    assert len(mine) == 10

    def goldens(sol):
        for start in sorted({int(z["start"][i]) for i in mine}):
            grp = [i for i in mine if int(z["start"][i]) == start]
            out = sol.solve_many([(int(z["target"][i]) // C, int(z["target"][i]) % C) for i in grp], (start // C, start % C))
            for i, r in zip(grp, out):
                assert [a * C + b for a, b in r[0]] == list(gio.csr_get(z["path_off"], z["path"], i)) and list(r[1:6]) == list(z["stats"][i]), i

    occ = (g == 1).astype(np.uint8)
    mm = fc.move_masks(occ, 1, 1)
    sets = nc.seeded_sets(occ, [5, 1], seed=97)
    sets[1] = [s]
    wants = [want_of(occ, mm, st) for st in sets]
    every = [(r, c) for r in range(R) for c in range(C)]
    e = pathfit.Engine(g)
    try:
        sol = pathfit.DijkstraSolver(g, engine=e)
        goldens(sol)
        n = pathfit.NearestSourceField(g, [[(v // C, v % C) for v in st] for st in sets], engine=e)
        flat = pathfit.NearestSourceField(g, [(v // C, v % C) for v in sets[0]], engine=e)      # one flat list of pairs: B = 1
        assert n.B == 2 and flat.B == 1 and np.array_equal(flat.fields[0], n.fields[0])
        for b, (merged, code, own, count) in enumerate(wants):
            assert np.array_equal(n.fields[b], merged) and np.array_equal(n.parents[b], code) and np.array_equal(n.owners[b], own)
            assert np.array_equal(n.territory_sizes(b), count) and n.territory_sizes(b).dtype == np.int64
            assert np.array_equal(n.reachable(b), np.isfinite(merged))
            got = n.paths(every, b=b)
            assert np.array_equal(n.chosen, own.reshape(-1)) and n.chosen.dtype == np.int32
            assert [p.cells.tolist() for p in got] == [fc.trace(code, v) for v in range(R * C)]
            assert [p.cells.tolist() for p in n.paths(every, b=b, reverse=True)] == [p.cells.tolist()[::-1] for p in got]
            for v in range(0, R * C, 7):
                o = int(own.reshape(-1)[v])
                assert n.nearest(b, every[v]) == ((o, float(merged.reshape(-1)[v])) if o >= 0 else (None, float("inf")))
                p = got[v].tolist()
                assert n.next_hop(b, every[v]) == (p[-2] if len(p) > 1 else None)
        long = max(n.paths(every, b=1), key=len)
        assert n.paths([long.tolist()[-1]], b=1, path_cap=len(long))[0] == long
        with pytest.raises(pathfit.PathfitError, match="more than path_cap"):
            n.paths([long.tolist()[-1]], b=1, path_cap=len(long) - 1)
        assert n.kernel_ms > 0 and n.parents_kernel_ms > 0 and n.owners_kernel_ms > 0
        assert n.buf.ptr and n.pbuf.ptr and n.obuf.ptr
        fresh = pathfit.NearestSourceField(g, [[(s // C, s % C)]], engine=e)     # closed before its lazy parts exist
        fresh.close()
        for use in (lambda: fresh.owners, lambda: fresh.parents, lambda: fresh.paths([(0, 0)]), lambda: fresh.nearest(0, (0, 0)),
                    lambda: fresh.territory_sizes(0), lambda: fresh.fields):
            with pytest.raises(pathfit.PathfitError, match="closed"):
                use()
        n.close()
        assert n.buf is None and n.pbuf is None and n.obuf is None and e.h
        with pytest.raises(pathfit.PathfitError, match="closed"):
            n.paths([(0, 0)])
        assert np.array_equal(n.owners[0], wants[0][2])               # what was downloaded stays readable
        assert np.array_equal(flat.owners[0], wants[0][2])            # another field on the same engine is untouched
        flat.close()
        goldens(sol)                                                  # the handle's slots and error word were shared safely
        own_engine = pathfit.NearestSourceField(g, [[(s // C, s % C)]])
        assert np.array_equal(own_engine.owners[0], wants[1][2])
        own_engine.close()
        assert own_engine.engine.h is None
    finally:
        e.close()
