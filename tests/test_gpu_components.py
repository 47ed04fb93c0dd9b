"""Connected components on the device (pf_components, pf_component_sizes, pf_components_same, pathfit.Components) against the model of
tests/component_checkers.py (an explicit-stack flood fill over field_checkers.move_masks, pinned by tests/test_component_checkers.py),
against the distance fields and against the A* kernels' own infeasibility proof.  Every comparison is exact equality; every output
buffer lies between canary words."""
import functools

import numpy as np
import pytest

import component_checkers as cc
import field_checkers as fc
import golden_io as gio
import thin_maps

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64                                                             # canary words in front of and behind every output


def run(e, ad, rs, want_info=True, want_sizes=True):
    """Raw Engine calls, every output between canaries -> dict(labels [R, C], info [4], sizes [count], first [count], count)."""
    from pathfit.engine import _View
    RC = e.R * e.C
    lb = e.put(np.full(RC + 2 * PAD, CANARY, np.int32))
    ib = e.put(np.full(4 + 2 * PAD, CANARY, np.int64))
    out = {}
    try:
        lv, iv = _View(e, lb.at(PAD), RC, np.int32), _View(e, ib.at(PAD), 4, np.int64)
        e.components(lv, ad, rs, iv if want_info else None)
        out["ms"] = e.last_kernel_ms()
        a = lb.download()
        assert np.all(a[:PAD] == CANARY) and np.all(a[-PAD:] == CANARY), "labels"
        out["labels"] = a[PAD:-PAD].reshape(e.R, e.C)
        a = ib.download()
        assert np.all(a[:PAD] == CANARY) and np.all(a[-PAD:] == CANARY), "info"
        out["info"] = a[PAD:-PAD]
        if not want_info:
            assert np.all(out["info"] == CANARY)
            out["info"] = None
        count = out["count"] = int(out["labels"].max()) + 1
        if want_sizes:
            sb = e.put(np.full(count + 2 * PAD, CANARY, np.int64))
            fb = e.put(np.full(count + 2 * PAD, CANARY, np.int32))
            try:
                e.component_sizes(lv, count, _View(e, sb.at(PAD), count, np.int64), _View(e, fb.at(PAD), count, np.int32))
                for name, b in (("sizes", sb), ("first", fb)):
                    a = b.download()
                    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), name
                    out[name] = a[PAD:len(a) - PAD]
            finally:
                sb.free()
                fb.free()
    finally:
        lb.free()
        ib.free()
    return out


def check(res, want, tag):
    lab, sizes, first = want
    assert np.array_equal(res["labels"], lab), tag
    if res["info"] is not None:
        assert np.array_equal(res["info"], cc.info_of(sizes)), (tag, res["info"], cc.info_of(sizes))
    if "sizes" in res:
        assert np.array_equal(res["sizes"], sizes) and np.array_equal(res["first"], first), tag


def check_map(g, policies=fc.POLICIES, wants=None):
    from pathfit.engine import Engine
    e = Engine(g)
    try:
        for i, (ad, rs) in enumerate(policies):
            check(run(e, ad, rs), wants[i] if wants else cc.flood_fill(g, ad, rs), (g.shape, ad, rs))
    finally:
        e.close()


# ---- 1. the golden maps, the four policies
@pytest.mark.parametrize("name", ["fig7", "fig13", "img1", "g128crop", "g256"])
def test_golden_maps(name):
    check_map(gio.grid(name)[0])


# ---- 2. thin and tiny maps
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_thin_maps(ad, rs):
    for R, C, ob in thin_maps.all_maps():
        check_map(thin_maps.thin_map(R, C, ob)[0], [(ad, rs)])


def test_all_obstacles_and_one_cell():
    from pathfit.engine import Engine
    e = Engine(np.ones((5, 7), np.uint8))
    try:
        for ad, rs in fc.POLICIES:
            res = run(e, ad, rs)
            assert res["count"] == 0 and np.all(res["labels"] == -1) and np.array_equal(res["info"], [0, 0, 0, -1])
            assert len(res["sizes"]) == 0 and len(res["first"]) == 0   # an empty sizes call: nothing written, nothing launched
            check(run(e, ad, rs, want_info=False), cc.flood_fill(np.ones((5, 7), np.uint8), ad, rs), "no info")
    finally:
        e.close()
    for v in (0, 2, 3):
        check_map(np.full((1, 1), v, np.uint8))
    check_map(np.ones((1, 1), np.uint8))


# ---- 3. 300 x 517 and the copies shifted by one free row and one free column
MAPS_300 = {
    "checkerboard": lambda: cc.checkerboard(300, 517),
    "row_serpentine": lambda: cc.row_serpentine(300, 517),
    "col_serpentine": lambda: cc.col_serpentine(300, 517),
    "rings": lambda: cc.rings(300, 517),
}
for _frac in (30, 41, 55):
    for _seed in (1, 2, 3):
        MAPS_300["random%d_s%d" % (_frac, _seed)] = functools.partial(cc.seeded_random, 300, 517, _frac / 100.0, 100 * _frac + _seed)


@pytest.mark.parametrize("name", list(MAPS_300))
def test_300x517_and_shifted(name):
    """155 100 cells.  The shipped (tiled) form labels tiles of 64 columns x 16 rows in LDS and links the tile borders in HBM:
    517 = 8 * 64 + 5 and 300 = 18 * 16 + 12, so 9 x 19 tiles, the last column of tiles 5 cells wide and the last row 12 high.  The
    global form (-DPF_CC_TILED=0) has no tile: a workgroup takes 256 consecutive cell ids.  The shifted copy (301 x 518) moves every
    structure by one cell against the tile borders, the 256-cell pieces and the scan's blocks."""
    g = MAPS_300[name]()
    assert g.shape == (300, 517)
    check_map(g)
    check_map(cc.shifted_copy(g))


# ---- 4. determinism: five runs on one handle
def test_five_runs_are_identical():
    from pathfit.engine import Engine
    g = cc.seeded_random(300, 517, 0.41, 4101)
    e = Engine(g)
    try:
        runs = [run(e, 1, 0) for _ in range(5)] + [run(e, 1, 1) for _ in range(5)]
        for group, pol in ((runs[:5], (1, 0)), (runs[5:], (1, 1))):
            check(group[0], cc.flood_fill(g, *pol), pol)
            for r in group[1:]:
                for key in ("labels", "info", "sizes", "first"):
                    assert np.array_equal(r[key], group[0][key]), (pol, key)
    finally:
        e.close()


# ---- 5. map changes on one handle, between searches
def test_update_grid_and_the_searches():
    from pathfit.engine import Engine
    from test_gpu_dist_field import sealed_rooms
    g = sealed_rooms()
    row = next(r for r in range(25, 58) if g[r, 29] != 1 and g[r, 31] != 1)
    a, b = row * 96 + 29, row * 96 + 31
    opened = g.copy()
    opened[row, 30] = 0
    e = Engine(g)
    try:
        for ad, rs in fc.POLICIES:
            _, st = e.astar_host(0, [a], [b], allow_diag=ad, restrict_corner=rs)
            assert st[0] == 1, (ad, rs)                                # (the search has built the handle's own labels by now)
            res = run(e, ad, rs)
            check(res, cc.flood_fill(g, ad, rs), ("sealed", ad, rs))
            assert res["labels"][row, 29] != res["labels"][row, 31] and res["labels"][row, 30] == -1
        e.update_grid(opened)
        for ad, rs in fc.POLICIES:
            res = run(e, ad, rs)
            check(res, cc.flood_fill(opened, ad, rs), ("opened", ad, rs))
            assert res["labels"][row, 29] == res["labels"][row, 30] == res["labels"][row, 31] >= 0
            paths, st = e.astar_host(0, [a], [b], allow_diag=ad, restrict_corner=rs)
            assert st[0] == 0 and list(paths[0]) == [a, a + 1, b], (ad, rs)
        e.update_grid(g)
        for ad, rs in fc.POLICIES:
            check(run(e, ad, rs), cc.flood_fill(g, ad, rs), ("sealed again", ad, rs))
            _, st = e.astar_host(0, [a], [b], allow_diag=ad, restrict_corner=rs)
            assert st[0] == 1, (ad, rs)
    finally:
        e.close()


# ---- 6. agreement with the distance fields and the A* kernels on g256, through the class
@pytest.mark.parametrize("ad, rs", fc.POLICIES)
def test_g256_against_fields_and_astar(ad, rs):
    import pathfit
    from pathfit.engine import Engine
    g = gio.grid("g256")[0]
    e = Engine(g)
    try:
        comp = pathfit.Components(g, bool(ad), bool(rs), engine=e)
        lab, sizes, first = cc.flood_fill(g, ad, rs)
        assert comp.count == len(sizes) and np.array_equal(comp.labels, lab) and np.array_equal(comp.sizes, sizes)
        assert comp.first_cells == [(int(v) // 256, int(v) % 256) for v in first]
        assert comp.largest == (int(np.argmax(sizes)), int(sizes.max())) and comp.free_cells == int((g != 1).sum())
        assert comp.kernel_ms > 0
        df = pathfit.DistanceField(g, comp.first_cells, bool(ad), bool(rs), engine=e)
        for k in range(comp.count):
            assert np.array_equal(df.reachable(k), comp.labels == k), k
            assert np.array_equal(comp.mask(k), lab == k)
        df.close()
        free = np.flatnonzero(g.reshape(-1) != 1)
        rnd = np.random.default_rng(256)
        flat = lab.reshape(-1)
        while True:                                                   # seeded pairs; at least 16 across components (the second region holds 603 cells)
            s, t = rnd.choice(free, 256), rnd.choice(free, 256)
            if int((flat[s] != flat[t]).sum()) >= 16:
                break
        differ = flat[s] != flat[t]
        same = comp.same([((int(x) // 256, int(x) % 256), (int(y) // 256, int(y) % 256)) for x, y in zip(s, t)])
        assert same.dtype == bool and np.array_equal(same, ~differ)
        assert np.array_equal(comp.label_of([(int(x) // 256, int(x) % 256) for x in s[:8]]), flat[s[:8]])
        for variant in (0, 2):
            _, st = e.astar_host(variant, s, t, allow_diag=bool(ad), restrict_corner=bool(rs))
            assert np.array_equal(st == 1, differ) and np.all((st == 0) | (st == 1)), variant
        comp.close()
    finally:
        e.close()


def test_class_refresh_and_close():
    import pathfit
    from test_gpu_dist_field import sealed_rooms
    g = sealed_rooms()
    row = next(r for r in range(25, 58) if g[r, 29] != 1 and g[r, 31] != 1)
    comp = pathfit.Components(g)
    before = comp.count
    want0 = cc.flood_fill(g, 1, 1)[0]
    assert np.array_equal(comp.label_of([(row, 29), (row, 31), (20, 30)]), want0[[row, row, 20], [29, 31, 30]])   # (before .labels is read)
    assert np.array_equal(comp.labels, want0)
    assert not comp.same([((row, 29), (row, 31))])[0]
    opened = g.copy()
    opened[row, 30] = 0
    comp.engine.update_grid(opened)
    assert comp.refresh() is comp and comp.count == before - 1
    want = cc.flood_fill(opened, 1, 1)
    assert np.array_equal(comp.labels, want[0]) and np.array_equal(comp.sizes, want[1])
    assert comp.same([((row, 29), (row, 31))])[0]
    comp.close()
    assert np.array_equal(comp.labels, want[0])                       # what was downloaded stays readable
    with pytest.raises(pathfit.PathfitError, match="Components: the labels are closed"):
        comp.same([((row, 29), (row, 31))])


# ---- 7. same
def test_same_pairs():
    from pathfit.engine import Engine, _View
    g = gio.grid("img1")[0]
    RC = g.size
    lab = cc.flood_fill(g, 1, 1)[0].reshape(-1)
    free0, free1, wall = int(np.flatnonzero(lab == 0)[0]), int(np.flatnonzero(lab == 1)[0]), int(np.flatnonzero(lab < 0)[0])
    wall2 = int(np.flatnonzero(lab < 0)[1])
    free0b = int(np.flatnonzero(lab == 0)[5])
    a = [free0, free0, free0, wall, wall, wall, -1, free0, RC, free0, free0, free1, -1, RC, 2 ** 31 - 1, -2 ** 31]
    b = [free0b, free1, wall, free0, wall2, wall, free0, -1, free0, RC, free0, free1, -1, RC, free0, free0]
    want = [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    rnd = np.random.default_rng(7)
    a = np.concatenate([a, rnd.integers(-3, RC + 3, 4096)]).astype(np.int32)
    b = np.concatenate([b, rnd.integers(-3, RC + 3, 4096)]).astype(np.int32)
    ok = (a >= 0) & (a < RC) & (b >= 0) & (b < RC)
    model = np.zeros(len(a), np.int32)
    model[ok] = (lab[a[ok]] >= 0) & (lab[a[ok]] == lab[b[ok]])
    assert list(model[:16]) == want and 100 < model.sum() < len(a) - 100
    e = Engine(g)
    try:
        dl = e.buf(RC, np.int32)
        e.components(dl, True, True)
        n = len(a)
        da, db = e.put(a), e.put(b)
        ds = e.put(np.full(n + 2 * PAD, CANARY, np.int32))
        e.components_same(dl, da, db, n, _View(e, ds.at(PAD), n, np.int32))
        got = ds.download()
        assert np.all(got[:PAD] == CANARY) and np.all(got[-PAD:] == CANARY)
        assert np.array_equal(got[PAD:-PAD], model)
        ds.upload(np.full(n + 2 * PAD, CANARY, np.int32))
        e.components_same(dl, da, db, 0, _View(e, ds.at(PAD), n, np.int32))   # n == 0: nothing is written
        assert np.all(ds.download() == CANARY)
        e.components_same(dl, da, db, 1, _View(e, ds.at(PAD), n, np.int32))
        got = ds.download()
        assert got[PAD] == 1 and np.all(np.delete(got, PAD) == CANARY)
        # labels outside [0, count) are ignored by the sizes call
        sb, fb = e.put(np.full(1 + 2 * PAD, CANARY, np.int64)), e.put(np.full(1 + 2 * PAD, CANARY, np.int32))
        e.component_sizes(dl, 1, _View(e, sb.at(PAD), 1, np.int64), _View(e, fb.at(PAD), 1, np.int32))
        assert np.array_equal(np.delete(sb.download(), PAD), np.full(2 * PAD, CANARY)) and sb.download()[PAD] == 281
        assert np.array_equal(np.delete(fb.download(), PAD), np.full(2 * PAD, CANARY)) and fb.download()[PAD] == free0
        e.component_sizes(dl, 2, None, None)
        for buf in (dl, da, db, ds, sb, fb):
            buf.free()
    finally:
        e.close()


def test_argument_errors():
    from pathfit.engine import Engine
    g = gio.grid("fig7")[0]
    e = Engine(g)
    try:
        L, h = e.L, e.h
        b = e.buf(g.size, np.int32)
        p = b.ptr

        def failed(rc, name):
            assert rc == -1 and L.pf_last_error(h).decode().startswith(name + ": bad arguments"), (rc, L.pf_last_error(h))
        failed(L.pf_components(h, 1, 1, None, None), "pf_components")
        failed(L.pf_component_sizes(h, None, 1, p, p), "pf_component_sizes")
        failed(L.pf_component_sizes(h, p, -1, p, p), "pf_component_sizes")
        failed(L.pf_components_same(h, None, 1, p, p, p), "pf_components_same")
        failed(L.pf_components_same(h, p, 1, None, p, p), "pf_components_same")
        failed(L.pf_components_same(h, p, 1, p, None, p), "pf_components_same")
        failed(L.pf_components_same(h, p, 1, p, p, None), "pf_components_same")
        failed(L.pf_components_same(h, p, -1, p, p, p), "pf_components_same")
        assert L.pf_components_same(h, p, 0, p, p, p) == 0 and L.pf_component_sizes(h, p, 0, None, None) == 0
        assert L.pf_components(None, 1, 1, p, None) < 0 and L.pf_component_sizes(None, p, 1, p, p) < 0
        assert L.pf_components_same(None, p, 1, p, p, p) < 0
        b.free()
    finally:
        e.close()


# ---- 8. large ids
def test_1024_squared():
    g = gio.upsample(gio.grid("g256")[0], 4)
    assert g.shape == (1024, 1024)
    want = cc.flood_fill(g, 1, 1)
    assert len(want[1]) == 10
    check_map(g, [(1, 1)], [want])


def test_4096_squared_split_wall():
    """16 777 216 cells (65 536 workgroups, cell ids up to 2^24): a full wall with one corner-cutting diagonal gap, the expected
    labels written with numpy.  The gap joins (1775, 2496) and (1776, 2495): 1776 is a multiple of 16 and 2496 of 64, so the one
    decisive diagonal crosses a corner of the 64 x 16 tiles and is linked in HBM, between ids near 7.3 million.  The labels are
    64 MiB per policy; one upload of the map and four downloads."""
    R = C = 4096
    w, gap = 2495, 1776
    assert gap % 16 == 0 and (w + 1) % 64 == 0
    g = cc.split_wall(R, C, w, gap)
    wants = [cc.split_wall_labels(R, C, w, gap, ad, rs) for ad, rs in fc.POLICIES]
    assert [len(x[1]) for x in wants] == [2, 1, 2, 2]
    check_map(g, fc.POLICIES, wants)
