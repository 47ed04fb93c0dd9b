"""Widest-path fields on the device (pf_clearance_widest, pathfit.Clearance.widest / max_margin / widest_path / widest_paths) against the
model of tests/widest_checkers.py (a max-heap widest-path search, pinned by tests/test_widest_checkers.py against
threshold-then-flood-fill).  Every comparison is exact equality; every output lies between canary words; the fields come from
pf_clearance_field on the same handle."""
import numpy as np
import pytest

import component_checkers as cc
import golden_io as gio
import thin_maps
import widest_checkers as wc

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64
TW, TH = 64, 16                                                      # the kernel's tile (PF_WD_TW x PF_WD_TH)


def between_canaries(e, n, dtype):
    return e.put(np.full(n + 2 * PAD, CANARY, dtype))


def inner(buf, tag):
    a = buf.download()
    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), tag
    return a[PAD:len(a) - PAD]


class Field:
    """An engine on a map and its clearance field in HBM (`d2`: the downloaded copy)."""

    def __init__(self, g, border=False):
        from pathfit.engine import Engine
        self.g, self.e = np.asarray(g), Engine(g)
        self.dfield = self.e.buf(self.g.size, np.int32)
        self.field(border)

    def field(self, border):
        self.e.clearance_field(self.dfield, border)
        self.d2 = self.dfield.download().reshape(self.g.shape)
        return self

    def run(self, sets, ad, rs, want_info=True):
        """One raw call, both outputs between canaries -> (w [B, R, C], info [B, 4] or None)."""
        from pathfit.engine import _View
        e, B, RC = self.e, len(sets), self.g.size
        off, src = wc.csr(sets)
        wb, ib = between_canaries(e, B * RC, np.int32), between_canaries(e, 4 * B, np.int64)
        try:
            e.clearance_widest(self.dfield, off, src, _View(e, wb.at(PAD), B * RC, np.int32), ad, rs, _View(e, ib.at(PAD), 4 * B, np.int64) if want_info else None)
            assert e.last_kernel_ms() > 0
            work = e.clearance_widest_work()
            assert work[3] == 0 and work[0] <= work[1] and (work[0] > 0) == (work[1] > 0)
            w, info = inner(wb, "w").reshape((B,) + self.g.shape), inner(ib, "info").reshape(B, 4)
            if not want_info:
                assert np.all(info == CANARY)
            return w, info if want_info else None
        finally:
            wb.free()
            ib.free()

    def check(self, sets, policies=wc.POLICIES, tag=None, want_info=(True,)):
        for ad, rs in policies:
            want, winfo = wc.widest(self.d2, sets, ad, rs)
            for wi in want_info:
                w, info = self.run(sets, ad, rs, wi)
                assert np.array_equal(w, want), (tag, self.g.shape, ad, rs, "w", np.argwhere(w != want)[:4])
                assert info is None or np.array_equal(info, winfo), (tag, self.g.shape, ad, rs, info, winfo)

    def close(self):
        self.e.close()


def some_sources(d2, n, seed):
    """n seeded cells with d2 >= 1 (fewer when the map holds fewer)."""
    free = np.flatnonzero(d2.reshape(-1) >= 1)
    if len(free) == 0:
        return [0]
    return [int(v) for v in np.random.default_rng(seed).choice(free, min(n, len(free)), replace=False)]


def check_map(g, sets=None, borders=(False, True), policies=wc.POLICIES, want_info=(True,), tag=None):
    f = Field(g)
    try:
        for border in borders:
            f.field(border)
            f.check(sets if sets is not None else [[s] for s in some_sources(f.d2, 2, g.size)], policies, (tag, border), want_info)
    finally:
        f.close()


# ---- 1. golden and thin maps
@pytest.mark.parametrize("name", ["fig7", "fig13", "img1"])
def test_golden_20x20_maps(name):
    g, s, t = gio.grid(name)
    check_map(g, [[s], [t], [s, t]], want_info=(True, False))


@pytest.mark.parametrize("R, C", thin_maps.SHAPES)
def test_thin_maps(R, C):
    for ob in (False, True):
        if not ob or thin_maps.has_obstacle_version(R, C):
            g, s, t = thin_maps.thin_map(R, C, ob)
            check_map(g, [[s], [t, s]], want_info=(True, False), tag=ob)


# ---- 2. sizes about the tile
@pytest.mark.parametrize("C", [TW - 1, TW, TW + 1])
@pytest.mark.parametrize("R", [TH - 1, TH, TH + 1, 63, 64, 65])
def test_sizes_about_the_tile(R, C):
    g = wc.seeded(R, C, 0.12, 100 * R + C)
    for m in (g, wc.shifted_rows(g), wc.shifted_cols(g)):
        f = Field(m)
        try:
            src = some_sources(f.d2, 3, R + C)
            f.check([src[:1], src], [(1, 1), (0, 1)])
            f.field(True).check([src[:1]], [(1, 0)])
        finally:
            f.close()


# ---- 3. the corner rule across a tile corner
def test_a_diagonal_gap_across_a_tile_corner():
    r, c = 2 * TH, TW                                                 # the four cells about (r, c) lie in four tiles
    g = wc.corner_gap(4 * TH + 3, 2 * TW + 5, r, c)
    assert g[r - 1, c - 1] == 1 and g[r, c] == 1 and g[r - 1, c] == 0 and g[r, c - 1] == 0
    f = Field(g)
    try:
        left, right = (r + 5) * g.shape[1] + 3, 3 * g.shape[1] + c + 9
        rows = {}
        for ad, rs in wc.POLICIES:
            f.check([[left], [right]], [(ad, rs)])
            rows[ad, rs] = f.run([[left], [right]], ad, rs)[0]
        free, restricted = rows[1, 0], rows[1, 1]
        assert free[0].reshape(-1)[right] == 1 and free[1].reshape(-1)[left] == 1      # through the gap, at the capacity of its two cells
        assert restricted[0].reshape(-1)[right] == 0 and restricted[1].reshape(-1)[left] == 0
        assert not np.array_equal(free, restricted)
        assert np.array_equal(rows[0, 1], rows[0, 0]) and np.array_equal(rows[0, 1], restricted)   # nothing else joins the sides
    finally:
        f.close()


# ---- 4. plateaus, ladder, many rounds
def test_plateaus_crossing_several_tiles():
    g = wc.plateau_map(70, 200, 9)
    check_map(g, [[35 * 200 + 100], [3 * 200 + 3, 66 * 200 + 190]], policies=[(1, 1), (0, 0)])
    open_ = np.zeros((50, 150), np.uint8)                            # with the border every ring of equal d2 runs round the map
    open_[25, 75] = 1
    check_map(open_, [[0], [24 * 150 + 75]], policies=[(1, 1), (0, 1)])


def test_bottleneck_ladder():
    g, centres = wc.door_ladder(9, room=11, height=21)
    f = Field(g)
    try:
        f.check([[centres[-1]], [centres[0]], [centres[4]]])
        w = f.run([[centres[-1]]], 1, 1)[0][0].reshape(-1)
        assert [int(w[c]) for c in centres[:-1]] == [((j + 2) // 2) ** 2 for j in range(8)] and w[centres[-1]] == f.d2.reshape(-1)[centres[-1]]
    finally:
        f.close()


def test_serpentine_65x65():
    g = cc.row_serpentine(65, 65)
    check_map(g, [[0], [64 * 65 + 64, 32 * 65]], borders=(False,))
    check_map(cc.col_serpentine(65, 65), [[0]], borders=(True,), policies=[(1, 1), (0, 0)])


@pytest.mark.parametrize("frac", [0.03, 0.3])
def test_300x517(frac):
    g = wc.seeded(300, 517, frac, int(frac * 100) + 11)
    f = Field(g)
    try:
        src = some_sources(f.d2, 2, 517)
        f.check([src[:1]], [(1, 1)])
        f.check([src], [(0, 0)] if frac < 0.1 else [(1, 0)])
    finally:
        f.close()


# ---- 5. many sets in one call
def test_1_3_and_70_sets_in_one_call():
    from test_gpu_dist_field import sealed_rooms
    g = sealed_rooms()
    f = Field(g)
    try:
        flat = f.d2.reshape(-1)
        wall, free = np.flatnonzero(flat == 0), np.flatnonzero(flat >= 1)
        inside = next(r * 96 + c for r in range(35, 45) for c in range(45, 55) if flat[r * 96 + c] >= 1)   # in the sealed room
        rnd = np.random.default_rng(70)
        sets = [[int(free[0])], [int(wall[0])], [int(free[7]), int(free[7])], [int(wall[1]), int(wall[2])], [inside], [int(wall[3]), int(free[9]), int(free[9])]]
        sets += [[int(v) for v in rnd.choice(free, int(rnd.integers(1, 5)))] for _ in range(64)]
        assert len(sets) == 70
        f.check(sets[:1], [(1, 1)])
        f.check(sets[1:4], [(1, 1), (0, 1)])
        f.check(sets, [(1, 1)], want_info=(True, False))
        f.check(sets[:12], [(1, 0), (0, 0)])
        w, info = f.run(sets[:6], 1, 1)
        assert not w[1].any() and list(info[1]) == [0, 0, -1, -1] and info[2][0] == 1 and list(info[3]) == [0, 0, -1, -1] and info[5][0] == 1
        room = np.zeros((96, 96), bool)
        room[21:61, 31:71] = True
        assert w[4][room].any() and not w[4][~room].any() and not w[0][room].any()   # a sealed room keeps its source in and the others out
    finally:
        f.close()


@pytest.mark.parametrize("border", [False, True])
def test_a_map_without_obstacles(border):
    g = np.zeros((33, 130), np.uint8)
    f = Field(g, border)
    try:
        f.check([[0], [16 * 130 + 65, 5]], [(1, 1), (0, 0)], want_info=(True, False))
        w, info = f.run([[16 * 130 + 65]], 1, 1)
        if border:
            assert w.max() == 17 ** 2 and w.min() == 1 and np.array_equal(w[0], np.minimum(f.d2, 17 ** 2))
        else:
            assert np.all(w == wc.NONE) and list(info[0]) == [1, g.size, wc.NONE, 0]
    finally:
        f.close()


# ---- 6. determinism, map change
def test_five_runs_are_identical():
    g = wc.seeded(130, 260, 0.2, 5)
    f = Field(g)
    try:
        sets = [[s] for s in some_sources(f.d2, 3, 6)]
        want = wc.widest(f.d2, sets, 1, 1)
        runs = [f.run(sets, 1, 1) for _ in range(5)]
        for w, info in runs:
            assert np.array_equal(w, want[0]) and np.array_equal(info, want[1])
    finally:
        f.close()


def test_a_door_opened_by_update_grid():
    import pathfit
    from test_gpu_dist_field import sealed_rooms
    g = sealed_rooms()
    row = next(r for r in range(25, 58) if g[r, 29] != 1 and g[r, 31] != 1)
    inside, outside = (row, 40), (row, 10)
    cl = pathfit.Clearance(g)
    try:
        assert cl.d2[inside] >= 1 and cl.d2[outside] >= 1
        f = cl.widest(inside)
        assert f.w[0][outside] == 0 and np.array_equal(f.w[0], wc.widest_one(cl.d2, [inside[0] * 96 + inside[1]], 1, 1)[0]) and f.kernel_ms > 0
        assert cl.max_margin(inside, outside) == (0, 0.0)
        f.close()
        opened = g.copy()
        opened[row, 30] = 0
        cl.engine.update_grid(opened)
        cl.refresh()
        f = cl.widest(inside)
        want, n = wc.widest_one(cl.d2, [inside[0] * 96 + inside[1]], 1, 1)
        assert np.array_equal(f.w[0], want) and f.w[0][outside] == 1 and np.array_equal(f.info[0], wc.info_of(want, n))
        assert cl.max_margin(inside, outside) == (1, 1.0)
        f.close()
    finally:
        cl.close()


# ---- 7. the equivalent form, on the device through the existing classes
def test_thresholds_against_components_on_g256():
    import pathfit
    g = gio.grid("g256")[0]
    cl = pathfit.Clearance(g)
    try:
        free = np.argwhere(cl.d2 >= 9)
        s = tuple(int(x) for x in free[len(free) // 2])
        f = cl.widest(s)
        w = f.w[0]
        cells = [(r, c) for r in range(256) for c in range(256)]
        top = int(w.max())
        assert top == cl.d2[s]
        for t in sorted(set([1, 2, 4, 5, 8, 9, top, top + 1])):
            comp = pathfit.Components(cl.inflated(margin_sq=t))
            same = np.asarray(comp.same([(s, c) for c in cells]), bool).reshape(256, 256)
            comp.close()
            assert np.array_equal(w >= t, same), t
        f.close()
    finally:
        cl.close()


# ---- 8. routes
@pytest.mark.parametrize("name", ["fig7", "doors40"])
def test_routes_against_the_model(name):
    import pathfit
    g = gio.grid("fig7")[0] if name == "fig7" else wc.doors_map(40)
    R, C = g.shape
    cl = pathfit.Clearance(g)
    try:
        d2 = cl.d2
        free = np.flatnonzero(d2.reshape(-1) >= 1)
        rnd = np.random.default_rng(R)
        for ad, rs in wc.POLICIES:
            s = int(rnd.choice(free))
            w = wc.widest_one(d2, [s], ad, rs)[0]
            targets = [int(v) for v in rnd.choice(R * C, 12, replace=False)] + [s, int(np.flatnonzero(d2.reshape(-1) == 0)[0])]
            sc, tcs = (s // C, s % C), [(t // C, t % C) for t in targets]
            paths, ws = cl.widest_paths(sc, tcs, ad, rs)
            assert np.array_equal(ws, w.reshape(-1)[targets])
            for t, p, x in zip(targets, paths, ws):
                want, wt = wc.widest_path(g, d2, s, t, ad, rs, w)
                assert p.cells.tolist() == want and x == wt, (name, ad, rs, s, t)
            reached = [(p, x) for p, x in zip(paths, ws) if x > 0]
            out, st = cl.path_clearance([p for p, _ in reached], margin_sq=1)
            assert np.all(st == 0) and np.array_equal(out[:, 0], [x for _, x in reached])   # the smallest d2 on each route is its w
            for t, tc in list(zip(targets, tcs))[:4] + list(zip(targets, tcs))[-2:]:
                wt = int(w.reshape(-1)[t])
                assert cl.max_margin(sc, tc, ad, rs) == (wt, float(np.sqrt(wt)))
                p, x = cl.widest_path(sc, tc, ad, rs)
                want = wc.widest_path(g, d2, s, t, ad, rs, w)
                assert (list(p.cells) if x else p, x) == want
                if x:
                    assert cl.path_clearance([p], margin_sq=1)[0][0, 0] == x
    finally:
        cl.close()


# ---- 9. argument errors of the raw ABI
def test_abi_errors_launch_nothing():
    g = gio.grid("fig7")[0]
    f = Field(g)
    try:
        e, L, h = f.e, f.e.L, f.e.h
        RC = g.size
        wb, ib = between_canaries(e, 2 * RC, np.int32), between_canaries(e, 8, np.int64)
        pw, pi, pd = wb.at(PAD), ib.at(PAD), f.dfield.ptr

        def arr(*v):
            return np.array(v, np.int32)

        def failed(B, off, src, msg, d2=pd, out=pw):
            rc = L.pf_clearance_widest(h, 1, 1, d2, B, off.ctypes.data if off is not None else None, src.ctypes.data if src is not None else None, out, pi)
            err = L.pf_last_error(h).decode()
            assert rc == -1 and err.startswith("pf_clearance_widest: ") and msg in err, (rc, err)
            assert np.all(inner(wb, "w") == CANARY) and np.all(inner(ib, "info") == CANARY), msg
        failed(0, arr(0), arr(5), "B = 0")
        failed(-3, arr(0), arr(5), "B = -3")
        failed(1, None, arr(5), "must not be null")
        failed(1, arr(0, 1), None, "must not be null")
        failed(1, arr(1, 2), arr(5, 6), "set_off[0] = 1")
        failed(2, arr(0, 2, 1), arr(5, 6), "set 1: set_off[2] = 1 lies below set_off[1] = 2")
        failed(2, arr(0, 1, 1), arr(5, 6), "set 1 is empty")
        failed(2, arr(0, 1, 3), arr(5, 6, RC), f"set 1, source 1 (index 2) = {RC} lies outside the grid")
        failed(1, arr(0, 1), arr(-1), "set 0, source 0 (index 0) = -1 lies outside the grid")
        failed(1, arr(0, 1), arr(5), "must not be null", d2=None)
        failed(1, arr(0, 1), arr(5), "must not be null", out=None)
        assert L.pf_clearance_widest(None, 1, 1, pd, 1, arr(0, 1).ctypes.data, arr(5).ctypes.data, pw, pi) == -2
        assert L.pf_clearance_widest_work(None, None) == -2 and L.pf_clearance_widest_work(h, None) == -1
        off, src = arr(0, 1, 2), arr(5, 6)                            # ... and the same buffers take a good call
        assert L.pf_clearance_widest(h, 1, 1, pd, 2, off.ctypes.data, src.ctypes.data, pw, pi) == 0
        assert np.array_equal(inner(wb, "w").reshape(2, 20, 20), wc.widest(f.d2, [[5], [6]], 1, 1)[0])
        wb.free()
        ib.free()
    finally:
        f.close()
