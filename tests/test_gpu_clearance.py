"""Clearance fields on the device (pf_clearance_field, pf_clearance_paths, pf_clearance_segments, pathfit.Clearance) against the models
of tests/clearance_checkers.py (brute force over the obstacle list, pinned by tests/test_clearance_checkers.py).  Every comparison
is exact equality; every output buffer lies between canary words."""
import numpy as np
import pytest

import clearance_checkers as ck
import component_checkers as cc
import golden_io as gio
import thin_maps

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64                                                             # canary words in front of and behind every output
MODES = [(0, True, True), (1, True, True), (0, False, False), (1, False, True), (0, True, False)]   # (border, d_near, d_info)


def between_canaries(e, n, dtype):
    return e.put(np.full(n + 2 * PAD, CANARY, dtype))


def inner(buf, tag):
    a = buf.download()
    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), tag
    return a[PAD:len(a) - PAD]


def run_field(e, border, want_near=True, want_info=True):
    """One raw Engine call, every output between canaries -> (d2 [R, C], near [R, C] or None, info [4] or None)."""
    from pathfit.engine import _View
    RC = e.R * e.C
    db, nb, ib = between_canaries(e, RC, np.int32), between_canaries(e, RC, np.int32), between_canaries(e, 4, np.int64)
    try:
        e.clearance_field(_View(e, db.at(PAD), RC, np.int32), border, _View(e, nb.at(PAD), RC, np.int32) if want_near else None,
                          _View(e, ib.at(PAD), 4, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        d2, near, info = inner(db, "d2").reshape(e.R, e.C), inner(nb, "near").reshape(e.R, e.C), inner(ib, "info")
        if not want_near:
            assert np.all(near == CANARY)
        if not want_info:
            assert np.all(info == CANARY)
        return d2, near if want_near else None, info if want_info else None
    finally:
        for b in (db, nb, ib):
            b.free()


def check_engine(e, g, modes=MODES, wants=None, tag=None):
    wants = wants or {}
    for border, wn, wi in modes:
        if border not in wants:
            wants[border] = ck.brute_force(g, bool(border))
        d2, near, info = run_field(e, border, wn, wi)
        w = wants[border]
        assert np.array_equal(d2, w[0]), (tag, g.shape, border, "d2")
        assert near is None or np.array_equal(near, w[1]), (tag, g.shape, border, "near")
        assert info is None or np.array_equal(info, w[2]), (tag, g.shape, border, info, w[2])


def check_map(g, modes=MODES, tag=None):
    from pathfit.engine import Engine
    e = Engine(g)
    try:
        check_engine(e, g, modes, tag=tag)
    finally:
        e.close()


def check_maps_on_one_handle(maps, modes=MODES):
    """Maps of one shape through pf_update_grid on one handle."""
    from pathfit.engine import Engine
    e = Engine(maps[0])
    try:
        for i, g in enumerate(maps):
            if i:
                e.update_grid(g)
            check_engine(e, g, modes, tag=i)
    finally:
        e.close()


# ---- 1. the field against brute force
@pytest.mark.parametrize("name", ["fig7", "fig13", "img1", "g128crop", "g256"])
def test_golden_maps(name):
    check_map(gio.grid(name)[0])


@pytest.mark.parametrize("R, C", thin_maps.SHAPES)
def test_thin_maps(R, C):
    for ob in (False, True):
        if not ob or thin_maps.has_obstacle_version(R, C):
            check_map(thin_maps.thin_map(R, C, ob)[0])


def test_no_obstacle_all_obstacle_and_one_free_cell():
    g = np.zeros((7, 70), np.uint8)
    check_map(g)
    d2, near, info = ck.brute_force(g)
    assert np.all(d2 == ck.NONE) and np.all(near == -1) and list(info) == [0, 490, ck.NONE, 0]
    check_map(np.ones((7, 70), np.uint8))
    one = np.ones((7, 70), np.uint8)
    one[3, 66] = 0
    check_map(one)
    for v in (0, 1, 2, 3):
        check_map(np.full((1, 1), v, np.uint8))


def test_a_single_obstacle_on_every_cell_of_5x70():
    maps = []
    for v in range(5 * 70):
        g = np.zeros((5, 70), np.uint8)
        g.reshape(-1)[v] = 1
        maps.append(g)
    check_maps_on_one_handle(maps, [(0, True, True), (1, True, False)])


@pytest.mark.parametrize("C", [63, 64, 65, 127, 128, 129])
def test_widths_about_the_64_cell_words(C):
    maps = []
    for cols in ((0,), (C - 1,), (0, C - 1), (63,) if C > 64 else (C // 2,), (62, 64) if C > 65 else (1, C - 2)):
        g = np.zeros((5, C), np.uint8)
        for i, c in enumerate(cols):
            g[(2 + 2 * i) % 5, c] = 1
        maps.append(g)
        full = np.zeros((5, C), np.uint8)
        full[:, list(cols)] = 1
        maps.append(full)
    check_maps_on_one_handle(maps)


def test_tie_maps():
    check_maps_on_one_handle(ck.tie_maps(), [(0, True, True), (1, True, True)])


@pytest.mark.parametrize("name", ["one_per_row", "first_column_only"])
def test_envelope_stress(name):
    """Dominated parabolas: one obstacle per row at a seeded column (a column sees 200 parabolas, most of them hidden), and obstacles
    in column 0 only (in column c every parabola has the height c^2, and the open columns are far beyond the outward scan's reach)."""
    g = ck.one_per_row(200, 200, 41) if name == "one_per_row" else ck.first_column_only(200, 200, 9, 42)
    check_map(g, MODES[:2])


@pytest.mark.parametrize("name", ["one_per_row", "first_column_only", "last_rows"])
def test_envelope_stress_4096_wide(name):
    """The same two at 100 x 4096, and obstacles in the last two rows only at 300 x 4096: at this width the outward scan gives up
    after 64 rows (a narrow map is scanned all the way), so these columns are the envelope pass's."""
    if name == "last_rows":
        g = np.zeros((300, 4096), np.uint8)
        g[298:, :] = ck.seeded(2, 4096, 0.005, 43)
    else:
        g = ck.one_per_row(100, 4096, 44) if name == "one_per_row" else ck.first_column_only(100, 4096, 5, 45)
    check_map(g, MODES[:2])


@pytest.mark.parametrize("frac", [0.001, 0.05, 0.4])
def test_300x517_and_shifted(frac):
    g = ck.seeded(300, 517, frac, int(frac * 1000) + 7)
    check_map(g, MODES[:3])
    check_map(ck.shifted_copy(g), MODES[:2])


@pytest.mark.parametrize("R, C", [(1400, 1100), (1024, 1024)])
def test_large_maps_with_32_obstacles(R, C):
    """Clearances of hundreds of cells, beyond the outward scan's reach at these widths (about 250 rows): both column passes write
    parts of one field.  The brute force stays at R C x 32."""
    check_map(ck.few(R, C, 32, R + C), MODES[:2])


def test_five_runs_are_identical():
    from pathfit.engine import Engine
    g = ck.seeded(300, 517, 0.002, 4101)
    e = Engine(g)
    try:
        for border in (0, 1):
            runs = [run_field(e, border) for _ in range(5)]
            w = ck.brute_force(g, bool(border))
            for r in runs:
                assert all(np.array_equal(x, y) for x, y in zip(r, w)), border
    finally:
        e.close()


def test_update_grid_then_refresh():
    import pathfit
    from test_gpu_dist_field import sealed_rooms
    g = sealed_rooms()
    row = next(r for r in range(25, 58) if g[r, 29] != 1 and g[r, 31] != 1)
    assert g[row, 30] == 1
    cl = pathfit.Clearance(g, nearest=True)
    want = ck.brute_force(g)
    assert cl.d2[row, 30] == 0 and cl.nearest[row, 30] == row * 96 + 30
    assert np.array_equal(cl.d2, want[0]) and np.array_equal(cl.nearest, want[1]) and np.array_equal(cl.info, want[2])
    assert cl.kernel_ms > 0 and cl.most_open == ((int(want[2][3]) // 96, int(want[2][3]) % 96), int(want[2][2]))
    opened = g.copy()
    opened[row, 30] = 0
    cl.engine.update_grid(opened)
    assert np.array_equal(cl.d2, want[0])                             # (what was downloaded stays until refresh)
    assert cl.refresh() is cl
    want = ck.brute_force(opened)
    assert cl.d2[row, 30] == 1 and np.array_equal(cl.d2, want[0]) and np.array_equal(cl.nearest, want[1]) and np.array_equal(cl.info, want[2])
    assert np.array_equal(cl.inflated(margin_sq=1), opened)
    cl.close()
    with pytest.raises(pathfit.PathfitError, match="Clearance: the field is closed"):
        cl.refresh()


# ---- 2. inflation
def test_inflated_maps_and_their_components():
    import pathfit
    from pathfit.engine import Engine
    g = gio.grid("g256")[0]
    e = Engine(g)
    try:
        cl = pathfit.Clearance(g, engine=e)
        d2 = ck.brute_force(g)[0]
        same = cl.inflated(margin_sq=1)
        assert np.array_equal(same == 1, g == 1) and np.array_equal(same, g)
        for margin in (1.5, 3):
            fat = cl.inflated(margin=margin)
            assert np.array_equal(fat, ck.inflated(g, d2, ck.margin_sq(margin))) and (fat == 1).sum() > (g == 1).sum()
            comp = pathfit.Components(fat)
            lab, sizes, _ = cc.flood_fill(fat, 1, 1)
            assert np.array_equal(comp.labels, lab) and np.array_equal(comp.sizes, sizes)
            comp.close()
        cl.close()
        assert e.h                                                   # a passed engine stays open
    finally:
        e.close()


# ---- 3. path rows
def run_paths(e, dfield, cells, lens, cap, margin, want_profile=True, n=None):
    """-> (out [n, 4], status [n], profile [n, cap] or None), everything between canaries (the profile: between canary ROWS too,
    because words beyond a row's length stay untouched)."""
    from pathfit.engine import _View
    n = len(lens) if n is None else n
    dc, dl = e.put(np.ascontiguousarray(cells, np.int32).reshape(-1)), e.put(np.asarray(lens, np.int32))
    ob, sb, pb = between_canaries(e, 4 * len(lens), np.int32), between_canaries(e, len(lens), np.int32), between_canaries(e, len(lens) * cap, np.int32)
    try:
        e.clearance_paths(dfield, n, cap, dc, dl, margin, _View(e, ob.at(PAD), 4 * n, np.int32), _View(e, sb.at(PAD), n, np.int32),
                          _View(e, pb.at(PAD), n * cap, np.int32) if want_profile else None)
        out, st, prof = inner(ob, "out").reshape(-1, 4), inner(sb, "status"), inner(pb, "profile").reshape(-1, cap)
        if not want_profile:
            assert np.all(prof == CANARY)
        return out, st, prof if want_profile else None
    finally:
        for b in (dc, dl, ob, sb, pb):
            b.free()


def check_paths(e, dfield, d2, rows, cap, margin, want_profile=True):
    cells = np.full((len(rows), cap), 0, np.int32)
    lens = np.zeros(len(rows), np.int32)
    for i, r in enumerate(rows):
        k = min(len(r), cap)
        cells[i, :k] = r[:k]
        lens[i] = len(r)
    out, st, prof = run_paths(e, dfield, cells, lens, cap, margin, want_profile)
    for i, r in enumerate(rows):
        mst, mout, mprof = ck.path_row(d2, r, cap, margin)
        assert st[i] == mst and np.array_equal(out[i], mout), (i, len(r), margin, out[i], mout)
        if want_profile:
            want = np.full(cap, CANARY, np.int32)
            if mprof is not None:
                want[:len(mprof)] = mprof
            assert np.array_equal(prof[i], want), (i, len(r), margin)
    return out, st


@pytest.fixture(scope="module")
def g256_field():
    from pathfit.engine import Engine
    g = gio.grid("g256")[0]
    e = Engine(g)
    dfield = e.buf(g.size, np.int32)
    e.clearance_field(dfield)
    d2 = dfield.download().reshape(g.shape)
    assert np.array_equal(d2, ck.brute_force(g)[0])
    yield e, g, dfield, d2
    e.close()


def test_path_rows_against_the_model(g256_field):
    e, g, dfield, d2 = g256_field
    flat = d2.reshape(-1)
    rnd = np.random.default_rng(31)
    open_cells, wall = np.flatnonzero(flat >= 2), np.flatnonzero(flat == 0)
    cap = 129
    rows = [rnd.choice(open_cells, L).astype(np.int32) for L in (1, 63, 64, 65, 129, 129, 2, 128)]
    first, last, twice = (rnd.choice(open_cells, 100).astype(np.int32) for _ in range(3))
    first[0] = wall[3]                                                # the minimum at the first cell
    last[-1] = wall[5]                                                # ... at the last cell
    twice[17] = twice[80] = wall[9]                                   # ... attained twice: the first position wins
    edge = rnd.choice(open_cells, 129).astype(np.int32)
    edge[64] = wall[1]                                                # the first cell of a lane's second trip
    rows += [first, last, twice, edge, np.array([wall[0]], np.int32)]
    rows += [np.zeros(0, np.int32), rnd.choice(open_cells, cap + 1).astype(np.int32), np.array([5, -1, 7], np.int32),
             np.array([5, 6, g.size], np.int32), np.array([2 ** 31 - 1], np.int32), np.array([-2 ** 31, 4], np.int32)]
    for margin in (0, 1, 2, 9, ck.NONE):
        out, st = check_paths(e, dfield, d2, rows, cap, margin)
        assert list(st[-6:]) == [1] * 6 and np.all(st[:-6] == 0)
        assert out[8][1] == 0 and out[9][1] == 99 and out[10][1] == 17 and out[11][1] == 64
        if margin == 0:
            assert np.all(out[:, 2] == 0) and np.all(out[:, 3] == -1)  # nothing undercuts 0
    check_paths(e, dfield, d2, rows, cap, 3, want_profile=False)
    # n == 0 launches nothing; the first row alone leaves the others untouched
    out, st, _ = run_paths(e, dfield, np.zeros((2, 4), np.int32), [1, 1], 4, 1, n=0)
    assert np.all(out == CANARY) and np.all(st == CANARY)
    out, st, prof = run_paths(e, dfield, np.zeros((2, 4), np.int32), [1, 1], 4, 1, n=1)
    assert st[0] == 0 and st[1] == CANARY and np.all(out[1] == CANARY) and prof[0, 0] == flat[0] and np.all(prof.reshape(-1)[1:] == CANARY)


def test_solver_rows_where_they_lie_in_hbm(g256_field):
    """A* rows from pf_astar_batch's own buffers, through the class."""
    import pathfit
    e, g, dfield, d2 = g256_field
    rnd = np.random.default_rng(12)
    free = np.flatnonzero(g.reshape(-1) != 1)
    n, cap = 48, e.default_path_cap()
    s, t = rnd.choice(free, n).astype(np.int32), rnd.choice(free, n).astype(np.int32)
    ds, dt = e.put(s), e.put(t)
    dc, dl, dst = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
    e.astar_batch(0, ds, dt, n, cap, dc, dl, dst)
    cells, lens = dc.download().reshape(n, cap), dl.download()
    assert (dst.download() == 0).sum() >= 24
    cl = pathfit.Clearance(g, engine=e)
    for margin in (1.5, 3.0):
        out, st = cl.path_clearance_device(dc, dl, n, cap, margin=margin)
        host = cl.path_clearance([cells[i, :lens[i]] for i in range(n)], margin=margin)
        assert out.shape == (n, 4) and out.dtype == np.int32 and np.array_equal(out, host[0]) and np.array_equal(st, host[1])
        for i in range(n):
            mst, mout, _ = ck.path_row(d2, cells[i, :max(lens[i], 0)], cap, ck.margin_sq(margin))
            assert st[i] == mst and np.array_equal(out[i], mout), i
    assert cl.paths_kernel_ms > 0
    # the smoothed waypoints of the same rows: how close does each straight piece pass?
    sm_ = pathfit.PathSmoother(g, engine=e)
    ways = sm_.smooth([cells[i, :lens[i]] for i in range(n) if lens[i] > 1])
    pairs = [(w.tolist()[j], w.tolist()[j + 1]) for w in ways for j in range(len(w.tolist()) - 1)]
    assert len(pairs) >= 24
    for touched in (False, True):
        dmin, at = cl.segment_clearance(pairs, touched)
        for k, (a, b) in enumerate(pairs):
            wmin, wat = ck.segment(d2, a, b, touched)
            assert dmin[k] == wmin and at[k] == (wat // 256, wat % 256), (k, a, b, touched)
        if touched:
            assert np.all(dmin >= 1)                                  # the strict smoother lets no segment touch an obstacle
    cl.close()
    for b in (ds, dt, dc, dl, dst):
        b.free()


def test_maaco_walk_and_ga_decode_rows():
    import pathfit
    g, s0, t0 = gio.grid("fig13")
    d2 = ck.brute_force(g)[0]
    m = pathfit.MAACO(g, 96, 4, 1.0, 7.0, 0.1, 2.5, 1.0, 0.9, 0.2, 0.9, 0.5, 0.1, seed=4)
    e = m.engine
    try:
        cl = pathfit.Clearance(g, engine=e)
        assert np.array_equal(cl.d2, d2)

        def check(dc, dl, n, cap):
            cells, lens = dc.download().reshape(n, cap), dl.download()
            out, st = cl.path_clearance_device(dc, dl, n, cap, margin=1.8)
            for i in range(n):
                mst, mout, _ = ck.path_row(d2, cells[i, :max(lens[i], 0)], cap, 4)
                assert st[i] == mst and np.array_equal(out[i], mout), i
            return int((st == 0).sum())
        n = m.walk_iteration_dev(0)
        dc, dl = m.walk_bufs()[:2]
        assert check(dc, dl, n, m.path_cap) >= 20
        W, n = 2, 80
        free = np.flatnonzero(g.reshape(-1) != 1)
        wps = np.random.default_rng(9).choice(free, (n, W)).astype(np.int32)
        cap = e.default_path_cap(W)
        dw, dc, dl, dst = e.put(wps), e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
        e.decode_batch(n, W, s0, t0, cap, dc, dl, dst, d_wp_cells=dw)
        assert check(dc, dl, n, cap) >= 40
        cl.close()
    finally:
        e.close()


def test_decode_cases_the_scorer_and_the_profile():
    """The golden rows: d_out[2] at margin_sq(1.8) is the number of cells that pay a safety penalty at min_safe_distance 1.8, and the
    safety pf_score_batch returns equals the value recomputed from the downloaded profile."""
    from pathfit.engine import Engine, score_params
    z = gio.load("decode_cases")
    names = [str(s) for s in z["grid_names"]]
    assert ck.margin_sq(1.8) == 4
    for gid, gname in enumerate(names):
        ids = [i for i in range(len(z["kind"])) if int(z["grid_id"][i]) == gid and len(gio.csr_get(z["path_off"], z["path"], i))][:40]
        if not ids:
            continue
        g = gio.grid(gname)[0]
        rows = [gio.csr_get(z["path_off"], z["path"], i) for i in ids]
        cap = max(len(r) for r in rows)
        e = Engine(g)
        try:
            dfield = e.buf(g.size, np.int32)
            e.clearance_field(dfield)
            d2 = dfield.download().reshape(g.shape)
            out, st = check_paths(e, dfield, d2, rows, cap, 4)
            cells = np.zeros((len(rows), cap), np.int32)
            for i, r in enumerate(rows):
                cells[i, :len(r)] = r
            _, _, prof = run_paths(e, dfield, cells, [len(r) for r in rows], cap, 4)
            got = e.score_host(rows, score_params(0, True, 0.3, 0.8, 1.8, 100.0))
            for i, r in enumerate(rows):
                total, paid = 0.0, 0
                for x in prof[i, :len(r)]:
                    dist = float(np.sqrt(np.float64(x)))
                    if dist < 1.8:
                        total += pow(1.8 - dist, 2.0)
                        paid += 1
                assert out[i, 2] == paid and got[i, 2] == total / len(r), (gname, ids[i], got[i, 2], total / len(r))
        finally:
            e.close()


# ---- 4. segments
def run_segments(e, dfield, a, b, touched, want_at=True, n=None):
    from pathfit.engine import _View
    n = len(a) if n is None else n
    da, db = e.put(np.asarray(a, np.int32)), e.put(np.asarray(b, np.int32))
    mb, ab = between_canaries(e, len(a), np.int32), between_canaries(e, len(a), np.int32)
    try:
        e.clearance_segments(dfield, da, db, n, _View(e, mb.at(PAD), n, np.int32), _View(e, ab.at(PAD), n, np.int32) if want_at else None, touched)
        return inner(mb, "min"), inner(ab, "at")
    finally:
        for buf in (da, db, mb, ab):
            buf.free()


def field_of(g, border=False):
    from pathfit.engine import Engine
    e = Engine(g)
    dfield = e.buf(g.size, np.int32)
    e.clearance_field(dfield, border)
    return e, dfield, dfield.download().reshape(g.shape)


@pytest.mark.parametrize("touched", [False, True])
def test_every_ordered_pair_of_a_12x13_map(touched):
    g = ck.seeded(12, 13, 0.12, 1213)
    e, dfield, d2 = field_of(g)
    try:
        assert np.array_equal(d2, ck.brute_force(g)[0])
        RC = g.size
        a, b = (v.reshape(-1) for v in np.mgrid[0:RC, 0:RC])
        dmin, at = run_segments(e, dfield, a, b, touched)
        for k in range(RC * RC):
            want = ck.segment(d2, (int(a[k]) // 13, int(a[k]) % 13), (int(b[k]) // 13, int(b[k]) % 13), touched)
            assert (dmin[k], at[k]) == want, (a[k], b[k], touched)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["fig7", "g256"])
def test_4000_seeded_pairs(name):
    g = gio.grid(name)[0]
    R, C = g.shape
    e, dfield, d2 = field_of(g, name == "fig7")                       # (fig7: a field with the border in it)
    try:
        rnd = np.random.default_rng(R)
        a, b = rnd.integers(0, R * C, 4000), rnd.integers(0, R * C, 4000)
        near = rnd.random(4000) < 0.5                                 # half of them short: steep, shallow and diagonal pieces
        br = np.clip(a // C + rnd.integers(-9, 10, 4000), 0, R - 1)
        bc = np.clip(a % C + rnd.integers(-9, 10, 4000), 0, C - 1)
        b = np.where(near, br * C + bc, b)
        for touched in (False, True):
            dmin, at = run_segments(e, dfield, a, b, touched)
            for k in range(4000):
                want = ck.segment(d2, (int(a[k]) // C, int(a[k]) % C), (int(b[k]) // C, int(b[k]) % C), touched)
                assert (dmin[k], at[k]) == want, (a[k], b[k], touched)
        dmin, at = run_segments(e, dfield, a, b, False, want_at=False)
        assert np.all(at == CANARY)
        dmin, at = run_segments(e, dfield, a, b, False, n=0)
        assert np.all(dmin == CANARY) and np.all(at == CANARY)
    finally:
        e.close()


def test_corridors_same_cell_and_endpoints_beside_the_grid():
    for shape in ((1, 4096), (4096, 1), (3, 4096), (4096, 3)):
        g = np.zeros(shape, np.uint8)
        g.reshape(-1)[[g.size // 3, g.size - 7]] = 1
        e, dfield, d2 = field_of(g)
        try:
            RC, C = g.size, shape[1]
            last_row0 = C - 1 if shape[0] < shape[1] else RC - C     # the far end of the first corridor
            a = [0, last_row0, 0, RC - 1, 5, RC // 3, -1, 0, RC, 0, 2 ** 31 - 1, 7]
            b = [last_row0, 0, RC - 1, 0, 5, RC // 3, 0, -1, 0, RC, 0, -2 ** 31]
            for touched in (False, True):
                dmin, at = run_segments(e, dfield, a, b, touched)
                for k in range(len(a)):
                    ok = 0 <= a[k] < RC and 0 <= b[k] < RC
                    want = ck.segment(d2, (a[k] // C, a[k] % C), (b[k] // C, b[k] % C), touched) if ok else (ck.NONE, -1)
                    assert (dmin[k], at[k]) == want, (shape, k, touched)
                assert dmin[4] == d2.reshape(-1)[5] and at[4] == 5 and dmin[5] == 0 and at[5] == RC // 3
        finally:
            e.close()


def test_abi_errors():
    from pathfit.engine import Engine
    g = gio.grid("fig7")[0]
    e = Engine(g)
    try:
        L, h = e.L, e.h
        buf = e.buf(4 * g.size, np.int32)
        p = buf.ptr

        def failed(rc, name):
            assert rc == -1 and L.pf_last_error(h).decode().startswith(name + ": bad arguments"), (rc, L.pf_last_error(h))
        failed(L.pf_clearance_field(h, 0, None, p, p), "pf_clearance_field")
        for args in ((None, 1, 4, p, p, 1, p, p, p), (p, -1, 4, p, p, 1, p, p, p), (p, 1, 0, p, p, 1, p, p, p), (p, 1, 4, None, p, 1, p, p, p),
                     (p, 1, 4, p, None, 1, p, p, p), (p, 1, 4, p, p, -1, p, p, p), (p, 1, 4, p, p, 1, None, p, p), (p, 1, 4, p, p, 1, p, p, None)):
            failed(L.pf_clearance_paths(h, *args), "pf_clearance_paths")
        for args in ((None, 0, 1, p, p, p, p), (p, 0, -1, p, p, p, p), (p, 0, 1, None, p, p, p), (p, 0, 1, p, None, p, p), (p, 0, 1, p, p, None, p)):
            failed(L.pf_clearance_segments(h, *args), "pf_clearance_segments")
        assert L.pf_clearance_paths(h, p, 0, 4, p, p, 1, p, None, p) == 0 and L.pf_clearance_segments(h, p, 0, 0, p, p, p, None) == 0
        assert L.pf_clearance_field(None, 0, p, None, None) == -2 and L.pf_clearance_paths(None, p, 1, 4, p, p, 1, p, p, p) == -2
        assert L.pf_clearance_segments(None, p, 0, 1, p, p, p, p) == -2
        buf.free()
    finally:
        e.close()
