"""The placement search on the device (pf_place_improve, pathfit.Placement) against the numpy model of tests/place_checkers.py (pinned
by tests/test_place_checkers.py).  Every comparison is exact equality, doubles as 64-bit words; every output buffer lies between
canary words.  A workgroup of 1024 threads searches a start, 64 / P sites a wavefront (P the power of two >= p), a lane a slot,
eight demands a step: the sizes lie about the multiples of the wavefront, the workgroup and the step on each axis, take every P,
and reach each axis's limit."""
import functools

import numpy as np
import pytest

import golden_io as gio
import place_checkers as pc
from tour_checkers import bits

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64                                                             # canary words in front of and behind every output


def between_canaries(e, n, dtype, inside=None):
    a = np.full(n + 2 * PAD, CANARY, dtype)
    if inside is not None:
        a[PAD:PAD + n] = inside
    return e.put(a)


def inner(buf, tag):
    a = buf.download()
    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), tag
    return a[PAD:len(a) - PAD]


@pytest.fixture(scope="module")
def eng():
    from pathfit import Engine
    e = Engine(gio.grid("fig7")[0])
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _model(key, m, n, start, mode, fixed, limit):
    return pc.improve_numpy(np.frombuffer(key, np.float64).reshape(m, n), list(start), mode, fixed, limit)


def model(a, start, mode, fixed, limit):
    a = np.ascontiguousarray(a, np.float64)
    return _model(a.tobytes(), a.shape[0], a.shape[1], tuple(int(v) for v in start), mode, fixed, limit)


def words(row, owner, value, status, info):
    return [int(v) for v in row], [int(v) for v in owner], tuple(bits(float(x)) for x in value), int(status), tuple(int(v) for v in info)


def run(e, mats, rows, mode, fixed, shared, limit, want_owner=True, want_info=True):
    """One raw Engine call, every output between canaries -> (row [B, p], owner [B, n], value [B, 4], status [B], info [B, 4])."""
    from pathfit.engine import _View
    mats = np.ascontiguousarray(mats, np.float64)
    rows = np.ascontiguousarray(rows, np.int32)
    B, p = rows.shape
    m, n = mats.shape[-2:]
    assert mats.shape == ((m, n) if shared else (B, m, n))
    dm = e.put(mats.reshape(-1))
    rb = between_canaries(e, B * p, np.int32, rows.reshape(-1))
    ob, vb = between_canaries(e, B * n, np.int32), between_canaries(e, 4 * B, np.float64)
    sb, ib = between_canaries(e, B, np.int32), between_canaries(e, 4 * B, np.int64)
    try:
        e.place_improve(mode, m, n, p, fixed, B, shared, dm, limit, _View(e, rb.at(PAD), B * p, np.int32), _View(e, ob.at(PAD), B * n, np.int32) if want_owner else None,
                        _View(e, vb.at(PAD), 4 * B, np.float64), _View(e, sb.at(PAD), B, np.int32), _View(e, ib.at(PAD), 4 * B, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        owner, info = inner(ob, "owner").reshape(B, n), inner(ib, "info").reshape(B, 4)
        assert (want_owner or np.all(owner == CANARY)) and (want_info or np.all(info == CANARY))
        return inner(rb, "row").reshape(B, p), owner, inner(vb, "value").reshape(B, 4), inner(sb, "status"), info
    finally:
        for b in (dm, rb, ob, vb, sb, ib):
            b.free()


def check(e, mats, rows, mode, fixed=0, shared=False, limit=None, tag=None):
    mats = np.ascontiguousarray(mats, np.float64)
    rows = np.ascontiguousarray(rows, np.int32)
    B, p = rows.shape
    m = mats.shape[-2]
    limit = 16 * p if limit is None else limit
    row, owner, value, status, info = run(e, mats, rows, mode, fixed, shared, limit)
    for b in range(B):
        want = model(mats if shared else mats[b], rows[b], mode, fixed, limit)
        assert words(row[b], owner[b], value[b], status[b], info[b]) == words(*want), (tag, m, mats.shape[-1], p, mode, fixed, B, b)
        assert pc.valid_row(list(row[b]), m, p, fixed) and list(row[b, :fixed]) == list(rows[b, :fixed])
    return row, owner, value, status, info


def full_row(m, p, seed):
    return [int(v) for v in np.random.default_rng([seed, m, p]).permutation(m)[:p]]


def half_row(m, p, seed):
    row = full_row(m, p, seed)
    return [v if s % 2 == 0 else -1 for s, v in enumerate(row)]


# ---- 1. sizes
@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("m,n,p", [(1, 1, 1), (2, 1, 1), (2, 3, 2), (3, 2, 3), (5, 7, 2)])
def test_the_smallest_shapes(eng, m, n, p, mode):
    for kind in pc.KINDS:
        mats = [pc.matrix(kind, m, n, s) for s in range(4)]
        for rows in ([[-1] * p] * 4, [full_row(m, p, s) for s in range(4)], [half_row(m, p, s) for s in range(4)]):
            row, owner, value, status, info = check(eng, mats, rows, mode, tag=kind)
            assert np.all(status == 0) and np.all(info[:, 1] == info[:, 0] + 1)
            for b in range(4):
                assert pc.better_candidates(mats[b], list(row[b]), mode, 0) == []


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096])
def test_demands_about_the_wavefront_and_the_workgroup(eng, n):
    m, p = 20, 3
    for mode in pc.MODES:
        mats = [pc.matrix("euclid", m, n, 1), pc.matrix("holes", m, n, 2), pc.matrix("ints", m, n, 3)]
        rows = [[-1] * p, half_row(m, p, 1), full_row(m, p, 2)]
        row, owner, value, status, info = check(eng, mats, rows, mode, tag="n")
        assert np.all(status == 0) and info[0, 0] >= p and info[0, 3] == n and info[0, 2] == 0


@pytest.mark.parametrize("m", [15, 16, 17, 63, 64, 65, 1023, 1024])
def test_sites_about_the_wavefront_and_the_workgroup(eng, m):
    n, p = 70, 4
    limit = 16 * p if m < 1000 else 5
    for mode in pc.MODES:
        mats = [pc.matrix("euclid", m, n, 4), pc.matrix("tenths", m, n, 5)]
        rows = [[-1] * p, [m - 1, 0, -1, m - 2]]                      # (the last sites stand in a row)
        row, owner, value, status, info = check(eng, mats, rows, mode, limit=limit, tag="m")
        assert info[0, 0] >= 4 and (m > 1000 or np.all(status == 0))


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64])
def test_slots_about_the_wavefront(eng, p):
    m, n = 80, 100
    for mode in pc.MODES:
        a = pc.matrix("euclid", m, n, 6)
        rows = [[-1] * p, full_row(m, p, 3), half_row(m, p, 4)]
        row, owner, value, status, info = check(eng, a, rows, mode, shared=True, limit=min(16 * p, 80), tag="p")
        assert info[0, 0] >= (row[0] >= 0).sum() >= min(p, 33) and np.all(info[:, 2] == 0)      # (a row may end with empty slots: no addition changes the key)


@pytest.mark.parametrize("m,n,p,limit", [(1024, 257, 64, 1), (130, 4096, 64, 2), (1024, 4096, 3, 2)])
def test_each_axis_at_its_limit_under_a_cap(eng, m, n, p, limit):
    a = pc.matrix("euclid", m, n, 7)
    row, owner, value, status, info = check(eng, a, [full_row(m, p, 5)], limit % 2, shared=True, limit=limit, tag="limit")
    assert status[0] == 2 and info[0, :2].tolist() == [limit, limit + 1]


# ---- 2. rows and batches
@pytest.mark.parametrize("mode", pc.MODES)
def test_fixed_slots_and_m_equal_p(eng, mode):
    m, n, p = 12, 40, 4
    a = pc.matrix("euclid", m, n, 8)
    for fixed in (0, 1, p):
        rows = [full_row(m, p, s) for s in range(3)] + [full_row(m, p, 3)[:max(fixed, 1)] + [-1] * (p - max(fixed, 1))]
        row, owner, value, status, info = check(eng, a, rows, mode, fixed=fixed, shared=True, tag="fixed")
        assert np.all(status == 0)
        if fixed == p:
            assert np.array_equal(row[:3], np.array(rows[:3])) and info[:3, :2].tolist() == [[0, 1]] * 3 and [bits(x) for x in value[:3, 0]] == [bits(x) for x in value[:3, 2]]
    b = pc.matrix("euclid", 5, 9, 2)
    row, owner, value, status, info = check(eng, b, [[-1] * 5, [4, 3, 2, 1, 0], [2, -1, -1, 0, -1]], mode, shared=True, tag="m == p")
    assert info[1].tolist()[:2] == [0, 1] and list(row[1]) == [4, 3, 2, 1, 0]                # every site is in the row: no candidate at all


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_batch_sizes_at_12_40_3(eng, B, shared):
    m, n, p, mode = 12, 40, 3, B % 2
    rows = [([-1] * p, full_row(m, p, b), half_row(m, p, b))[b % 3] for b in range(B)]
    if shared:
        check(eng, pc.matrix("euclid", m, n, 9), rows, mode, shared=True, tag="batch")
    else:
        check(eng, [pc.matrix(pc.KINDS[b % 4], m, n, b) for b in range(B)], rows, mode, tag="batch")


def test_the_cap_on_the_moves(eng):
    m, n, p = 30, 90, 5
    a = pc.matrix("euclid", m, n, 10)
    for mode in pc.MODES:
        full = model(a, [-1] * p, mode, 0, 16 * p)
        moves = full[4][0]
        assert full[3] == 0 and moves >= p
        for limit in (0, 1, moves - 1, moves):
            row, owner, value, status, info = check(eng, a, [[-1] * p, full[0]], mode, shared=True, limit=limit, tag="cap")
            assert list(status) == [0 if limit == moves else 2, 0] and info[0, :2].tolist() == [limit, limit + 1] and info[1, :2].tolist() == [0, 1]
            assert limit or list(row[0]) == [-1] * p


def test_owner_null_info_null_and_five_identical_runs(eng):
    m, n, p = 40, 300, 6
    mats = [pc.matrix(kind, m, n, 11) for kind in pc.KINDS]
    rows = [[-1] * p, full_row(m, p, 1), half_row(m, p, 2), full_row(m, p, 3)]
    ref = check(eng, mats, rows, 1, tag="identical")
    for _ in range(5):
        again = run(eng, mats, rows, 1, 0, False, 16 * p)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, ref))
    bare = run(eng, mats, rows, 1, 0, False, 16 * p, want_owner=False, want_info=False)
    assert all(bare[x].tobytes() == ref[x].tobytes() for x in (0, 2, 3))


# ---- 3. what the matrices hold
@pytest.mark.parametrize("m,n,p", [(6, 9, 3), (70, 130, 5)])
def test_matrix_content(eng, m, n, p):
    base = pc.matrix("euclid", m, n, 12)
    dark_column = base.copy()
    dark_column[:, n // 2] = pc.INF
    rooms = np.full((m, n), pc.INF)                                   # three rooms: site i reaches the demands of room i % 3 only
    for i in range(m):
        rooms[i, i % 3::3] = base[i, i % 3::3]
    big = np.where(pc.matrix("ints", m, n, 5) == 1.0, pc.BIG, base)
    on_demand = base.copy()
    on_demand[np.arange(min(m, n)), np.arange(min(m, n))] = 0.0       # a site on a demand: zero entries
    on_demand[:, 0] = 0.0                                             # and a zero column
    mats = [pc.matrix("ints", m, n, 2), np.full((m, n), 2.75), pc.matrix("tenths", m, n, 2), dark_column, np.full((m, n), pc.INF), rooms, big, on_demand,
            np.zeros((m, n))]
    for mode in pc.MODES:
        for rows in ([[-1] * p] * len(mats), [half_row(m, p, b) for b in range(len(mats))]):
            row, owner, value, status, info = check(eng, mats, rows, mode, tag="content")
            assert np.all(status == 0)
            assert info[3, 2] == 1 and owner[3, n // 2] == -1 and info[4, 2] == n and np.all(owner[4] == -1) and info[4, 0] == 0
            assert info[5, 2] == 0 and len({int(v) % 3 for v in row[5] if v >= 0}) == 3
            assert np.isfinite(value[6]).all()
    assert list(run(eng, mats[4], [[-1] * p], 0, 0, True, 16 * p)[0][0]) == [-1] * p          # no addition changes the key: the slots stay empty


def test_two_rooms_get_a_site_each(eng):
    for mode in pc.MODES:
        row, owner, value, status, info = check(eng, pc.two_rooms(), [[-1, -1]], mode, shared=True, tag="rooms")
        assert info[0, 2:].tolist() == [0, 6] and min(row[0]) < 2 <= max(row[0])


# ---- 4. argument errors of the raw ABI
def test_argument_and_validation_errors_leave_every_output_untouched(eng):
    e, L = eng, eng.L
    m, n, p, B = 5, 6, 3, 3
    good = np.array([pc.matrix("euclid", m, n, b) for b in range(B)])
    rows = np.array([[0, -1, 3], [4, 2, -1], [1, 0, 2]], np.int32)
    held = np.full(B * p + 2 * PAD, CANARY, np.int32)
    held[PAD:PAD + B * p] = rows.reshape(-1)
    rb, ob, vb = e.put(held), between_canaries(e, B * n, np.int32), between_canaries(e, 4 * B, np.float64)
    sb, ib = between_canaries(e, B, np.int32), between_canaries(e, 4 * B, np.int64)
    dm = e.put(good.reshape(-1))
    sel, owner, value, status, info = rb.at(PAD), ob.at(PAD), vb.at(PAD), sb.at(PAD), ib.at(PAD)
    try:
        improve = L.pf_place_improve
        out = (sel, owner, value, status, info)
        assert improve(None, 0, m, n, p, 1, B, 0, dm.ptr, 9, *out) == -2
        for args, msg in [((2, m, n, p, 1, B, 0, dm.ptr, 9) + out, "mode = 2"), ((-1, m, n, p, 1, B, 0, dm.ptr, 9) + out, "mode = -1"),
                          ((0, 0, n, p, 1, B, 0, dm.ptr, 9) + out, "m = 0"), ((0, 1025, n, p, 1, B, 0, dm.ptr, 9) + out, "m = 1025"),
                          ((0, m, 0, p, 1, B, 0, dm.ptr, 9) + out, "n = 0"), ((0, m, 4097, p, 1, B, 0, dm.ptr, 9) + out, "n = 4097"),
                          ((0, m, n, 0, 0, B, 0, dm.ptr, 9) + out, "p = 0"), ((0, m, n, 6, 1, B, 0, dm.ptr, 9) + out, "p = 6"),
                          ((0, 100, n, 65, 1, B, 0, dm.ptr, 9) + out, "p = 65"), ((0, m, n, p, -1, B, 0, dm.ptr, 9) + out, "fixed = -1"),
                          ((0, m, n, p, 4, B, 0, dm.ptr, 9) + out, "fixed = 4"), ((0, m, n, p, 1, 0, 0, dm.ptr, 9) + out, "B = 0"),
                          ((0, m, n, p, 1, B, 2, dm.ptr, 9) + out, "shared = 2"), ((0, m, n, p, 1, B, -1, dm.ptr, 9) + out, "shared = -1"),
                          ((0, m, n, p, 1, B, 0, dm.ptr, -1) + out, "max_moves = -1"), ((0, m, n, p, 1, B, 0, dm.ptr, (1 << 20) + 1) + out, "max_moves = 1048577"),
                          ((0, m, n, p, 1, B, 0, None, 9) + out, "must not be null"), ((0, m, n, p, 1, B, 0, dm.ptr, 9, None, owner, value, status, info), "must not be null"),
                          ((0, m, n, p, 1, B, 0, dm.ptr, 9, sel, owner, None, status, info), "must not be null"),
                          ((0, m, n, p, 1, B, 0, dm.ptr, 9, sel, owner, value, None, info), "must not be null")]:
            assert improve(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode(), (msg, L.pf_last_error(e.h))
        # a NaN, a negative entry, -0.0 and 2^1010: the smallest (b, i, j) is named
        for x in (np.nan, -1.0, -0.0, 2.0 ** 1010, -pc.INF):
            bad = good.copy()
            bad[2, 1, 3], bad[1, 3, 4] = x, x
            assert pc.first_bad_entry(bad) == (1, 3, 4)
            dm.upload(bad.reshape(-1))
            assert improve(e.h, 1, m, n, p, 1, B, 0, dm.ptr, 9, *out) == -1 and "(b, i, j) = (1, 3, 4)" in L.pf_last_error(e.h).decode(), (x, L.pf_last_error(e.h))
            bad[1, 3, 4] = pc.BIG
            dm.upload(bad.reshape(-1))
            assert improve(e.h, 1, m, n, p, 1, B, 0, dm.ptr, 9, *out) == -1 and "(b, i, j) = (2, 1, 3)" in L.pf_last_error(e.h).decode(), (x, L.pf_last_error(e.h))
        dm.upload(good.reshape(-1))
        # a bad row: the smallest (b, slot) is named
        for change, fixed, at in [({(2, 2): 0}, 1, (2, 2)), ({(1, 1): 4, (2, 2): 0}, 1, (1, 1)), ({(1, 2): 5}, 1, (1, 2)), ({(0, 1): -2}, 1, (0, 1)),
                                  ({(1, 0): -1}, 1, (1, 0)), ({}, 2, (0, 1)), ({(0, 1): 3, (0, 2): 3}, 0, (0, 2))]:
            broken = rows.copy()
            for (b, s), v in change.items():
                broken[b, s] = v
            assert pc.first_bad_row(broken, m, p, fixed) == at
            held[PAD:PAD + B * p] = broken.reshape(-1)
            rb.upload(held)
            assert improve(e.h, 0, m, n, p, fixed, B, 0, dm.ptr, 9, *out) == -1
            assert f"(b, slot) = ({at[0]}, {at[1]})" in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
            assert np.array_equal(rb.download(), held)
        for b in (ob, vb, sb, ib):
            assert np.all(b.download() == CANARY)
        # the handle still works
        held[PAD:PAD + B * p] = rows.reshape(-1)
        rb.upload(held)
        assert improve(e.h, 1, m, n, p, 1, B, 0, dm.ptr, 9, *out) == 0
        want = model(good[0], rows[0], 1, 1, 9)
        assert bits(float(vb.download()[PAD])) == bits(want[2][0]) and list(rb.download()[PAD:PAD + p]) == want[0]
    finally:
        for b in (rb, ob, vb, sb, ib, dm):
            b.free()


# ---- 5. Placement end to end
def ids_of(g, cells):
    return [r * g.shape[1] + c for r, c in cells]


def against_the_model(t, g, fields, search):
    """The matrix against the gathered fields (float64 [m, R * C]); the row, sites, total, radius, unserved, owner, history and moves
    against the model; field()'s merged row and every paths() row."""
    want_m = np.ascontiguousarray(fields[:, ids_of(g, t.demands)])
    assert t.matrix.tobytes() == want_m.tobytes()
    want = pc.search(want_m, t.count, t.mode, keep=t.keep, max_moves=t.max_moves, **search)
    assert list(t.row) == want["row"] and t.sites == [v for v in want["row"] if v >= 0] and t.cells == [t.candidates[v] for v in t.sites]
    assert [bits(t.total), bits(t.radius), t.unserved, t.moves] == [bits(want["total"]), bits(want["radius"]), want["unserved"], want["moves"]]
    assert t.history == want["history"] and [tuple(bits(x) for x in k[1:]) for k in t.history] == [tuple(bits(x) for x in k[1:]) for k in want["history"]]
    assert [t.sites[o] if o >= 0 else -1 for o in t.owner] == want["owner"] and t.loads == [want["owner"].count(v) for v in t.sites]
    assert t.feasible == (t.unserved == 0) and sum(t.loads) == t.n - t.unserved
    got = t.placement_cost(t.sites)
    assert (bits(got.total), bits(got.radius), got.unserved) == (bits(t.total), bits(t.radius), t.unserved)
    return want


def field_and_paths(t, df, g):
    """field()'s merged row at every demand cell equals near as a word; every paths() row equals DistanceField.paths', cell for cell
    (df: a DistanceField over the candidate sites, in order)."""
    near = t.matrix[t.sites].min(0)
    nf = t.field()
    try:
        assert nf.fields.reshape(-1)[ids_of(g, t.demands)].tobytes() == near.tobytes()
    finally:
        nf.close()
    paths = t.paths()
    assert len(paths) == t.n
    served = [j for j in range(t.n) if t.owner[j] >= 0]
    assert [j for j in range(t.n) if paths[j] is not None] == served
    rows = df.paths([t.demands[j] for j in served], k=[t.sites[int(t.owner[j])] for j in served])
    for j, row in zip(served, rows):
        assert len(row) > 0 and np.array_equal(paths[j].cells, row.cells) and paths[j][0] == t.cells[int(t.owner[j])] and paths[j][-1] == t.demands[j]


@pytest.mark.parametrize("objective", ["sum", "max"])
def test_placement_on_the_map_every_free_cell_a_site_and_a_demand(objective):
    from pathfit import DistanceField, Engine, Placement
    g = gio.grid(pc.MAP_NAME)[0]
    cells = pc.map_cells(g)
    e = Engine(g)
    t = df = None
    try:
        t = Placement(g, cells, cells, pc.MAP_COUNT, objective=objective, engine=e, **pc.MAP_SEARCH)
        df = DistanceField(g, sources=cells, engine=e)
        against_the_model(t, g, df.fields.reshape(len(cells), -1), pc.MAP_SEARCH)
        assert t.feasible and t.kernel_ms > 0 and len(t.history) == 3 and len(t.sites) == pc.MAP_COUNT and t.history[0] >= t.history[-1]
        field_and_paths(t, df, g)
    finally:
        for o in (t, df):
            if o is not None:
                o.close()
        e.close()


def seeded_cells(g, count, seed):
    free = np.flatnonzero(np.asarray(g).reshape(-1) != 1)
    pick = np.random.default_rng(seed).choice(free, count, replace=False)
    return [(int(v) // g.shape[1], int(v) % g.shape[1]) for v in pick]


def test_placement_on_g256_with_200_sites_and_1000_demands():
    from pathfit import DistanceField, Engine, Placement
    g = gio.grid("g256")[0]
    sites, demands = seeded_cells(g, 200, 1), seeded_cells(g, 1000, 2)
    search = dict(starts=5, rounds=2, seed=9)
    e = Engine(g)
    t = df = None
    try:
        t = Placement(g, sites, demands, 8, objective="max", keep=[7, 3], engine=e, **search)
        df = DistanceField(g, sources=sites, engine=e)
        against_the_model(t, g, df.fields.reshape(200, -1), search)
        assert t.sites[:2] == [7, 3] and len(t.history) == 3 and t.kernel_ms > 0
        field_and_paths(t, df, g)
    finally:
        for o in (t, df):
            if o is not None:
                o.close()
        e.close()


def two_rooms_map():
    """Two rooms joined by two doors; candidate sites and demands in both."""
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    g[1, 10] = g[7, 10] = 0
    return g, [(4, 2), (0, 18), (8, 12), (4, 9), (1, 11), (7, 5)], [(8, 18), (8, 3), (2, 5), (6, 14), (0, 0), (4, 20), (1, 9), (7, 11)]


def test_fields_in_three_chunks(monkeypatch):
    from pathfit import DistanceField, Placement
    g, sites, demands = two_rooms_map()
    search = dict(starts=4, rounds=2, seed=0)
    whole = Placement(g, sites, demands, 2, **search)
    monkeypatch.setattr(Placement, "CHUNK_BYTES", 2 * 189 * 8)        # two rows of the 9 x 21 map at a time: chunks of 2, 2 and 2
    t = Placement(g, sites, demands, 2, engine=whole.engine, **search)
    df = DistanceField(g, sources=sites, engine=whole.engine)
    try:
        assert t.chunk == 2 and whole.chunk == 6
        assert t.matrix.tobytes() == whole.matrix.tobytes() and list(t.row) == list(whole.row) and t.history == whole.history
        against_the_model(t, g, df.fields.reshape(6, -1), search)
        for _ in range(2):                                           # a released chunk is computed again
            field_and_paths(t, df, g)
        assert [list(p.cells) for p in t.paths()] == [list(p.cells) for p in whole.paths()]
    finally:
        for o in (t, df, whole):
            o.close()


def test_a_demand_in_a_sealed_room_stays_unserved():
    from pathfit import DistanceField, Placement
    g, sites, demands = two_rooms_map()
    g[:, 15] = 1                                                      # a third room on the right: it holds demands, no site
    sites = [s for s in sites if s[1] < 15]
    demands = [d for d in demands if d[1] != 15]
    shut = [j for j, d in enumerate(demands) if d[1] > 15]
    search = dict(starts=3, rounds=1, seed=0)
    t = Placement(g, sites, demands, 2, **search)
    df = DistanceField(g, sources=sites, engine=t.engine)
    try:
        against_the_model(t, g, df.fields.reshape(len(sites), -1), search)
        assert shut and not t.feasible and t.unserved == len(shut) and all(t.owner[j] == -1 for j in shut) and np.isfinite(t.total)
        field_and_paths(t, df, g)
        assert all(t.paths()[j] is None for j in shut)
    finally:
        for o in (t, df):
            o.close()


def test_refresh_after_a_door_closes():
    from pathfit import DistanceField, Placement
    g, sites, demands = two_rooms_map()
    search = dict(starts=4, rounds=2, seed=1)
    t = Placement(g, sites, demands, 1, **search)
    try:
        first = list(t.sites)
        assert t.feasible
        g2 = g.copy()
        g2[1, 10] = g2[7, 10] = 1                                    # both doors shut: one site serves one room only
        t.engine.update_grid(g2)
        t.refresh()
        df = DistanceField(g2, sources=sites, engine=t.engine)
        try:
            against_the_model(t, g2, df.fields.reshape(6, -1), search)
            field_and_paths(t, df, g2)
        finally:
            df.close()
        assert not t.feasible and t.unserved > 0 and list(t.sites) != first      # the site moves to the room with more demands
    finally:
        t.close()


def test_cost_map_legs_on_g256():
    from pathfit import Clearance, CostField, Engine, Placement
    g = gio.grid("g256")[0]
    sites, demands = seeded_cells(g, 6, 3), seeded_cells(g, 12, 4)
    search = dict(starts=3, rounds=1, seed=2)
    e = Engine(g)
    t = cf = cl = None
    try:
        cl = Clearance(g, engine=e)
        cost = cl.cost_map(margin=4)
        t = Placement(g, sites, demands, 2, cost=cost, engine=e, **search)
        cf = CostField(g, cost, [[s] for s in sites], engine=e)
        against_the_model(t, g, cf.fields.reshape(6, -1), search)
        for j, leg in enumerate(t.paths()):
            if t.owner[j] < 0:
                assert leg is None
                continue
            assert len(leg) > 0 and np.array_equal(leg.cells, cf.paths([demands[j]], b=t.sites[int(t.owner[j])])[0].cells)
    finally:
        for o in (t, cf, cl):
            if o is not None:
                o.close()
        e.close()


def test_a_placement_fleet_tours_and_an_assignment_take_turns(eng):
    import assign_checkers as ac
    import fleet_checkers as fl
    from pathfit import Assignment, FleetTours, Placement
    g = gio.grid("fig7")[0]
    cells = pc.map_cells(g)
    p = Placement(g, cells[::7], cells[::3], 3, engine=eng, starts=3, rounds=1)
    f = FleetTours(g, fl.MAP_ROBOTS, fl.MAP_TASKS, engine=eng, **fl.MAP_SEARCH)
    a = Assignment(g, ac.GREEDY_ROBOTS, ac.GREEDY_TASKS, engine=eng)
    try:
        row, total, pp = list(p.row), p.total, [None if x is None else list(x.cells) for x in p.paths()]
        lf, pa = f.paths(), a.paths()
        f.refresh()
        assert [None if x is None else list(x.cells) for x in p.paths()] == pp
        p.refresh()
        a.refresh()
        assert list(p.row) == row and bits(p.total) == bits(total) and [None if x is None else list(x.cells) for x in p.paths()] == pp
        assert f.total == fl.MAP_ROUNDS_TOTAL and [list(x.cells) for x in f.paths()] == [list(x.cells) for x in lf]
        assert a.total == ac.GREEDY_OPTIMUM and [list(x.cells) for x in a.paths()] == [list(x.cells) for x in pa]
    finally:
        for o in (p, f, a):
            o.close()


def test_solve_matrices(eng):
    from pathfit import Placement
    mats = np.array([pc.matrix(kind, 10, 25, 2) for kind in ("ints", "euclid", "holes")])
    rows = [[3, -1, -1], [3, 9, 0], [3, -1, 5]]
    out = Placement.solve_matrices(eng, mats, rows, objective="max", fixed=1)
    for b in range(3):
        assert words(out.row[b], out.owner[b], out.value[b], out.status[b], out.info[b]) == words(*model(mats[b], rows[b], 1, 1, 48))
    out = Placement.solve_matrices(eng, mats[1], [[-1] * 4] * 2 + [[1, 2, 3, 4]], shared=True, max_moves=2)
    for b, row in enumerate([[-1] * 4] * 2 + [[1, 2, 3, 4]]):
        assert words(out.row[b], out.owner[b], out.value[b], out.status[b], out.info[b]) == words(*model(mats[1], row, 0, 0, 2))
