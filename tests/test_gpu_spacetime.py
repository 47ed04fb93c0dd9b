"""Space-time fields on the device (pf_spacetime_stamp / _field / _paths / _conflicts, pathfit.SpaceTime) against the model of
tests/spacetime_checkers.py (pinned by tests/test_spacetime_checkers.py).  Every comparison is exact equality; every output lies
between canary words; arrive, every word of the reach planes and the info words are all compared."""
import functools

import numpy as np
import pytest

import golden_io as gio
import spacetime_checkers as sc

pytestmark = pytest.mark.gpu

CANARY = -77
CAN64 = np.uint64(0xB3B3B3B3B3B3B3B3)
PAD = 64
POLICIES = sc.POLICIES
MAPS20 = ("fig7", "fig13", "img1", "img2", "img3")


def between_canaries(e, n, dtype):
    return e.put(np.full(n + 2 * PAD, CAN64 if np.dtype(dtype) == np.uint64 else CANARY, dtype))


def inner(buf, tag):
    a = buf.download()
    can = CAN64 if a.dtype == np.uint64 else CANARY
    assert np.all(a[:PAD] == can) and np.all(a[len(a) - PAD:] == can), tag
    return a[PAD:len(a) - PAD]


def view(e, buf, n):
    from pathfit.engine import _View
    return _View(e, buf.at(PAD), n, buf.dtype)


def csr(sets):
    off = np.cumsum([0] + [len(s) for s in sets]).astype(np.int32)
    return off, np.array([v for s in sets for v in s], np.int32)


def run_field(e, occ, T, sets, ad, rs, want_reach=True, want_info=True):
    """One raw call -> (arrive int32 [B, R, C], reach uint64 [B, T + 1, R, Wc] or None, info int64 [B, 4] or None)."""
    B, RC, Wc = len(sets), e.R * e.C, (e.C + 63) // 64
    nr = B * (T + 1) * e.R * Wc
    ab, rb, ib = between_canaries(e, B * RC, np.int32), between_canaries(e, nr, np.uint64), between_canaries(e, 4 * B, np.int64)
    try:
        off, src = csr(sets)
        e.spacetime_field(T, occ, off, src, view(e, ab, B * RC), bool(ad), bool(rs), view(e, rb, nr) if want_reach else None,
                          view(e, ib, 4 * B) if want_info else None)
        assert e.last_kernel_ms() > 0
        a, r, i = inner(ab, "arrive").reshape(B, e.R, e.C), inner(rb, "reach").reshape(B, T + 1, e.R, Wc), inner(ib, "info").reshape(B, 4)
        if not want_reach:
            assert np.all(r == CAN64)
        if not want_info:
            assert np.all(i == CANARY)
        return a, r if want_reach else None, i if want_info else None
    finally:
        for b in (ab, rb, ib):
            b.free()


def check_field(e, S, D, sets, ad, rs, tag=None, occ=None):
    """The device against the word model, set by set: arrive, every reach word, info.  -> (arrive, reach words)"""
    T = D.shape[0] - 1
    Dw = sc.pack(D)
    own = occ is None
    occ = e.put(Dw) if own else occ
    try:
        a, r, info = run_field(e, occ, T, sets, ad, rs)
    finally:
        if own:
            occ.free()
    for b, s in enumerate(sets):
        wa, wr = sc.field_words(S, Dw, s, ad, rs)
        assert np.array_equal(a[b], wa), (tag, S.shape, T, ad, rs, b)
        assert np.array_equal(r[b], wr), (tag, S.shape, T, ad, rs, b)
        assert list(info[b]) == list(sc.info_of(wa)), (tag, S.shape, T, ad, rs, b, info[b])
    return a, r


def patrols(shape, T, n, seed, free=None):
    """n seeded obstacles: random king walks with waits, alternating after_end kinds, seeded start ticks and corner stamping."""
    R, C = shape
    rnd = np.random.default_rng(seed)
    D = np.zeros((T + 1, R, C), bool)
    for i in range(n):
        v = int(rnd.integers(0, R * C)) if free is None else int(rnd.choice(free))
        row = [v]
        for _ in range(int(rnd.integers(1, T + 2))):
            k = int(rnd.integers(-1, 8))
            r, c = v // C + (0 if k < 0 else sc.DR[k]), v % C + (0 if k < 0 else sc.DC[k])
            if 0 <= r < R and 0 <= c < C:
                v = r * C + c
            row.append(v)
        sc.planes(shape, T, [row], [int(rnd.integers(0, T // 2 + 1))], "stay" if i % 2 else "vanish", bool(i % 3 == 0), into=D)
    return D


def seeded(R, C, p, seed):
    return np.random.default_rng(seed).random((R, C)) < p


def engine(S):
    from pathfit.engine import Engine
    return Engine(np.asarray(S, np.uint8))


# ---- 1. the field against the model
def pocket(col):
    S = np.zeros((2, 9), bool)
    S[1, :] = True
    S[1, col] = False
    return S, sc.planes((2, 9), 24, [list(range(8, -1, -1))], None, "vanish")[0]


@pytest.mark.parametrize("col", [3, 4])
def test_pocket_maps(col):
    S, D = pocket(col)
    e = engine(S)
    try:
        for ad, rs in POLICIES:
            a, _ = check_field(e, S, D, [[0]], ad, rs, "pocket")
            if col == 3:
                assert (a[0, 0, 8], a[0, 1, 3]) == ((9, 3) if (ad, rs) == (1, 0) else (11, 4))
            else:
                assert a[0, 0, 8] == (8 if (ad, rs) == (1, 0) else -1)
    finally:
        e.close()


@pytest.mark.parametrize("name", MAPS20)
def test_golden_maps_with_patrols(name):
    g, s, t = gio.grid(name)
    S = g == 1
    free = np.flatnonzero(~S.reshape(-1))
    e = engine(S)
    try:
        for n in (0, 1, 5):
            D = patrols((20, 20), 50, n, 20 + n, free)
            for ad, rs in POLICIES:
                check_field(e, S, D, [[s], [t, s]], ad, rs, (name, n))
    finally:
        e.close()


@pytest.mark.parametrize("side", [1, 2, 3])
def test_thin_maps(side):
    # 4096 x 1 (4096 words, more than fit LDS: the HBM form, four words a thread) and 1 x 4096 walked end to end
    for R, C, T in ((side, 4096, 4100 if side == 1 else 70), (4096, side, 90), (side, 200, 260)):
        S = seeded(R, C, 0.0 if side == 1 else 0.1, R + C)
        S[0, 0] = False
        D = patrols((R, C), T, 3, R * 7 + C)
        D[:, 0, :2] = False
        e = engine(S)
        try:
            if T > 1000:
                a, _ = check_field(e, S, D, [[0]], 1, 1, "thin")
            else:
                for ad, rs in POLICIES:
                    a, _ = check_field(e, S, D, [[0], [R * C - 1, (R * C) // 2]], ad, rs, "thin")
            assert (a[0] >= 0).sum() > 1
        finally:
            e.close()


@pytest.mark.parametrize("C", [63, 64, 65, 127, 128, 129])
def test_word_borders(C):
    for R in (3, 8, 17):
        S = seeded(R, C, 0.2, R * C)
        S[:, 60:68] = False                                           # room to move across the border of words 0 and 1
        T = 40
        # an obstacle and a source on each side of a word border, an obstacle that walks across it both ways
        rows = [[R // 2 * C + 63], [R // 2 * C + min(64, C - 1)], [C + c for c in range(58, min(70, C))], [2 * C + c for c in range(min(69, C - 1), 57, -1)]]
        D = sc.planes((R, C), T, rows, [0, 3, 2, 1], "vanish", corners=True)[0] | patrols((R, C), T, 2, C + R)
        e = engine(S)
        try:
            for ad, rs in POLICIES:
                check_field(e, S, D, [[62], [min(64, C - 1)], [C + 63, 2 * C + 60]], ad, rs, "border")
        finally:
            e.close()
        if R == 8 and C + 3 <= 129:                                   # a shifted copy gives the shifted field
            S2, D2 = np.zeros((R, C + 3), bool), np.zeros((T + 1, R, C + 3), bool)
            S2[:, :3] = True
            S2[:, 3:], D2[:, :, 3:] = S, D
            e = engine(S2)
            try:
                a2, _ = check_field(e, S2, D2, [[62 // C * (C + 3) + 62 % C + 3]], 1, 1, "shifted")
                assert np.array_equal(a2[0][:, 3:], sc.field_words(S, sc.pack(D), [62], 1, 1, False)[0])
            finally:
                e.close()


def test_horizons():
    S = seeded(9, 70, 0.2, 5)
    S[0, 0] = False
    far = int(sc.field_words(S, sc.pack(np.zeros((701, 9, 70), bool)), [0], 1, 1, False)[0].max())
    assert far > 10
    e = engine(S)
    try:
        for T in (0, 1, far, far - 1):
            a, _ = check_field(e, S, np.zeros((T + 1, 9, 70), bool), [[0]], 1, 1, "T")
            assert a.max() == min(T, far)
    finally:
        e.close()


def test_source_sets():
    S = seeded(12, 30, 0.2, 3)
    S[5, 5] = S[0, 0] = False
    S[8:11, 20:23] = False
    S[7, 19:24] = S[11, 19:24] = True                                 # a sealed room round (8..10, 20..22)
    S[7:12, 19] = S[7:12, 23] = True
    T = 45
    D = patrols((12, 30), T, 3, 8)
    D[0, 5, 5] = True
    rnd = np.random.default_rng(4)
    e = engine(S)
    try:
        special = [[5 * 30 + 5], [0, 0, 0], [int(v) for v in np.flatnonzero(S.reshape(-1))[:3]], [9 * 30 + 21], []]
        a, _ = check_field(e, S, D, special, 1, 1, "special")
        assert (a[0] == -1).all() and (a[2] == -1).all() and (a[4] == -1).all() and (a[3] >= 0).sum() <= 9
        for B in (1, 3, 70):
            check_field(e, S, D, [[int(v) for v in rnd.integers(0, 360, 1 + b % 3)] for b in range(B)], 1, B % 2, "B")
        occ = e.put(sc.pack(D))
        a, r, i = run_field(e, occ, T, [[0]], 1, 1, want_reach=False, want_info=False)   # the optional outputs
        occ.free()
        assert r is None and i is None and np.array_equal(a[0], sc.field_words(S, sc.pack(D), [0], 1, 1, False)[0])
    finally:
        e.close()
    S = seeded(6, 7, 0.15, 1)                                         # 300 sets on a tiny map: more than one per CU, workgroups loop
    e = engine(S)
    try:
        check_field(e, S, patrols((6, 7), 20, 2, 2), [[b % 42, (5 * b) % 42] for b in range(300)], 1, 1, "300")
    finally:
        e.close()


# One map for each form the kernel has.  The live planes lie in LDS while 3 * R * ceil(C / 64) * 8 bytes fit 60 KiB (2560 words),
# else in HBM; a workgroup has min(1024, words rounded up to 64) threads, so a thread owns one word up to 1024 words and several
# beyond.  40 x 70: LDS, 128 threads.  256 x 256: LDS, 1024 threads, one word each.  300 x 500: LDS, 2400 words, three a thread.
# 1024 x 1100: HBM, 18432 words, 18 a thread (two sets: two scratch slots).
@pytest.mark.parametrize("R,C,T", [(40, 70, 60), (256, 256, 80), (300, 500, 60), (1024, 1100, 40)])
def test_every_form_of_the_kernel(R, C, T):
    S = seeded(R, C, 0.2, R)
    S[0, 0] = S[R - 1, C - 1] = False
    D = patrols((R, C), T, 5, C)
    e = engine(S)
    try:
        a, _ = check_field(e, S, D, [[0], [R * C - 1, R // 2 * C + C // 2]], 1, 1, "form")
        assert (a >= 0).sum() > 100
    finally:
        e.close()


def test_five_runs_are_identical_and_a_door_opens():
    S = seeded(30, 90, 0.25, 9)
    S[:, 40] = True                                                   # a wall with a door at (15, 40), shut at first
    S[0, 0] = False
    T = 150
    D = patrols((30, 90), T, 4, 1)
    e = engine(S)
    occ = e.put(sc.pack(D))
    try:
        runs = [run_field(e, occ, T, [[0]], 1, 1) for _ in range(5)]
        for a, r, i in runs[1:]:
            assert np.array_equal(a, runs[0][0]) and np.array_equal(r, runs[0][1]) and np.array_equal(i, runs[0][2])
        a0, _ = check_field(e, S, D, [[0]], 1, 1, "shut", occ)
        assert (a0[0][:, 41:] == -1).all()
        S2 = S.copy()
        S2[15, 39:42] = False
        e.update_grid(S2.astype(np.uint8))
        a1, _ = check_field(e, S2, D, [[0]], 1, 1, "open", occ)
        assert (a1[0][:, 41:] >= 0).any()
    finally:
        occ.free()
        e.close()


def test_zero_planes_against_the_static_fields():
    import pathfit
    S = seeded(14, 20, 0.3, 11)
    S[0, 0] = False
    T = 14 * 20
    D = np.zeros((T + 1, 14, 20), bool)
    e = engine(S)
    try:
        for ad, rs in POLICIES:
            a, _ = check_field(e, S, D, [[0], [279, 5]], ad, rs, "static")
            comp = pathfit.Components(S.astype(np.uint8), bool(ad), bool(rs), engine=e)
            lab = comp.labels
            for b, srcs in enumerate(([0], [279, 5])):
                want = np.zeros((14, 20), bool)
                for s in srcs:
                    if not S.reshape(-1)[s]:
                        want |= lab == lab.reshape(-1)[s]
                assert np.array_equal(a[b] >= 0, want), (ad, rs, b)
            comp.close()
            if not ad:
                out = e.buf((2, 280), np.float64)
                e.dist_field_merged([0, 1, 3], [0, 279, 5], out, False, bool(rs))
                d = out.download().reshape(2, 14, 20)
                out.free()
                assert np.array_equal(np.where(np.isfinite(d), d, -1.0), a.astype(np.float64))
    finally:
        e.close()


def test_parked_obstacle_against_a_closed_cell():
    S = seeded(10, 66, 0.2, 2)
    S[0, 0] = S[4, 64] = False
    T = 120
    D = sc.planes((10, 66), T, [[4 * 66 + 64]], None, "stay")[0]
    e = engine(S)
    try:
        got = {p: check_field(e, S, D, [[0]], *p, "parked")[0] for p in POLICIES}
        S2 = S.copy()
        S2[4, 64] = True
        e.update_grid(S2.astype(np.uint8))
        for p in POLICIES:
            assert np.array_equal(check_field(e, S2, np.zeros_like(D), [[0]], *p, "closed")[0], got[p])
    finally:
        e.close()


# ---- 2. the stamp
def run_stamp(e, T, occ_words, rows, t0, after_end, corners, clear, cap=None, lens=None):
    """-> (the planes uint64 [T + 1, R, Wc] after the call, status)"""
    Wc = (e.C + 63) // 64
    n = len(rows)
    cap = cap or max(max((len(r) for r in rows), default=1), 1)
    cells = np.full((n, cap), 10 ** 9, np.int32)                      # (words beyond a row's length must never be read as cells)
    for i, r in enumerate(rows):
        cells[i, :min(len(r), cap)] = r[:cap]
    lens = np.array([len(r) for r in rows], np.int32) if lens is None else np.asarray(lens, np.int32)
    nw = (T + 1) * e.R * Wc
    ob = e.put(np.concatenate([np.full(PAD, CAN64), occ_words.reshape(-1), np.full(PAD, CAN64)]).astype(np.uint64))
    sb = between_canaries(e, n, np.int32)
    bufs = [e.put(cells), e.put(lens), e.put(np.asarray(t0, np.int32)) if t0 is not None else None]
    try:
        e.spacetime_stamp(T, view(e, ob, nw), n, cap, bufs[0], bufs[1], view(e, sb, n), bufs[2], after_end, corners, clear)
        return inner(ob, "planes").reshape(T + 1, e.R, Wc), inner(sb, "status")
    finally:
        for b in [ob, sb] + [b for b in bufs if b is not None]:
            b.free()


def test_stamp_against_the_model():
    R, C, T = 9, 70, 30
    e = engine(np.zeros((R, C), bool))
    rnd = np.random.default_rng(6)
    try:
        rows = [[int(v) for v in rnd.integers(0, R * C, int(rnd.integers(1, 50)))] for _ in range(12)]      # jumps, rows past T
        diag = [r * C + 60 + r for r in range(8)] + [7 * C + 66 - r for r in range(5)]                        # unit diagonals across a word border
        rows += [diag, diag, diag[::-1], [5], [5]]                                                          # duplicates and overlaps
        t0 = [int(v) for v in rnd.integers(0, T + 1, len(rows))]
        base = sc.pack(patrols((R, C), T, 2, 3))
        for after_end in (True, False):
            for corners in (False, True):
                for clear in (False, True):
                    got, st = run_stamp(e, T, base, rows, t0, after_end, corners, clear)
                    want, wst = sc.planes((R, C), T, rows, t0, "stay" if after_end else "vanish", corners)
                    assert np.array_equal(got, sc.pack(want) | (0 if clear else base)), (after_end, corners, clear)
                    assert np.array_equal(st, wst) and not st.any()
        got, st = run_stamp(e, T, base, rows, None, True, True, False)                                      # d_t0 NULL: all 0
        assert np.array_equal(got, sc.pack(sc.planes((R, C), T, rows, None, "stay", True)[0]) | base)
        # every kind of bad row between good ones: empty, too long, a cell below 0 and beyond R C, t0 below 0 and beyond T
        rows = [[3, 4], [], [7] * 9, [5, -1, 6], [5, R * C], [8, 9], [10, 11], [12]]
        lens = [2, 0, 9, 3, 2, 2, 2, 1]
        t0 = [0, 0, 0, 0, 0, -1, T + 1, T]
        got, st = run_stamp(e, T, base, rows, t0, True, True, False, cap=8, lens=lens)
        assert list(st) == [0, 1, 1, 1, 1, 1, 1, 0]
        assert np.array_equal(got, sc.pack(sc.planes((R, C), T, [[3, 4], [12]], [0, T], "stay", True)[0]) | base)
    finally:
        e.close()


def test_stamp_astar_rows_where_the_solver_left_them():
    g, s, t = gio.grid("fig7")
    S = g == 1
    T = 45
    e = engine(S)
    try:
        free = np.flatnonzero(~S.reshape(-1))
        rnd = np.random.default_rng(12)
        n, cap = 6, e.default_path_cap()
        ds, dt = e.put(rnd.choice(free, n).astype(np.int32)), e.put(rnd.choice(free, n).astype(np.int32))
        dc, dl, dst = e.buf((n, cap), np.int32), e.buf(n, np.int32), e.buf(n, np.int32)
        e.astar_batch(0, ds, dt, n, cap, dc, dl, dst)
        cells, lens = dc.download().reshape(n, cap), dl.download()
        rows = [cells[i, :lens[i]].tolist() for i in range(n)]
        assert all(len(r) > 1 for r in rows)
        occ, st = e.buf((T + 1) * 20, np.uint64), e.buf(n, np.int32)
        e.spacetime_stamp(T, occ, n, cap, dc, dl, st, None, True, True, True)
        assert e.last_kernel_ms() > 0 and not st.download().any()
        want = sc.planes((20, 20), T, rows, None, "stay", True)[0]
        assert np.array_equal(occ.download().reshape(T + 1, 20, 1), sc.pack(want))
    finally:
        e.close()


# ---- 3. routes and conflicts
def run_paths(e, T, occ, B, reach, queries, cap, ad, rs, ticks=True):
    """queries: (set, target, tick) -> (rows as lists, len, status, ticks used); the rows lie between canary rows and a row's words
    beyond its length stay canaries."""
    n = len(queries)
    q = np.array(queries, np.int32).reshape(n, 3)
    cb, lb, sb, tb = (between_canaries(e, m, np.int32) for m in (n * cap, n, n, n))
    bufs = [e.put(q[:, 0].copy()), e.put(q[:, 1].copy()), e.put(q[:, 2].copy())]
    try:
        e.spacetime_paths(T, occ, B, reach, n, bufs[0], bufs[1], cap, view(e, cb, n * cap), view(e, lb, n), view(e, sb, n), bufs[2] if ticks else None,
                          view(e, tb, n), bool(ad), bool(rs))
        cells, lens, st, tk = inner(cb, "cells").reshape(n, cap), inner(lb, "len"), inner(sb, "status"), inner(tb, "ticks")
        for i in range(n):
            assert 0 <= lens[i] <= cap and np.all(cells[i, lens[i]:] == CANARY), i
            assert (st[i] == 0) == (lens[i] > 0)
        return [cells[i, :lens[i]].tolist() for i in range(n)], lens, st, tk
    finally:
        for b in [cb, lb, sb, tb] + bufs:
            b.free()


def run_conflicts(e, T, occ, rows, t0, hold, ad, rs, cap=None, lens=None):
    n = len(rows)
    cap = cap or max(max((len(r) for r in rows), default=1), 1)
    cells = np.full((n, cap), 10 ** 9, np.int32)
    for i, r in enumerate(rows):
        cells[i, :min(len(r), cap)] = r[:cap]
    lens = np.array([len(r) for r in rows], np.int32) if lens is None else np.asarray(lens, np.int32)
    ob, sb = between_canaries(e, 4 * n, np.int32), between_canaries(e, n, np.int32)
    bufs = [e.put(cells), e.put(lens), e.put(np.asarray(t0, np.int32)) if t0 is not None else None]
    try:
        e.spacetime_conflicts(T, occ, n, cap, bufs[0], bufs[1], view(e, ob, 4 * n), view(e, sb, n), bufs[2], hold, bool(ad), bool(rs))
        return inner(ob, "out").reshape(n, 4), inner(sb, "status")
    finally:
        for b in [ob, sb] + [b for b in bufs if b is not None]:
            b.free()


@pytest.mark.parametrize("ad,rs", POLICIES)
def test_paths_against_the_model_and_the_conflict_check(ad, rs):
    g, s, t = gio.grid("fig13")
    S = g == 1
    T = 60
    D = patrols((20, 20), T, 6, 31, np.flatnonzero(~S.reshape(-1)))
    D[:, s // 20, s % 20] = False                                     # (the start stays clear)
    Dw = sc.pack(D)
    sets = [[s], [t, 21]]
    e = engine(S)
    occ = e.put(Dw)
    reach = e.buf((2, T + 1, 20), np.uint64)
    da = e.buf((2, 400), np.int32)
    try:
        e.spacetime_field(T, occ, *csr(sets), da, bool(ad), bool(rs), reach)
        arrive = da.download().reshape(2, 400)
        model = [sc.unpack(sc.field_words(S, Dw, x, ad, rs)[1], 20) for x in sets]
        rnd = np.random.default_rng(5)
        queries = []
        for b in (0, 1):
            for v in rnd.integers(0, 400, 40):
                a = int(arrive[b, v])
                queries += [(b, int(v), -1), (b, int(v), -2), (b, int(v), min(a + 3, T) if a >= 0 else 7)]
        queries += [(2, 5, -1), (-1, 5, -1), (0, 400, -1), (0, -1, -1), (0, s, T + 1), (0, s, -3), (0, s, 0), (0, s, T)]
        rows, lens, st, tk = run_paths(e, T, occ, 2, reach, queries, T + 1, ad, rs)
        ok_rows, holds = [], []
        for i, (b, v, tick) in enumerate(queries):
            want, wst, wtk = sc.route(S, D, model[b], v, tick, ad, rs) if 0 <= b < 2 else (None, sc.ST_INFEASIBLE, -1)
            assert (st[i], tk[i]) == (wst, wtk) and rows[i] == (want or []), (i, queries[i])
            if want:
                ok_rows.append(want)
                holds.append(tick == -2)
        assert len(ok_rows) > 60 and any(holds) and st[-2] == 0 and (st[-8:-2] == 1).all()
        for hold in (False, True):                                    # every traced row is free of conflicts; the hold rows stay so
            sel = [r for r, h in zip(ok_rows, holds) if h or not hold]
            out, cst = run_conflicts(e, T, occ, sel, None, hold, ad, rs)
            assert np.array_equal(out, np.tile(np.array([-1, 0, -1, 0], np.int32), (len(sel), 1))) and not cst.any()
        # d_tick NULL: all earliest; rows of exactly L and L - 1 cells: the second overflows, untouched
        far = int(np.argmax(arrive[0]))
        L = int(arrive[0, far]) + 1
        for cap, want_st in ((L, 0), (L - 1, 3)):
            rows2, lens2, st2, tk2 = run_paths(e, T, occ, 2, reach, [(0, far, 0), (0, s, 0)], cap, ad, rs, ticks=False)
            assert list(st2) == [want_st, 0] and list(tk2) == [L - 1, 0] and list(lens2) == [L if want_st == 0 else 0, 1]
        # garbage reach planes: every walk ends and says so
        j3 = np.random.default_rng(1).integers(0, 2 ** 64, (3, 2 * (T + 1) * 20), dtype=np.uint64)
        junk = e.put(j3[0] & j3[1] & j3[2])                           # one bit in eight: most walks lose their predecessor
        rows3, lens3, st3, tk3 = run_paths(e, T, occ, 2, junk, [(b, int(v), k) for b in (0, 1) for v in rnd.integers(0, 400, 20) for k in (-1, -2, T)], T + 1, ad, rs)
        assert np.all((st3 == 0) | (st3 == 1) | (st3 == 3)) and (st3 == 3).any()
        junk.free()
    finally:
        for b in (occ, reach, da):
            b.free()
        e.close()


def test_conflict_kinds_status_and_hold():
    S = np.zeros((3, 4), bool)
    S[2, 3] = True
    T = 6
    D = sc.planes((3, 4), T, [[1, 0], [6]], [0, 1], "vanish")[0]
    D2 = sc.planes((3, 4), T, [[9, 5, 5, 1]], [2], "stay")[0]
    rows = [[0, 1], [4, 0], [5, 10], [7, 10], [7, 11], [4, 6], [1, 1], [11], [4, 4, 4, 4], [0], [4, 5], [0, 1, 2, 6, 10, 9, 8, 4, 0], [0, 1, 5, 4]]
    t0 = [0, 0, 0, 0, 0, 0, 0, 2, 4, 6, 0, 0, 1]
    e = engine(S)
    try:
        for planes in (D, D2):
            occ = e.put(sc.pack(planes))
            for ad, rs in POLICIES:
                for hold in (False, True):
                    out, st = run_conflicts(e, T, occ, rows, t0, hold, ad, rs)
                    for i, r in enumerate(rows):
                        w, wst = sc.conflicts(S, planes, r, t0[i], ad, rs, hold)
                        assert tuple(out[i]) == w and st[i] == wst, (i, ad, rs, hold, out[i], w)
            occ.free()
        occ = e.put(sc.pack(D))
        out, st = run_conflicts(e, T, occ, rows[:4], None, False, 1, 1)
        assert [int(k) for k in out[:, 1]] == [sc.SWAP, sc.VERTEX, sc.CORNER, sc.STATIC] and not st.any()
        out, st = run_conflicts(e, T, occ, [[1], [], [1] * 5, [12], [-1], [1], [1]], [0, 0, 0, 0, 0, -1, T + 1], False, 1, 1, cap=4, lens=[1, 0, 5, 1, 1, 1, 1])
        assert list(st) == [0, 1, 1, 1, 1, 1, 1] and all(tuple(o) == (-1, 0, -1, 0) for o in out[1:])
        occ.free()
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def g256():
    g, s, t = gio.grid("g256")
    return g == 1, s, t


def test_a_static_route_meets_a_patrol_on_g256():
    S, s, t = g256()
    e = engine(S)
    try:
        paths, st = e.astar_host(2, [s], [t], path_cap=4096)          # the Dijkstra variant's route on the static map
        route = [int(v) for v in paths[0]]
        assert st[0] == 0 and len(route) > 40
        T = len(route) + 40
        mid = len(route) // 2
        patrol = route[mid + 6:mid - 7:-1]                            # walks the route's middle stretch against the robot
        D = sc.planes((256, 256), T, [patrol], [mid - 6], "vanish")[0]
        want, wst = sc.conflicts(S, D, route, 0, 1, 1)
        assert want[0] >= 0 and want[1] in (sc.VERTEX, sc.SWAP) and want[3] >= 1 and wst == 0     # the model finds the conflict
        st8 = pathfit_spacetime(S, T, e)
        st8.add([np.array(patrol, np.int32)], start_ticks=[mid - 6], after_end="vanish")
        assert np.array_equal(st8.occupancy(), D)
        first, kind, cell, count = st8.conflicts([np.array(route, np.int32)])
        assert (int(first[0]), int(kind[0]), int(cell[0]), int(count[0])) == want and st8.status[0] == 0
        arrive = st8.arrival([(s // 256, s % 256)])                   # ... and the space-time route goes round it
        got = st8.paths([(t // 256, t % 256)])[0]
        assert got is not None and len(got) == arrive[0].reshape(-1)[t] + 1 >= len(route)
        assert [int(c) for c in st8.conflicts([got])[0]] == [-1]
        st8.close()
    finally:
        e.close()


def pathfit_spacetime(S, T, e, rs=True, ad=True):
    import pathfit
    return pathfit.SpaceTime(np.asarray(S, np.uint8), T, rs, ad, engine=e)


@pytest.mark.parametrize("name", ["fig7", "g256"])
def test_plan_fleet_against_the_model(name):
    if name == "g256":
        S = g256()[0]
    else:
        S = gio.grid(name)[0] == 1
    R, C = S.shape
    rnd = np.random.default_rng(88)
    region = np.flatnonzero(~S[:32, :32].reshape(-1)) if name == "g256" else np.flatnonzero(~S.reshape(-1))
    W = min(C, 32)
    cells = [int(v) // W * C + int(v) % W for v in rnd.choice(region, 16, replace=False)]
    starts, goals = cells[:8], cells[8:]
    T = 90
    e = engine(S)
    try:
        for ad, rs in ((1, 1), (0, 1)) if name == "g256" else ((1, 1), (1, 0), (0, 1)):
            want, wst, wD = sc.fleet(S, T, starts, goals, ad, rs)
            f = pathfit_spacetime(S, T, e, bool(rs), bool(ad))
            routes, st = f.plan_fleet([(v // C, v % C) for v in starts], [(v // C, v % C) for v in goals])
            assert np.array_equal(st, wst)
            for i in range(8):
                assert (routes[i] is None) == (want[i] is None)
                if want[i] is not None:
                    assert routes[i].cells.tolist() == want[i], (name, ad, rs, i)
            assert np.array_equal(f.occupancy(), wD)
            shared, swaps, corner, n = sc.fleet_violations(want, T, C, rs)
            assert (shared, swaps, corner) == (0, 0, 0) and n == sum(r is not None for r in routes) >= 2
            f.close()
    finally:
        e.close()


def test_class_round_trip():
    S = seeded(12, 70, 0.15, 21)
    S[0, 0] = S[11, 69] = False
    T = 100
    e = engine(S)
    try:
        f = pathfit_spacetime(S, T, e)
        row = [(5, c) for c in range(69, 0, -1)]
        f.add([row], after_end="vanish", corners=True).add([[(3, 3)]], start_ticks=[4])
        D = sc.planes((12, 70), T, [[5 * 70 + c for c in range(69, 0, -1)]], None, "vanish", True)[0] | sc.planes((12, 70), T, [[3 * 70 + 3]], [4], "stay")[0]
        assert np.array_equal(f.occupancy(), D) and not f.status.any()
        a = f.arrival([[(0, 0)], [(11, 69), (0, 0)]])
        for b, src in enumerate(([0], [11 * 70 + 69, 0])):
            wa, _ = sc.field_words(S, sc.pack(D), src, 1, 1, False)
            assert np.array_equal(a[b], wa) and list(f.info[b]) == list(sc.info_of(wa))
        got = f.paths([(11, 69), (0, 0)], "hold")
        reach = [sc.unpack(sc.field_words(S, sc.pack(D), src, 1, 1)[1], 70) for src in ([0], [11 * 70 + 69, 0])]
        for q, v in enumerate((11 * 70 + 69, 0)):
            want, wst, wtk = sc.route(S, D, reach[q], v, -2, 1, 1)
            assert (got[q].cells.tolist() if got[q] is not None else None, f.status[q], f.ticks[q]) == (want, wst, wtk)
        f.clear()
        assert not f.occupancy().any()
        f.close()
    finally:
        e.close()


# ---- 4. argument errors leave every output untouched
def test_raw_argument_errors_leave_canaries():
    from pathfit._lib import PathfitError
    S = np.zeros((5, 70), bool)
    T, W = 6, 5 * 2
    e = engine(S)
    occ0 = np.arange((T + 1) * W, dtype=np.uint64)
    ob = e.put(np.concatenate([np.full(PAD, CAN64), occ0, np.full(PAD, CAN64)]).astype(np.uint64))
    occ = view(e, ob, (T + 1) * W)
    outs = {k: between_canaries(e, 4096, dt) for k, dt in (("i", np.int32), ("r", np.uint64), ("l", np.int64), ("j", np.int32), ("k", np.int32), ("m", np.int32))}
    vi, vr, vl, vj, vk, vm = (view(e, outs[k], 4096) for k in "irljkm")
    rows, lens, t0 = e.put(np.zeros((2, 4), np.int32)), e.put(np.array([2, 2], np.int32)), e.put(np.zeros(2, np.int32))

    def field(**kw):
        a = dict(horizon=T, d_occ=occ, set_off=[0, 1], sources=[3], d_arrive=vi, d_reach=vr, d_info=vl)
        a.update(kw)
        e.spacetime_field(a["horizon"], a["d_occ"], a["set_off"], a["sources"], a["d_arrive"], True, True, a["d_reach"], a["d_info"])

    def stamp(**kw):
        a = dict(horizon=T, d_occ=occ, n=2, path_cap=4, d_cells=rows, d_len=lens, d_status=vi)
        a.update(kw)
        e.spacetime_stamp(a["horizon"], a["d_occ"], a["n"], a["path_cap"], a["d_cells"], a["d_len"], a["d_status"], t0)

    def paths(**kw):
        a = dict(horizon=T, d_occ=occ, B=1, d_reach=vr, n=2, d_set_idx=t0, d_target=t0, path_cap=8, d_cells=vi, d_len=vj, d_status=vk)
        a.update(kw)
        e.spacetime_paths(a["horizon"], a["d_occ"], a["B"], a["d_reach"], a["n"], a["d_set_idx"], a["d_target"], a["path_cap"], a["d_cells"], a["d_len"],
                          a["d_status"], t0, vm)

    def conflicts(**kw):
        a = dict(horizon=T, d_occ=occ, n=2, path_cap=4, d_cells=rows, d_len=lens, d_out=vi, d_status=vj)
        a.update(kw)
        e.spacetime_conflicts(a["horizon"], a["d_occ"], a["n"], a["path_cap"], a["d_cells"], a["d_len"], a["d_out"], a["d_status"], t0)

    bad = [(field, dict(horizon=-1), "horizon"), (field, dict(horizon=2 ** 20 + 1), "horizon"), (field, dict(set_off=[0]), "at least one source set"),
           (field, dict(d_occ=None), "must not be null"), (field, dict(d_arrive=None), "must not be null"), (field, dict(set_off=[1, 2]), "start at 0"),
           (field, dict(set_off=[0, 2, 1], sources=[1, 2]), "decrease"), (field, dict(sources=[350]), "source 0 = 350 lies outside"),
           (field, dict(set_off=[0, 2], sources=[3, -1]), "source 1 = -1 lies outside"),
           (stamp, dict(horizon=-1), "horizon"), (stamp, dict(n=-1), "bad arguments"), (stamp, dict(path_cap=0), "bad arguments"), (stamp, dict(d_occ=None), "must not be null"),
           (stamp, dict(d_cells=None), "must not be null"), (stamp, dict(d_len=None), "must not be null"), (stamp, dict(d_status=None), "must not be null"),
           (paths, dict(horizon=2 ** 20 + 1), "horizon"), (paths, dict(B=0), "bad arguments"), (paths, dict(n=-1), "bad arguments"), (paths, dict(path_cap=0), "bad arguments"),
           (paths, dict(d_reach=None), "must not be null"), (paths, dict(d_target=None), "must not be null"), (paths, dict(d_set_idx=None), "must not be null"),
           (paths, dict(d_cells=None), "must not be null"), (paths, dict(d_status=None), "must not be null"),
           (conflicts, dict(horizon=-2), "horizon"), (conflicts, dict(n=-1), "bad arguments"), (conflicts, dict(path_cap=0), "bad arguments"),
           (conflicts, dict(d_occ=None), "must not be null"), (conflicts, dict(d_out=None), "must not be null"), (conflicts, dict(d_status=None), "must not be null")]
    try:
        for call, kw, text in bad:
            with pytest.raises(PathfitError, match=text):
                call(**kw)
        for call in (stamp, paths, conflicts):                        # n == 0 returns 0 and launches nothing
            call(n=0)
        L = e.L
        assert L.pf_spacetime_field(None, 1, 1, T, occ.ptr, 1, None, None, vi.ptr, None, None) == -2
        assert L.pf_spacetime_stamp(None, T, occ.ptr, 0, 1, None, None, None, 0, 0, 0, None) == -2
        assert L.pf_spacetime_paths(None, 1, 1, T, occ.ptr, 1, None, 0, None, None, None, 1, None, None, None, None) == -2
        assert L.pf_spacetime_conflicts(None, 1, 1, T, occ.ptr, 0, 1, None, None, None, 0, None, None) == -2
        for k, b in outs.items():
            a = b.download()
            assert np.all(a == (CAN64 if a.dtype == np.uint64 else CANARY)), k
        assert np.array_equal(inner(ob, "planes"), occ0)
    finally:
        for b in list(outs.values()) + [ob, rows, lens, t0]:
            b.free()
        e.close()
