"""SpaceTime argument checks: ValueError before any device is touched, and the numpy side of the class over a model engine whose
buffers are host arrays and whose four space-time calls are the CPU model (runs on a CPU-only host)."""
import ctypes

import numpy as np
import pytest

import spacetime_checkers as sc


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import spacetime

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(spacetime, "Engine", boom)


class HostMemory:
    """The few library calls DevBuf makes, on host arrays: a DevBuf of a ModelEngine is a numpy array behind a pointer."""

    def __init__(self):
        self.live = {}

    def pf_dev_alloc(self, h, nbytes, ref):
        a = np.zeros(max(int(nbytes), 1), np.uint8)
        self.live[a.ctypes.data] = a
        ref._obj.value = a.ctypes.data
        return 0

    def pf_dev_free(self, h, ptr):
        self.live.pop(ptr, None)
        return 0

    def pf_h2d(self, h, dst, src, n):
        ctypes.memmove(dst, src, n)
        return 0

    pf_d2h = pf_d2d = pf_h2d

    def pf_memset(self, h, ptr, value, n):
        ctypes.memset(ptr, value, n)
        return 0


def host(buf, count, dtype):
    """The `count` elements behind a buffer's pointer as a writable array."""
    dtype = np.dtype(dtype)
    return np.frombuffer((ctypes.c_char * (int(count) * dtype.itemsize)).from_address(buf.ptr), dtype)


class ModelEngine:
    """An engine of the grid's shape without a device: buffers in host memory, the space-time calls answered by the model.  `sealed`:
    every call fails the test (the arguments must be checked first)."""
    h = 1

    def __init__(self, g):
        self.g = np.asarray(g)
        self.R, self.C = self.g.shape
        self.grid_u8 = np.asarray(g, np.uint8)
        self.L = HostMemory()
        self.sealed = False
        self.calls = []

    def _ck(self, rc):
        assert rc == 0

    def _open(self, name):
        assert not self.sealed, f"the device was touched before the arguments were checked ({name})"
        self.calls.append(name)

    def buf(self, shape, dtype):
        from pathfit.engine import DevBuf
        self._open("buf")
        return DevBuf(self, shape, dtype)

    def put(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype)
        return self.buf(a.shape if a.ndim else (1,), a.dtype).upload(a)

    def update_grid(self, g):
        self.g = np.asarray(g)
        self.grid_u8 = np.asarray(g, np.uint8)

    def last_kernel_ms(self):
        return 0.25

    def close(self):
        self.h = None

    # ---- the four calls
    def _static(self):
        return self.g == 1

    def _planes(self, T, d_occ):
        Wc = (self.C + 63) // 64
        words = host(d_occ, (T + 1) * self.R * Wc, np.uint64).reshape(T + 1, self.R, Wc)
        return words, sc.unpack(words, self.C)

    def _rows(self, n, cap, d_cells, d_len, d_t0):
        cells, lens = host(d_cells, n * cap, np.int32).reshape(n, cap), host(d_len, n, np.int32)
        t0 = host(d_t0, n, np.int32) if d_t0 else np.zeros(n, np.int32)
        return [cells[i, :lens[i]].tolist() if 0 < lens[i] <= cap else [] for i in range(n)], t0     # (an empty row is a bad row, as one too long)

    def spacetime_stamp(self, T, d_occ, n, cap, d_cells, d_len, d_status, d_t0=None, after_end=True, corners=False, clear=False):
        self._open("spacetime_stamp")
        if n == 0:
            return
        words, _ = self._planes(T, d_occ)
        rows, t0 = self._rows(n, cap, d_cells, d_len, d_t0)
        D, st = sc.planes((self.R, self.C), T, rows, t0, "stay" if after_end else "vanish", corners)
        if clear:
            words[:] = 0
        words |= sc.pack(D)
        host(d_status, n, np.int32)[:] = st

    def spacetime_field(self, T, d_occ, set_off, sources, d_arrive, allow_diag=True, restrict_corner=True, d_reach=None, d_info=None):
        self._open("spacetime_field")
        words, _ = self._planes(T, d_occ)
        off, src = np.asarray(set_off), np.asarray(sources)
        B, RC, W = len(off) - 1, self.R * self.C, self.R * words.shape[2]
        for b in range(B):
            a, r = sc.field_words(self._static(), words, src[off[b]:off[b + 1]], int(allow_diag), int(restrict_corner))
            host(d_arrive, B * RC, np.int32)[b * RC:(b + 1) * RC] = a.reshape(-1)
            if d_reach:
                host(d_reach, B * (T + 1) * W, np.uint64)[b * (T + 1) * W:(b + 1) * (T + 1) * W] = r.reshape(-1)
            if d_info:
                host(d_info, 4 * B, np.int64)[4 * b:4 * b + 4] = sc.info_of(a)

    def spacetime_paths(self, T, d_occ, B, d_reach, n, d_set_idx, d_target, cap, d_cells, d_len, d_status, d_tick=None, d_tick_out=None, allow_diag=True,
                        restrict_corner=True):
        self._open("spacetime_paths")
        if n == 0:
            return
        words, D = self._planes(T, d_occ)
        W = self.R * words.shape[2]
        reach = sc.unpack(host(d_reach, B * (T + 1) * W, np.uint64).reshape(B, T + 1, self.R, words.shape[2]), self.C)
        ks, tg = host(d_set_idx, n, np.int32), host(d_target, n, np.int32)
        tk = host(d_tick, n, np.int32) if d_tick else np.full(n, -1, np.int32)
        cells, lens, st = host(d_cells, n * cap, np.int32).reshape(n, cap), host(d_len, n, np.int32), host(d_status, n, np.int32)
        for q in range(n):
            ok = 0 <= ks[q] < B
            got, s, used = sc.route(self._static(), D, reach[ks[q]], int(tg[q]), int(tk[q]), int(allow_diag), int(restrict_corner), cap) if ok else (None, 1, -1)
            lens[q], st[q] = (len(got) if got else 0), s
            if got:
                cells[q, :len(got)] = got
            if d_tick_out:
                host(d_tick_out, n, np.int32)[q] = used

    def spacetime_conflicts(self, T, d_occ, n, cap, d_cells, d_len, d_out, d_status, d_t0=None, hold=False, allow_diag=True, restrict_corner=True):
        self._open("spacetime_conflicts")
        if n == 0:
            return
        _, D = self._planes(T, d_occ)
        rows, t0 = self._rows(n, cap, d_cells, d_len, d_t0)
        out, st = host(d_out, 4 * n, np.int32).reshape(n, 4), host(d_status, n, np.int32)
        for i, r in enumerate(rows):
            out[i], st[i] = sc.conflicts(self._static(), D, r, int(t0[i]), int(allow_diag), int(restrict_corner), hold, cap)

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


GRID = (np.random.default_rng(3).random((7, 9)) < 0.2).astype(int)
GRID[0, 0] = GRID[6, 8] = 0


def make(g=GRID, horizon=20, **kw):
    from pathfit import SpaceTime
    return SpaceTime(g, horizon, **kw)


def sealed():
    e = ModelEngine(GRID)
    f = make(engine=e)
    e.sealed = True
    return f, e


def test_constructor_errors(no_engine):
    for g in (np.zeros(16, int), np.zeros((2, 2, 2), int)):
        with pytest.raises(ValueError, match="^SpaceTime: grid must be 2-D"):
            make(g)
    for T in (-1, 2 ** 20 + 1, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="^SpaceTime: horizon must be an integer in"):
            make(horizon=T)

    class Other:
        R, C = 3, 3
    with pytest.raises(ValueError, match="^SpaceTime: the engine's grid has another shape"):
        make(engine=Other())


def test_add_errors():
    from pathfit import CellPath
    f, e = sealed()
    for bad, text in ((5, "obstacles must be a sequence of paths"), ([5], "must be a CellPath, a list of"), ([[(0, 0), (7, 0)]], r"obstacles\[0\]\[1\] = \(7, 0\) is outside"),
                      ([[]], r"obstacles\[0\] is empty"), ([np.array([1, 63], np.int32)], r"obstacles\[0\]\[1\] = cell 63 is outside"),
                      ([CellPath([1, 2], 8)], "belongs to a grid of 8 columns"), ([[(0, 0), 3]], "must be an")):
        with pytest.raises(ValueError, match="^SpaceTime: .*" + text):
            f.add(bad)
    for t0 in ([0, 0], [1.5], [-1], [21], "x"):
        with pytest.raises(ValueError, match="^SpaceTime: start_ticks"):
            f.add([[(0, 0)]], start_ticks=t0)
    with pytest.raises(ValueError, match="^SpaceTime: after_end must be 'stay' or 'vanish'"):
        f.add([[(0, 0)]], after_end="go")
    for kw in (dict(n=-1, path_cap=4), dict(n=2, path_cap=0), dict(n=2, path_cap=4, after_end=1)):
        with pytest.raises(ValueError, match="^SpaceTime: "):
            f.add_rows(None, None, **kw)
    with pytest.raises(ValueError, match="^SpaceTime: d_cells must be a DevBuf"):
        f.add_rows(np.zeros(8, np.int32), None, 2, 4)
    assert e.calls == ["buf"] * 0 and f.add([]).status.size == 0


def test_arrival_paths_conflicts_fleet_errors():
    f, e = sealed()
    for bad, text in ("ab", "sources must be a list"), (7, "sources must be a list"), ([], "sources is empty"), ([(0, 9)], r"sources\[0\] = \(0, 9\) is outside"), \
            ([[(0, 0)], [(7, 7)]], r"sources\[1\]\[0\] = \(7, 7\) is outside"), ([[(0, 0)], 4], r"sources\[1\] must be a list"):
        with pytest.raises(ValueError, match="^SpaceTime: " + text):
            f.arrival(bad)
    with pytest.raises(ValueError, match="^SpaceTime: paths needs an arrival call"):
        f.paths([(0, 0)])
    with pytest.raises(ValueError, match=r"^SpaceTime: targets\[0\] = \(9, 9\) is outside"):
        f.paths([(9, 9)])
    for ticks in ("soon", -1, 21, [1, 2], 1.5):
        with pytest.raises(ValueError, match="^SpaceTime: ticks must be None, 'hold'"):
            f.paths([(0, 0)], ticks)
    with pytest.raises(ValueError, match=r"^SpaceTime: paths\[0\]\[0\] = \(0, 9\) is outside"):
        f.conflicts([[(0, 9)]])
    with pytest.raises(ValueError, match="^SpaceTime: start_ticks"):
        f.conflicts([[(0, 0)]], start_ticks=[30])
    with pytest.raises(ValueError, match="^SpaceTime: 2 starts and 1 goals"):
        f.plan_fleet([(0, 0), (1, 1)], [(2, 2)])
    for order in ([0, 0], [0], [0, 2], 5):
        with pytest.raises(ValueError, match="^SpaceTime: order"):
            f.plan_fleet([(0, 0), (6, 8)], [(6, 8), (0, 0)], order)
    with pytest.raises(ValueError, match=r"^SpaceTime: goals\[1\] = \(0, -1\) is outside"):
        f.plan_fleet([(0, 0), (6, 8)], [(6, 8), (0, -1)])
    assert e.calls == []


def test_k_errors_after_an_arrival_call():
    e = ModelEngine(GRID)
    f = make(engine=e)
    f.arrival([[(0, 0)], [(6, 8)], [(0, 0), (6, 8)]])
    e.sealed = True
    with pytest.raises(ValueError, match="^SpaceTime: k is needed: the last arrival call had 3 sets and there are 2 targets"):
        f.paths([(0, 0), (1, 1)])
    for k in (3, -1, [0, 3], [0], 1.5):
        with pytest.raises(ValueError, match="^SpaceTime: k"):
            f.paths([(0, 0), (1, 1)], k=k)


def test_the_numpy_side_over_the_model_engine():
    from pathfit import CellPath
    from pathfit._lib import PathfitError
    e = ModelEngine(GRID)
    S = GRID == 1
    T, C = 20, 9
    f = make(engine=e, horizon=T)
    patrol = [(3, c) for c in range(8, -1, -1)]
    f.add([patrol, CellPath([6 * 9 + 8], 9)], start_ticks=[2, 5], after_end="vanish", corners=True)
    f.add([np.array([10], np.int32)], after_end="stay")
    D = sc.planes((7, 9), T, [[27 + c for c in range(8, -1, -1)], [62]], [2, 5], "vanish", True)[0] | sc.planes((7, 9), T, [[10]], None, "stay")[0]
    assert np.array_equal(f.occupancy(), D) and f.occupancy().dtype == bool and not f.status.any() and f.kernel_ms == 0.25
    a = f.arrival([(0, 0)])
    want, wr = sc.field_words(S, sc.pack(D), [0], 1, 1)
    assert a.shape == (1, 7, 9) and a.dtype == np.int32 and np.array_equal(a[0], want) and list(f.info[0]) == list(sc.info_of(want))
    assert np.array_equal(f.reach_device.download().reshape(T + 1, 7, 1), wr) and f.sets == 1
    reach = sc.unpack(wr, 9)
    got = f.paths([(6, 8), (1, 1), (6, 8)], ticks=[T, 1, T])
    for q, (v, tick) in enumerate(((62, T), (10, 1), (62, T))):
        w, st, tk = sc.route(S, D, reach, v, tick, 1, 1)
        assert (None if got[q] is None else got[q].cells.tolist(), f.status[q], f.ticks[q]) == (w, st, tk)
    assert got[1] is None and isinstance(got[0], CellPath) and got[0][0] == (0, 0)
    hold = f.paths([(6, 8)], "hold")[0]
    assert hold.cells.tolist() == sc.route(S, D, reach, 62, -2, 1, 1)[0] and f.ticks[0] == sc.hold_tick(reach, D, 62)
    first, kind, cell, count = f.conflicts([hold, [(2, 0), (3, 0), (3, 1)]], start_ticks=[0, 9], hold=True)
    assert (first[0], kind[0], cell[0], count[0]) == (-1, 0, -1, 0)
    assert (first[1], kind[1], cell[1], count[1]) == sc.conflicts(S, D, [18, 27, 28], 9, 1, 1, True)[0] and list(f.status) == [0, 0]
    assert f.paths([], None) == [] and f.conflicts([])[0].size == 0
    a2 = f.arrival([[(0, 0)], [(6, 8)]], keep=False)
    assert a2.shape == (2, 7, 9) and f.reach_device is None and np.array_equal(a2[0], a[0])
    rows = e.put(np.array([[5, 6, 7, 0], [200, 0, 0, 0]], np.int32))
    lens = e.put(np.array([3, 1], np.int32))
    assert list(f.add_rows(rows, lens, 2, 4, after_end="vanish")) == [0, 1]
    D |= sc.planes((7, 9), T, [[5, 6, 7]], None, "vanish")[0]
    assert np.array_equal(f.occupancy(), D)
    f.clear()
    assert not f.occupancy().any()
    # the fleet, against the model's
    starts, goals = [(0, 0), (6, 8), (0, 8)], [(6, 8), (0, 0), (6, 0)]
    routes, st = f.plan_fleet(starts, goals, order=[2, 0, 1])
    want, wst, wD = sc.fleet(S, T, [0, 62, 8], [62, 0, 54], 1, 1, order=[2, 0, 1])
    assert [None if r is None else r.cells.tolist() for r in routes] == want and np.array_equal(st, wst) and np.array_equal(f.occupancy(), wD)
    f.close()
    with pytest.raises(PathfitError, match="^SpaceTime: the field is closed"):
        f.arrival([(0, 0)])
