"""Clearance.widest / max_margin / widest_path / widest_paths: ValueError before any device call, and the facade's numpy side over a
model engine whose `clearance_widest` is the checker (runs on a CPU-only host)."""
import math

import numpy as np
import pytest

import clearance_checkers as ck
import golden_io as gio
import widest_checkers as wc


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import clearance

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(clearance, "Engine", boom)
    monkeypatch.setattr(clearance, "DistanceField", boom)


class HostBuf:
    def __init__(self, n, dtype):
        self.a = np.zeros(int(np.prod(n)), dtype)
        self.freed = False

    def download(self):
        return self.a.copy()

    def read(self, off, n):
        return self.a[off:off + n].copy()

    def free(self):
        self.freed = True


class ModelEngine:
    """An engine of the grid's shape whose `clearance_field` and `clearance_widest` are the models; every device call fails the test
    when `sealed`."""
    h = 1

    def __init__(self, g, border=False):
        self.g, (self.R, self.C) = g, g.shape
        self.grid_u8 = np.asarray(g, np.uint8)
        self.sealed, self.widest_calls, self.bufs = False, 0, []

    def buf(self, n, dtype):
        assert not self.sealed, "the device was touched before the arguments were checked (buf)"
        self.bufs.append(HostBuf(n, dtype))
        return self.bufs[-1]

    def clearance_field(self, d_d2, border, d_near, d_info):
        d2, near, info = ck.brute_force(self.g, border)
        d_d2.a[:] = d2.reshape(-1)
        d_info.a[:] = info

    def clearance_widest(self, d_d2, set_off, sources, d_out, allow_diag=True, restrict_corner=True, d_info=None):
        assert not self.sealed, "the device was touched before the arguments were checked (clearance_widest)"
        sets = [list(sources[set_off[b]:set_off[b + 1]]) for b in range(len(set_off) - 1)]
        w, info = wc.widest(d_d2.a.reshape(self.R, self.C), sets, allow_diag, restrict_corner)
        d_out.a[:] = w.reshape(-1)
        d_info.a[:] = info.reshape(-1)
        self.widest_calls += 1
        self.last = (sets, bool(allow_diag), bool(restrict_corner))

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def make(g, **kw):
    from pathfit import Clearance
    return Clearance(g, **kw)


@pytest.fixture
def sealed(no_engine):
    g, _, _ = gio.grid("img1")
    e = ModelEngine(g)
    cl = make(g, engine=e)
    e.sealed = True
    return cl


@pytest.fixture
def model(no_engine):
    g, _, _ = gio.grid("img1")
    return make(g, engine=ModelEngine(g))


BAD_NESTING = "sources must be an \\(r, c\\) pair, a list of such pairs or a list of such lists"


@pytest.mark.parametrize("bad, msg", [
    (5, BAD_NESTING),
    ("ab", BAD_NESTING),
    (None, BAD_NESTING),
    ([3.5, 2], BAD_NESTING),
    ([[[(0, 0)]]], r"sources\[0\]\[0\] must be an \(r, c\) pair"),
    ([[(0, 0)], 7], r"sources\[1\] must be a list of \(r, c\) pairs"),
    ([], "sources is empty"),
    ([[]], r"sources\[0\] is empty"),
    ([[(0, 0)], []], r"sources\[1\] is empty"),
    ((0, 20), r"sources = \(0, 20\) is outside the 20x20 grid"),
    ((-1, 0), r"sources = \(-1, 0\) is outside the 20x20 grid"),
    ([(0, 0), (20, 0)], r"sources\[1\] = \(20, 0\) is outside the 20x20 grid"),
    ([(0, 0), (1, 2, 3)], r"sources\[1\] must be an \(r, c\) pair"),
    ([[(0, 0)], [(1, 1), (0, 99)]], r"sources\[1\]\[1\] = \(0, 99\) is outside the 20x20 grid"),
    ([[(0, 0)], [(1, 1), 7]], r"sources\[1\]\[1\] must be an \(r, c\) pair"),
])
def test_sources(sealed, bad, msg):
    with pytest.raises(ValueError, match="^Clearance: " + msg):
        sealed.widest(bad)


@pytest.mark.parametrize("a, b, msg", [
    ((0, 20), (1, 1), r"source = \(0, 20\) is outside the 20x20 grid"),
    ((0, 0), (20, 1), r"target = \(20, 1\) is outside the 20x20 grid"),
    (7, (1, 1), r"source must be an \(r, c\) pair"),
    ((0, 0), "ab", r"target must be an \(r, c\) pair"),
])
def test_pairs(sealed, a, b, msg):
    for call in (sealed.max_margin, sealed.widest_path):
        with pytest.raises(ValueError, match="^Clearance: " + msg):
            call(a, b)


@pytest.mark.parametrize("targets, msg", [
    (5, "targets must be a list of"),
    ([(0, 0), (0, 20)], r"targets\[1\] = \(0, 20\) is outside the 20x20 grid"),
    ([(0, 0), 3], r"targets\[1\] must be an \(r, c\) pair"),
])
def test_targets(sealed, targets, msg):
    with pytest.raises(ValueError, match="^Clearance: " + msg):
        sealed.widest_paths((0, 0), targets)
    with pytest.raises(ValueError, match=r"^Clearance: source = \(0, 20\) is outside"):
        sealed.widest_paths((0, 20), [(0, 0)])


def test_checked_calls_reach_the_device(sealed):
    for call in (lambda: sealed.widest((0, 0)), lambda: sealed.widest([(0, 0), (0, 0)]), lambda: sealed.widest([[(0, 0)], [(1, 1)]]),
                 lambda: sealed.max_margin((0, 0), (1, 1)), lambda: sealed.widest_path((0, 0), (1, 1)),
                 lambda: sealed.widest_paths((0, 0), [(1, 1)])):
        with pytest.raises(AssertionError, match="the device was touched"):
            call()
    paths, ws = sealed.widest_paths((0, 0), [])                       # no target: an answer, no device call
    assert paths == [] and len(ws) == 0


@pytest.mark.parametrize("kw", [{}, {"margin": 1.5, "margin_sq": 3}])
def test_reachable_takes_exactly_one_margin(model, kw):
    f = model.widest((0, 0))
    with pytest.raises(ValueError, match="^Clearance: give exactly one of margin and margin_sq"):
        f.reachable(**kw)
    with pytest.raises(ValueError, match=r"^Clearance: margin_sq must be an integer in \[1, 2\^31 - 1\]"):
        f.reachable(margin_sq=0)
    with pytest.raises(ValueError, match=r"^Clearance: margin must be a number in \(0, 46340\)"):
        f.reachable(margin=0)


def test_the_three_forms_of_sources(model):
    e = model.engine
    free = [tuple(int(x) for x in p) for p in np.argwhere(model.d2 >= 4)[:3]]
    one = model.widest(free[0])
    assert e.last[0] == [[free[0][0] * 20 + free[0][1]]] and one.B == 1 and one.w.shape == (1, 20, 20)
    lst = model.widest(free, False, True)
    assert e.last == ([[r * 20 + c for r, c in free]], False, True) and lst.w.shape == (1, 20, 20)
    many = model.widest([[free[0]], free[1:], np.array(free)])
    assert [len(s) for s in e.last[0]] == [1, 2, 3] and many.w.shape == (3, 20, 20) and many.info.shape == (3, 4)
    assert np.array_equal(many.w[0], one.w[0]) and many.info.dtype == np.int64
    want, winfo = wc.widest(model.d2, e.last[0], True, True)
    assert np.array_equal(many.w, want) and np.array_equal(many.info, winfo)


def test_radius_reachable_and_close(model):
    import pathfit
    s = tuple(int(x) for x in np.argwhere(model.d2 == model.d2.max())[0])
    f = model.widest(s)
    w = f.w
    assert w.dtype == np.int32 and w is f.w and w[0][s] == model.d2[s] and (w[0] > 0).any() and (w[0] == 0).any()
    assert np.array_equal(f.radius, np.sqrt(w.astype(np.float64)))
    for m in (1.0, 1.5, 2.0, 2.9):
        assert np.array_equal(f.reachable(margin=m), w >= ck.margin_sq(m))
    assert np.array_equal(f.reachable(margin_sq=4), w >= 4) and f.reachable(margin_sq=4).dtype == bool
    assert np.array_equal(f.reachable(margin_sq=1)[0], w[0] > 0)
    assert f.at(0, s[0] * 20 + s[1]) == model.d2[s]
    buf = f.w_device
    f.close()
    assert buf.freed and f.w is w                                     # what was downloaded stays readable
    g = model.widest(s)
    assert g.at(0, s[0] * 20 + s[1]) == model.d2[s] and g._w is None  # one word read, nothing downloaded
    g.close()
    with pytest.raises(pathfit.PathfitError, match="Clearance: the widest-path field is closed"):
        g.w
    # a map without an obstacle: w is PF_CLEAR_NONE, the radius inf
    z = np.zeros((3, 4), int)
    open_ = make(z, engine=ModelEngine(z)).widest((1, 1))
    assert np.all(open_.w == wc.NONE) and np.all(np.isinf(open_.radius)) and np.all(open_.reachable(margin_sq=wc.NONE))


def test_max_margin(model):
    d2 = model.d2
    free = np.argwhere(d2 >= 1)
    s = tuple(int(x) for x in free[0])
    w = wc.widest_one(d2, [s[0] * 20 + s[1]], True, True)[0]
    for t in [tuple(int(x) for x in p) for p in free[::17]] + [tuple(int(x) for x in np.argwhere(d2 == 0)[0])]:
        got = model.max_margin(s, t)
        assert got == (int(w[t]), math.sqrt(int(w[t]))) and isinstance(got[0], int)
    assert all(b.freed for b in model.engine.bufs[2:])                # every field of a call is freed again
    z = np.zeros((3, 4), int)
    assert make(z, engine=ModelEngine(z)).max_margin((0, 0), (2, 3)) == (wc.NONE, math.inf)


def test_widest_paths_groups_the_targets_by_threshold(model, monkeypatch):
    from pathfit import Clearance
    from pathfit.paths import CellPath
    d2 = model.d2
    s = tuple(int(x) for x in np.argwhere(d2 == d2.max())[0])
    sid = s[0] * 20 + s[1]
    w = wc.widest_one(d2, [sid], True, False)[0].reshape(-1)
    targets = [int(v) for v in np.random.default_rng(5).choice(400, 40, replace=False)] + [sid]
    calls = []

    def routes(self, msq, source, tids, ad, rs):
        calls.append((msq, list(tids)))
        assert source == sid and (ad, rs) == (True, False)
        return [CellPath(np.array(wc.widest_path(self.grid, d2, source, t, ad, rs, w)[0], np.int32), 20) for t in tids]
    monkeypatch.setattr(Clearance, "_routes", routes)
    paths, ws = model.widest_paths(s, [(t // 20, t % 20) for t in targets], True, False)
    assert np.array_equal(ws, w[targets]) and ws.dtype == np.int32
    distinct = sorted(set(int(x) for x in w[targets] if x > 0))
    assert [c[0] for c in calls] == distinct and len(distinct) >= 2   # one route call per distinct threshold
    for msq, tids in calls:
        assert tids == [t for t in targets if w[t] == msq]
    for t, p, x in zip(targets, paths, ws):
        assert p.cells.tolist() == wc.widest_path(model.grid, d2, sid, t, True, False, w)[0] and bool(p) == (x > 0)
    assert paths[-1].tolist() == [s]                                  # source == target: the one-cell path
    # widest_path: one target; ([], 0) where no robot gets through
    wall = tuple(int(x) for x in np.argwhere(d2 == 0)[0])
    assert model.widest_path(s, wall, True, False) == ([], 0)
    p, x = model.widest_path(s, (targets[0] // 20, targets[0] % 20), True, False)
    assert (p.cells.tolist(), x) == wc.widest_path(model.grid, d2, sid, targets[0], True, False, w) or x == 0
