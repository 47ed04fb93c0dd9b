"""AnyAngle argument checks: ValueError before any device is touched, the node rules, `also`, `map`, `gap`, and the class's numpy side
over a model engine whose calls are tests/sight_checkers.py (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio
import sight_checkers as sc


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import any_angle

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(any_angle, "Engine", boom)


class HostBuf:
    def __init__(self, shape, dtype):
        self.a = np.zeros(shape, dtype).reshape(-1)

    def download(self):
        return self.a.copy()

    def free(self):
        pass


class ModelEngine:
    """An engine of the grid's shape whose sight calls are the model; every device call fails the test when `sealed`."""
    h = 1

    def __init__(self, g):
        self.g, (self.R, self.C) = np.array(g), g.shape
        self.grid_u8 = np.asarray(g, np.uint8)
        self.sealed = False
        self.calls = []

    def _open(self, name):
        assert not self.sealed, f"the device was touched before the arguments were checked ({name})"
        self.calls.append(name)

    def update_grid(self, g):
        self.g, self.grid_u8 = np.array(g), np.asarray(g, np.uint8)

    def buf(self, shape, dtype):
        self._open("buf")
        return HostBuf(shape, dtype)

    def put(self, arr):
        self._open("put")
        b = HostBuf(np.shape(arr), np.asarray(arr).dtype)
        b.a[:] = np.asarray(arr).reshape(-1)
        return b

    def sight_pack(self, nodes, d_adj, ld, strict, rsq, d_info):
        self._open("sight_pack")
        self.adj = sc.adjacency(sc.occ_of(self.g), nodes, strict, rsq)
        d_adj.a[:] = sc.pack_bits(self.adj, ld).reshape(-1)
        d_info.a[:] = sc.pack_info(self.adj)

    def sight_field(self, nodes, d_adj, ld, off, src, d_dist, d_parent, d_info):
        self._open("sight_field")
        adj, tail = sc.unpack_bits(d_adj.a.reshape(len(nodes), ld), len(nodes))
        assert not tail.any()
        self.nodes = np.asarray(nodes)
        self.dist, self.par, info = sc.field(adj, sc.weights(nodes, self.C), off, src)
        d_dist.a[:], d_parent.a[:], d_info.a[:] = self.dist.reshape(-1), self.par.reshape(-1), info.reshape(-1)

    def sight_field_work(self):
        return (1, 1, 0, 0)

    def sight_paths(self, nodes, B, d_dist, d_parent, n, d_target, way_cap, d_way, d_way_len, d_status, d_set, d_stats, reverse):
        self._open("sight_paths")
        way = d_way.a.reshape(n, way_cap)
        for i in range(n):
            b = int(d_set.a[i])
            st, cells, length, turns = sc.route(nodes, self.C, self.dist[b], self.par[b], int(d_target.a[i]), reverse, way_cap)
            way[i, :len(cells)] = cells
            d_way_len.a[i], d_status.a[i], d_stats.a[2 * i], d_stats.a[2 * i + 1] = len(cells), st, length, turns

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def make(g, *a, **kw):
    from pathfit import AnyAngle
    return AnyAngle(g, *a, **kw)


FIG7 = gio.grid("fig7")[0]


# ---- the constructor
def test_grid_must_be_2d(no_engine):
    for g in (np.zeros(16, int), np.zeros((2, 2, 2), int)):
        with pytest.raises(ValueError, match="^AnyAngle: grid must be 2-D"):
            make(g)


def test_engine_of_another_shape(no_engine):
    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^AnyAngle: the engine's grid has another shape"):
        make(FIG7, engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    with pytest.raises(AssertionError, match="the device was touched"):
        make(FIG7)


@pytest.mark.parametrize("kw, msg", [
    (dict(nodes="all"), r'nodes must be "free", "corners" or a list of \(r, c\) pairs'),
    (dict(nodes=5), "nodes must be a list"),
    (dict(nodes=[(0, 0), (20, 0)]), r"nodes\[1\] = \(20, 0\) is outside the 20x20 grid"),
    (dict(nodes=[(0, 0, 1)]), r"nodes\[0\] must be an \(r, c\) pair"),
    (dict(nodes=[]), "the node list holds 0 cells, 1 .. 16384 are supported"),
    (dict(also="ab"), "also must be a list"),
    (dict(also=[(0, -1)]), r"also\[0\] = \(0, -1\) is outside"),
    (dict(max_range=-1), "max_range must be None or a finite number >= 0"),
    (dict(max_range=float("nan")), "max_range must be None or a finite number >= 0"),
    (dict(max_range=True), "max_range must be None or a finite number >= 0"),
    (dict(max_range="far"), "max_range must be None or a finite number >= 0"),
])
def test_constructor_arguments(no_engine, kw, msg):
    with pytest.raises(ValueError, match="^AnyAngle: " + msg):
        make(FIG7, **kw)


def test_too_many_free_cells_and_a_grid_beyond_the_integer_range(no_engine):
    with pytest.raises(ValueError, match=r'^AnyAngle: the node list holds 16385 cells, 1 .. 16384 are supported \(nodes="corners" is the roadmap'):
        make(np.zeros((5, 3277), np.uint8))
    with pytest.raises(ValueError, match=r"^AnyAngle: R\^2 \+ C\^2 must stay below 2\^31 - 1"):
        make(np.zeros((46341, 1), np.uint8))
    with pytest.raises(AssertionError, match="the device was touched"):
        make(np.zeros((128, 128), np.uint8))                         # exactly 16 384 nodes pass


# ---- the node rules and `also`
def test_node_rules_and_also(no_engine):
    from pathfit.any_angle import corner_cells, free_cells
    for name in sc.MAPS:
        g = gio.grid(name)[0]
        assert np.array_equal(free_cells(g), sc.free_nodes(g)) and np.array_equal(corner_cells(g), sc.corner_nodes(g))
    g = np.zeros((5, 6), np.uint8)
    g[2, 2] = g[2, 3] = g[0, 0] = 1
    assert {divmod(int(v), 6) for v in corner_cells(g)} == {(1, 1), (1, 4), (3, 1), (3, 4)}
    a = make(g, "corners", also=[(4, 5), (0, 1), (4, 5), (1, 1)], engine=ModelEngine(g))
    assert list(a.node_cells) == [1, 7, 10, 19, 22, 29] and a.M == 6 and a.ld == 1 and a.node_cells.dtype == np.int32
    b = make(g, [(4, 0), (2, 2), (0, 1)], engine=ModelEngine(g))     # an explicit list, one cell on an obstacle: kept, isolated
    assert list(b.node_cells) == [1, 14, 24] and list(b.graph_info) == [2, 1, 0, 1]
    assert np.array_equal(b.adjacency(), np.array([[1, 0, 1], [0, 0, 0], [1, 0, 1]], bool)) and list(b.degree()) == [1, 0, 1]
    assert len(make(g, engine=ModelEngine(g)).node_cells) == 27


# ---- the calls
@pytest.fixture
def aa(no_engine):
    e = ModelEngine(FIG7)
    a = make(FIG7, engine=e)
    a.field([(0, 0), [(19, 19), (0, 0)]])
    e.sealed = True
    return a


def first_obstacle(g):
    return tuple(int(v) for v in np.argwhere(g == 1)[0])


@pytest.mark.parametrize("bad, msg", [
    ([], "sources is empty"), (5, "sources must be a list"), ("ab", "sources must be a list"),
    ([(0, 20)], r"sources\[0\] = \(0, 20\) is outside the 20x20 grid"), ([[(0, 0), (0, -1)]], r"sources\[0\]\[1\] = \(0, -1\) is outside"),
    ([3], r"sources\[0\] must be an \(r, c\) pair or a list of them"), ([[(0, 0, 0)]], r"sources\[0\]\[0\] must be an \(r, c\) pair"),
])
def test_sources(aa, bad, msg):
    with pytest.raises(ValueError, match="^AnyAngle: " + msg):
        aa.field(bad)


def test_a_source_or_target_that_is_no_node(aa):
    ob = first_obstacle(FIG7)
    with pytest.raises(ValueError, match=rf"^AnyAngle: sources\[0\] = \({ob[0]}, {ob[1]}\) is not among the nodes \(add it with also=\)"):
        aa.field([ob])
    with pytest.raises(ValueError, match=r"^AnyAngle: targets\[1\] = .* is not among the nodes"):
        aa.paths([(0, 0), ob])
    with pytest.raises(ValueError, match=r"^AnyAngle: a = .* is not among the nodes"):
        aa.route(ob, (0, 0))
    with pytest.raises(ValueError, match=r"^AnyAngle: b = \(0, 20\) is outside"):
        aa.route((0, 0), (0, 20))


def test_paths_map_and_gap_arguments(aa):
    for bad, msg in [(5, "targets must be a list"), ("ab", "targets must be a list"), ([(20, 0)], r"targets\[0\] = \(20, 0\) is outside")]:
        with pytest.raises(ValueError, match="^AnyAngle: " + msg):
            aa.paths(bad)
    for bad, msg in [(2, r"k = 2 is outside \[0, 2\)"), (-1, "k = -1 is outside"), ([0], "k holds 1 set indices for 2 targets"), ([0, 2], r"k\[1\] = 2 is outside"),
                     (1.5, "k must be None, a set index or one per target")]:
        with pytest.raises(ValueError, match="^AnyAngle: " + msg):
            aa.paths([(0, 0), (19, 19)], bad)
    for bad in (2, -1, 0.5, True):
        with pytest.raises(ValueError, match="^AnyAngle: b = .* is outside"):
            aa.map(bad)
    with pytest.raises(ValueError, match="^AnyAngle: 1 lengths for 2 targets"):
        aa.gap([30.0], [(0, 0), (19, 19)])
    with pytest.raises(ValueError, match="^AnyAngle: lengths must be numbers"):
        aa.gap(["x", None], [(0, 0), (19, 19)])
    with pytest.raises(ValueError, match="^AnyAngle: k = 2 is outside"):
        aa.gap([30.0], [(19, 19)], 2)
    assert aa.paths([]) == [] and len(aa.status) == 0 and len(aa.gap([], [])) == 0


def test_calls_that_need_a_field(no_engine):
    a = make(FIG7, engine=ModelEngine(FIG7))
    for call, what in ((lambda: a.map(), "map"), (lambda: a.paths([(0, 0)]), "paths"), (lambda: a.gap([1.0], [(0, 0)]), "gap")):
        with pytest.raises(ValueError, match=f"^AnyAngle: {what} needs a field\\(\\) call before it"):
            call()


def test_closed(no_engine):
    from pathfit import PathfitError
    a = make(FIG7, engine=ModelEngine(FIG7))
    a.close()
    for call in (lambda: a.field([(0, 0)]), lambda: a.adjacency(), lambda: a.refresh(), lambda: a.route((0, 0), (19, 19))):
        with pytest.raises(PathfitError, match="^AnyAngle: the field is closed"):
            call()


# ---- the numpy side over the model engine
def test_the_table_through_the_class(no_engine):
    for name, (dij, smoothed, best, corners) in sc.TABLE.items():
        g, s, t = gio.grid(name)
        S, T = divmod(s, 20), divmod(t, 20)
        a = make(g, engine=ModelEngine(g))
        d = a.field([S])
        assert d.shape == (1, a.M) and abs(d[0, np.searchsorted(a.node_cells, t)] - best) < 5e-12
        m = a.map()
        assert m.shape == (20, 20) and m[S] == 0.0 and m[T] == d[0, np.searchsorted(a.node_cells, t)] and np.all(np.isinf(m[g == 1]))
        p = a.paths([T])[0]
        assert p[0] == S and p[-1] == T and a.lengths[0] == m[T] and a.status[0] == 0 and a.turns[0] >= 1
        back = a.paths([T], 0, reverse=True)[0]
        assert back.tolist() == p.tolist()[::-1]
        gap = a.gap([smoothed, dij, best], [T, T, T])
        assert gap[0] > 0 and gap[1] > gap[0] and abs(gap[2]) < 1e-12 and abs(gap[0] - (smoothed / best - 1)) < 1e-12
        c = make(g, "corners", also=[S, T], engine=ModelEngine(g))
        assert abs(c.field([S])[0, np.searchsorted(c.node_cells, t)] - corners) < 5e-12
        r = c.route(S, T)
        assert r[0] == S and r[-1] == T and abs(c.lengths[0] - corners) < 5e-12 and c.lengths[0] >= a.lengths[0]


def test_sets_unreachable_targets_and_refresh(no_engine):
    g = np.zeros((6, 8), np.uint8)
    g[:, 4] = 1
    g[2, 4] = 0                                                      # a wall with a door
    e = ModelEngine(g)
    a = make(g, also=[(0, 4)], engine=e)                             # a node on the wall: kept, isolated
    assert a.graph_info[3] == 1 and a.M == 44
    d = a.field([[(0, 0), (5, 0)], (0, 7), [(0, 4)]])
    assert d.shape == (3, 44) and list(a.info[:, 1]) == [2, 1, 0] and list(a.info[:, 0]) == [43, 43, 0] and np.all(np.isinf(d[2]))
    ps = a.paths([(5, 7), (5, 7), (0, 4), (0, 0)], [0, 1, 0, 2])
    assert list(a.status) == [0, 0, 2, 2] and len(ps[2]) == 0 and len(ps[3]) == 0 and np.isinf(a.lengths[2]) and a.lengths[1] == 5.0
    assert (2, 4) in ps[0].tolist() or len(ps[0]) >= 3
    before = a.lengths[0]
    shut = g.copy()
    shut[2, 4] = 1
    e.update_grid(shut)
    a.refresh()
    assert list(a.info[:, 0]) == [24, 18, 0] and a.graph_info[3] == 1 + 1      # the door's cell is a node on an obstacle now
    a.paths([(5, 7)], 0)
    assert list(a.status) == [2] and a.gap([before], [(5, 7)])[0] == -1.0   # (finite / inf - 1)
    assert np.isnan(a.gap([np.inf], [(5, 7)])[0]) and a.gap([7.0], [(5, 7)])[0] == -1.0
