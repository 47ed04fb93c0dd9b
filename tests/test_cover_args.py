"""Coverage argument checks: every ValueError before any device is touched, and the numpy side (the chunks, `keep`, the perturbation
stream and its dropped draws, incumbent replacement and its tie rule, history, coverage_of, seen_by / unique, map, exposure, field,
refresh, solve_masks) over a model engine whose pf_cover_pack and pf_cover_improve are the checkers' (runs on a CPU-only host)."""
import numpy as np
import pytest

import cost_checkers as cost_ck
import cover_checkers as cc
import field_checkers as fc
import golden_io as gio
import visibility_checkers as vc
from test_assign_args import HostBuf
from test_assign_args import ModelEngine as FieldModelEngine


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import cover

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(cover, "Engine", boom)


class Buf(HostBuf):
    def read(self, elem_offset, count):
        return self.a[int(elem_offset):int(elem_offset) + int(count)].copy()


class ModelEngine(FieldModelEngine):
    """The field calls of the assignment tests' model engine, pf_visibility_field as the integer model, pf_cover_pack in numpy and
    pf_cover_improve as the checkers' literal loop; `improves` logs (m, n, p, fixed, B, shared, max_moves, the start rows) per call,
    `packs` (kind, K, n, ld, radius, row0).  `script`: keys to answer with instead, one list of (covered, open) per call."""

    def __init__(self, g, script=None):
        super().__init__(g)
        self.improves, self.packs = [], []
        self.script = script

    def buf(self, shape, dtype):
        return Buf(shape, dtype)

    def put(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype)
        return Buf(a.shape if a.ndim else (1,), a.dtype).upload(a)

    def dist_field_batch(self, ids, d_out, ad, rs):
        assert ad is True
        super().dist_field_batch(ids, d_out, ad, rs)

    def visibility_field(self, ids, d_seen, restrict=True, max_range_sq=-1, d_info=None):
        self.calls.append("visibility_field")
        self.rows_asked.append(len(ids))
        occ = vc.occ_of(self.grid_u8)
        rows = np.array([vc.seen_map(occ, (int(s) // self.C, int(s) % self.C), bool(restrict), int(max_range_sq)) for s in ids], np.uint8).reshape(-1)
        d_seen.a[:len(rows)] = rows

    def cover_pack(self, kind, K, n, d_src, ld, d_targets, radius, row0, d_mask):
        self.calls.append("cover_pack")
        self.packs.append((kind, K, n, ld, radius, row0))
        assert d_src.a.dtype == (np.uint8 if kind == 0 else np.float64) and d_targets.a.dtype == np.int32 and d_mask.a.dtype == np.uint64
        src = d_src.a[:K * ld].reshape(K, ld)[:, d_targets.a[:n]]
        d_mask.a.reshape(-1, cc.words_of(n))[row0:row0 + K] = cc.pack(src != 0 if kind == 0 else src <= radius)

    def cover_improve(self, m, n, p, fixed, B, shared, d_mask, max_moves, d_sel, d_covered, d_value, d_status, d_info=None):
        self.calls.append("cover_improve")
        W = cc.words_of(n)
        masks = d_mask.a.reshape(-1, m, W)
        assert len(masks) == (1 if shared else B) and cc.first_bad_tail(masks, n) is None and cc.first_bad_row(d_sel.a, m, p, fixed) is None
        rows = d_sel.a.reshape(B, p).copy()
        self.improves.append((m, n, p, fixed, B, bool(shared), max_moves, rows))
        for b in range(B):
            M = masks[0 if shared else b]
            row, covered, v, st, info = cc.improve(cc.sets_of(cc.unpack(M, n)), n, rows[b], fixed, max_moves)
            if self.script is not None:
                cov, opn = self.script[len(self.improves) - 1][b]
                row, v = list(rows[b]), (cov, opn, v[2], v[3])
                covered = cc.planes(M, row)[0]
            d_sel.a[b * p:(b + 1) * p] = row
            if d_covered is not None:
                d_covered.a[b * W:(b + 1) * W] = covered
            d_value.a[4 * b:4 * b + 4] = v
            d_status.a[b] = st
            if d_info is not None:
                d_info.a[4 * b:4 * b + 4] = info


def fig7():
    return gio.grid("fig7")[0]


def make(g, sites, *a, **kw):
    from pathfit import Coverage
    return Coverage(g, sites, *a, **kw)


def reach_bits(g, sites, targets, radius, rs=True):
    mm = fc.move_masks(np.asarray(g, np.uint8), True, rs)
    C = g.shape[1]
    fields = np.array([fc.reference_dijkstra(np.asarray(g, np.uint8), mm, r * C + c)[0] for r, c in sites]).reshape(len(sites), -1)
    return fields[:, [r * C + c for r, c in targets]] <= radius


CELLS = cc.map_cells(fig7())
S9, T40 = CELLS[5::33], CELLS[2::7][:40]                              # 9 candidate sites, 40 targets


# ---- every ValueError, before the device
def test_grid_engine_and_by(no_engine):
    with pytest.raises(ValueError, match="^Coverage: grid must be 2-D"):
        make(np.zeros(16, int), [(0, 0)])

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^Coverage: the engine's grid has another shape"):
        make(fig7(), [(0, 0)], engine=Other())
    for bad in ("see", "", 0, None):
        with pytest.raises(ValueError, match="^Coverage: by must be 'sight' or 'reach'"):
            make(fig7(), S9, by=bad)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(fig7(), S9, 3)


def test_sites_targets_and_count(no_engine):
    g = np.zeros((70, 70), int)
    cells = [(r, c) for r in range(70) for c in range(70)]
    with pytest.raises(ValueError, match="^Coverage: sites is empty"):
        make(g, [])
    with pytest.raises(ValueError, match="^Coverage: targets is empty"):
        make(g, [(0, 0)], targets=[])
    with pytest.raises(ValueError, match="^Coverage: targets is empty"):
        make(np.ones((3, 3), int), [(0, 0)])                          # no free cell
    with pytest.raises(ValueError, match="^Coverage: sites must be a list"):
        make(g, 5)
    with pytest.raises(ValueError, match="^Coverage: targets must be a list"):
        make(g, [(0, 0)], targets=5)
    with pytest.raises(ValueError, match=r"^Coverage: targets\[1\] = \(70, 0\) is outside the 70x70 grid"):
        make(g, [(0, 0)], targets=[(0, 0), (70, 0)])
    with pytest.raises(ValueError, match=r"^Coverage: sites\[0\] must be an \(r, c\) pair"):
        make(g, [7])
    with pytest.raises(ValueError, match="^Coverage: 1025 sites; at most 1024 are searched"):
        make(g, cells[:1025], 2)
    with pytest.raises(ValueError, match="^Coverage: 1100000 targets; at most 1048576 are covered"):
        make(np.zeros((1100, 1000), np.uint8), [(0, 0)])              # every free cell of a large map
    for bad in (0, 4, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match=r"^Coverage: count must be an integer in \[1, 3\]"):
            make(g, cells[:3], bad)
    with pytest.raises(ValueError, match=r"^Coverage: count must be an integer in \[1, 64\]"):
        make(g, cells[:100], 65)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, cells[:1024], None, targets=cells[:4096])


def test_keep(no_engine):
    g = fig7()
    with pytest.raises(ValueError, match="^Coverage: keep must be a list"):
        make(g, S9, 3, keep=4)
    for bad in ([9], [-1], [1.5], ["a"], [True]):
        with pytest.raises(ValueError, match=r"^Coverage: keep\[0\] = .* is outside \[0, 9\)"):
            make(g, S9, 3, keep=bad)
    with pytest.raises(ValueError, match="^Coverage: keep names a site twice"):
        make(g, S9, 3, keep=[2, 2])
    with pytest.raises(ValueError, match="^Coverage: keep holds 4 sites, more than count = 3"):
        make(g, S9, 3, keep=[0, 1, 2, 3])
    for good in ([], [8], (0, 1, 2), np.array([4, 5])):
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, S9, 3, keep=good)


def test_range_radius_and_cost(no_engine):
    g = fig7()
    for bad in (-1, float("inf"), float("nan"), "far", True):
        with pytest.raises(ValueError, match="^Coverage: max_range must be None or a finite number >= 0"):
            make(g, S9, 3, max_range=bad)
    with pytest.raises(ValueError, match="^Coverage: radius and cost belong to by='reach'"):
        make(g, S9, 3, radius=3.0)
    with pytest.raises(ValueError, match="^Coverage: radius and cost belong to by='reach'"):
        make(g, S9, 3, cost=np.ones((20, 20)))
    with pytest.raises(ValueError, match="^Coverage: max_range belongs to by='sight'"):
        make(g, S9, 3, by="reach", radius=3.0, max_range=4)
    for bad in (None, -0.5, float("inf"), float("nan"), "3", True, [1]):
        with pytest.raises(ValueError, match="^Coverage: radius must be a finite number >= 0"):
            make(g, S9, 3, by="reach", radius=bad)
    with pytest.raises(ValueError, match="^Coverage: cost has shape"):
        make(g, S9, 3, by="reach", radius=3.0, cost=np.ones((20, 19)))
    c = np.ones((20, 20))
    c[tuple(np.argwhere(g != 1)[3])] = 0.5
    with pytest.raises(ValueError, match="^Coverage: cost"):
        make(g, S9, 3, by="reach", radius=3.0, cost=c)
    for kw in (dict(max_range=0), dict(max_range=7.5), dict(by="reach", radius=0), dict(by="reach", radius=np.float64(2.5), cost=np.ones((20, 20)))):
        with pytest.raises(AssertionError, match="the device was touched"):
            make(g, S9, 3, **kw)


def test_starts_rounds_seed_and_max_moves(no_engine):
    g = fig7()
    for name, bad in (("starts", (0, -1, 1.5, "8", True, None, (1 << 16) + 1)), ("rounds", (-1, 2.0, None, True)), ("seed", (-1, 0.5, None, "x")),
                      ("max_moves", (-1, (1 << 20) + 1, 3.0, True))):
        for v in bad:
            with pytest.raises(ValueError, match=f"^Coverage: {name} must be an integer in "):
                make(g, S9, 3, **{name: v})
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, S9, 3, starts=1, rounds=0, seed=np.int64(5), max_moves=0)


def test_solve_masks_errors():
    from pathfit import Coverage
    e = ModelEngine(fig7())
    sm = Coverage.solve_masks
    z = np.zeros((2, 3, 2), np.uint64)
    for bad in (np.zeros((2, 3, 4, 5), np.uint64), np.zeros((2, 3, 2), np.int64), np.zeros((2, 3, 2)), np.zeros((0, 2), np.uint64), [[1, 2]]):
        with pytest.raises(ValueError, match="^Coverage: masks must be a uint64 array"):
            sm(e, bad, [[0]], 100)
    for bad in (0, (1 << 20) + 1, 100.0, None):
        with pytest.raises(ValueError, match=r"^Coverage: n must be an integer in \[1, 1048576\]"):
            sm(e, z, [[0], [1]], bad)
    with pytest.raises(ValueError, match="^Coverage: masks holds 2 words a row, n = 129 needs 3"):
        sm(e, z, [[0], [1]], 129)
    with pytest.raises(ValueError, match="^Coverage: 1025 sites; at most 1024"):
        sm(e, np.zeros((1, 1025, 1), np.uint64), [[0]], 10)
    with pytest.raises(ValueError, match="^Coverage: shared=True takes one"):
        sm(e, z, [[0], [1]], 100, shared=True)
    with pytest.raises(ValueError, match="^Coverage: max_moves must be an integer"):
        sm(e, z, [[0], [1]], 100, max_moves=-1)
    with pytest.raises(ValueError, match=r"^Coverage: fixed must be an integer in \[0, 2\]"):
        sm(e, z, [[0, 1], [1, 2]], 100, fixed=3)
    with pytest.raises(ValueError, match=r"^Coverage: count must be an integer in \[1, 3\]"):
        sm(e, z[:1], [[0, 1, 2, -1]], 100)
    for rows in ([[0, 1]] * 3, [[0.0, 1.0]] * 2, "abc", [[[0]]] * 2):
        with pytest.raises(ValueError, match="^Coverage: rows must be an integer array"):
            sm(e, z, rows, 100)
    bad = np.array([cc.pack(cc.bits(0.3, 4, 70, b)) for b in range(3)])
    bad[2, 1, 1] |= np.uint64(1) << np.uint64(6)
    bad[1, 3, 1] |= np.uint64(1) << np.uint64(63)
    with pytest.raises(ValueError, match=r"^Coverage: masks\[1, 3\] holds a bit at an element >= n = 70"):
        sm(e, bad, [[0, 1]] * 3, 70)
    a = np.array([cc.pack(cc.bits(0.3, 5, 70, b)) for b in range(3)])
    for rows, fixed, at in (([[0, 1], [2, 2], [0, 1]], 0, r"\[1, 1\] = 2"), ([[0, 1], [2, 3], [0, 5]], 0, r"\[2, 1\] = 5"), ([[0, -2], [2, 3], [0, 1]], 0, r"\[0, 1\] = -2"),
                            ([[0, 1], [-1, 3], [0, 1]], 1, r"\[1, 0\] = -1")):
        with pytest.raises(ValueError, match=rf"^Coverage: rows{at}: a start holds sites"):
            sm(e, a, rows, 70, fixed=fixed)
    assert e.calls == []


# ---- the numpy side over the model engine
def test_the_facade_over_the_model():
    g = fig7()
    e = ModelEngine(g)
    search = dict(starts=4, rounds=3, seed=5)
    t = make(g, S9, 3, targets=T40, keep=[6], engine=e, **search)
    m, n, p = 9, 40, 3
    bits = cc.sight_bits(g, S9, T40)
    M = cc.pack(bits)
    assert e.calls == ["visibility_field", "cover_pack"] + ["cover_improve"] * 4 and e.packs == [(0, 9, 40, 400, 0.0, 0)]
    assert np.array_equal(t.masks, M) and t.max_moves == 48 and t.count == 3 and t.words == 1
    # the calls: the kept row alone, then the rounds' perturbations of the incumbent, all over the one shared mask set
    assert [c[:7] for c in e.improves] == [(m, n, p, 1, 1, True, 48)] + [(m, n, p, 1, 4, True, 48)] * 3
    assert e.improves[0][7].tolist() == [[6, -1, -1]]
    S = cc.sets_of(bits)
    rng = np.random.default_rng(5)
    best = cc.improve(S, n, [6, -1, -1], 1, 48)
    for call in e.improves[1:]:
        assert call[7].tolist() == cc.perturbations(rng, best[0], 1, m, 4)
        for row in call[7]:
            got = cc.improve(S, n, row, 1, 48)
            if cc.key_of_result(got, n) < cc.key_of_result(best, n):
                best = got
    want = cc.search(M, n, p, keep=(6,), **search)
    assert list(t.row) == want["row"] == best[0] and t.row[0] == 6 and t.sites == [v for v in t.row if v >= 0] and t.cells == [S9[v] for v in t.sites]
    assert (t.covered, t.moves, t.drops, t.history) == (want["count"], want["moves"], want["drops"], want["history"]) and len(t.history) == 4
    assert t.coverage == t.covered / 40 and t.complete == (t.covered == 40) and np.array_equal(t.mask, cc.unpack(want["covered"], n))
    # seen_by and unique come from the open rows only
    assert np.array_equal(t.seen_by, bits[t.sites].sum(0)) and t.seen_by.dtype == np.int32
    assert t.unique == [[j for j in range(n) if bits[s, j] and t.seen_by[j] == 1] for s in t.sites] and sum(len(u) for u in t.unique) == want["unique"]
    shown = t.map()
    assert shown.shape == (20, 20) and shown.dtype == bool and int(shown.sum()) == t.covered and all(shown[T40[j]] == t.mask[j] for j in range(n))
    # coverage_of: any other set, on the host
    assert t.coverage_of(t.sites) == t.covered and t.coverage_of([]) == 0 and t.coverage_of([0, 4]) == int((bits[0] | bits[4]).sum())
    assert t.coverage_of(range(9)) == int(bits.any(0).sum())
    with pytest.raises(ValueError, match=r"^Coverage: sites\[1\] = 9 is outside \[0, 9\)"):
        t.coverage_of([0, 9])
    with pytest.raises(ValueError, match="^Coverage: sites names a site twice"):
        t.coverage_of([1, 1])
    with pytest.raises(ValueError, match="^Coverage: sites must be a sequence"):
        t.coverage_of(3)
    with pytest.raises(ValueError, match="^Coverage: field\\(\\) belongs to by='reach'"):
        t.field()
    t.close()


def test_targets_none_count_none_and_the_range():
    g = fig7()
    e = ModelEngine(g)
    t = make(g, S9, max_range=6.5, restrict_diagonal_near_obstacle=False, starts=2, rounds=1, engine=e)
    assert t.targets == CELLS and t.n == 290 and t.count == 9 and t.max_moves == 144 and t.range_sq == 42 and t.words == 5
    bits = cc.sight_bits(g, S9, CELLS, strict=False, max_range_sq=42)
    want = cc.search(cc.pack(bits), 290, 9, starts=2, rounds=1)
    assert np.array_equal(t.masks, cc.pack(bits)) and list(t.row) == want["row"] and t.history == want["history"] and t.covered == want["count"]
    assert cc.first_bad_tail(t.masks, 290) is None


def test_reach_with_and_without_a_cost_map_and_refresh():
    g = fig7()
    e = ModelEngine(g)
    t = make(g, S9, 4, targets=T40, by="reach", radius=7.0, starts=3, rounds=1, engine=e)
    assert e.calls == ["dist_field_batch", "cover_pack", "cover_improve", "cover_improve"] and e.packs == [(1, 9, 40, 400, 7.0, 0)]
    bits = reach_bits(g, S9, T40, 7.0)
    assert np.array_equal(t.masks, cc.pack(bits)) and list(t.row) == cc.search(cc.pack(bits), 40, 4, starts=3, rounds=1)["row"]
    with pytest.raises(ValueError, match="^Coverage: exposure\\(\\) belongs to by='sight'"):
        t.exposure()
    with pytest.raises(ValueError, match="^Coverage: refresh\\(cost\\) needs a coverage built with a cost map"):
        t.refresh(cost=np.ones((20, 20)))

    from pathfit import nearest_field

    class Seen(Exception):
        pass

    def fake(grid, sets, ad, rs, engine=None):
        raise Seen(sets, ad, rs, engine)
    real = nearest_field.NearestSourceField
    nearest_field.NearestSourceField = fake
    try:
        with pytest.raises(Seen) as got:
            t.field()
        assert got.value.args == ([t.cells], True, True, e)
    finally:
        nearest_field.NearestSourceField = real
    # a door closes: refresh recomputes on the engine's map
    g2 = g.copy()
    g2[g2 > 1] = 0
    for r, c in [tuple(c) for c in np.argwhere(g2 == 0) if tuple(c) not in S9 + T40][:25]:
        g2[r, c] = 1
    e.update_grid(g2)
    t.refresh()
    bits2 = reach_bits(g2, S9, T40, 7.0)
    assert not np.array_equal(bits, bits2) and np.array_equal(t.masks, cc.pack(bits2)) and t.covered == cc.search(cc.pack(bits2), 40, 4, starts=3, rounds=1)["count"]
    # under a cost map the fields are pf_cost_field's, single-source sets
    e = ModelEngine(g)
    cost = cost_ck.cost_of_kind("u50", g.shape, 3)
    C = g.shape[1]
    u = make(g, S9[:4], 2, targets=T40[:12], by="reach", radius=20.0, cost=cost, starts=2, rounds=1, engine=e)
    assert e.calls == ["cost_field", "cover_pack", "cover_improve", "cover_improve"]
    want = cost_ck.fields(g, cost, [[r * C + c] for r, c in S9[:4]], True, True)[0].reshape(4, -1)[:, [r * C + c for r, c in T40[:12]]] <= 20.0
    assert np.array_equal(u.masks, cc.pack(want)) and 0 < want.sum() < want.size
    with pytest.raises(ValueError, match="^Coverage: field\\(\\) belongs to by='reach' without a cost map"):
        u.field()


def test_exposure_is_visibilitys_of_the_open_cells():
    from pathfit import visibility
    g = fig7()
    e = ModelEngine(g)
    t = make(g, S9, 2, targets=T40, max_range=9, starts=2, rounds=1, engine=e)
    asked = []

    class Fake:
        def __init__(self, grid, strict, engine=None):
            asked.append((strict, engine))

        def exposure(self, cells, max_range):
            asked.append((cells, max_range))
            return np.zeros((20, 20), np.int32)

        def close(self):
            asked.append("closed")
    real = visibility.Visibility
    visibility.Visibility = Fake
    try:
        assert t.exposure().shape == (20, 20)
    finally:
        visibility.Visibility = real
    assert asked == [(True, e), (t.cells, 9), "closed"]


def test_dropped_draws_and_the_stream():
    """Placement's perturbation stream, unchanged: one draw a round, a draw whose site is in the row is dropped."""
    from pathfit import cover, placement
    assert cover.perturbations is placement.perturbations
    rng = np.random.default_rng(11)
    draws = np.random.default_rng(11).integers(0, [8, 12], (6, 2, 2))          # Q = (p - f) // 4 = 2 draws a start
    row = [3, 7, 0, 1, 2, 4, 5, 6, 8, -1]
    rows = cover.perturbations(rng, row, 2, 12, 6)
    assert rows == cc.perturbations(np.random.default_rng(11), row, 2, 12, 6)
    dropped = 0
    for s in range(6):
        want = list(row)
        for slot, site in draws[s]:
            if int(site) in want:
                dropped += 1
            else:
                want[2 + int(slot)] = int(site)
        assert rows[s] == want and rows[s][:2] == [3, 7] and cc.valid_row(rows[s], 12, 10, 2)
    assert dropped > 0
    twin = np.random.default_rng(11)
    twin.integers(0, [8, 12], (6, 2, 2))
    assert rng.integers(0, 1 << 30) == twin.integers(0, 1 << 30)      # one draw a round, whatever was dropped


def test_the_incumbent_is_replaced_by_a_strictly_smaller_key_at_the_smallest_index():
    g = fig7()
    script = [[(20, 3)], [(20, 3), (19, 1), (20, 2)], [(25, 3), (30, 3), (30, 3)], [(30, 3), (30, 2), (29, 1)], [(30, 2), (30, 3), (12, 0)]]
    e = ModelEngine(g, script)
    t = make(g, S9, 3, targets=T40, starts=3, rounds=4, engine=e)
    assert t.history == [(20, 3), (20, 2), (10, 3), (10, 2), (10, 2)] and t.covered == 30 and len(t.history) == 5
    rows = [c[7] for c in e.improves]                                 # (the scripted answers keep the start rows)
    rng = np.random.default_rng(0)
    incumbents = [rows[0][0], rows[1][2], rows[2][1], rows[3][1]]     # fewer sites at equal coverage win; of two equal keys the first; coverage comes first
    for call, inc in zip(rows[1:], incumbents):
        assert call.tolist() == cc.perturbations(rng, [int(v) for v in inc], 0, 9, 3)
    assert list(t.row) == list(rows[3][1])


def test_every_slot_kept_and_one_site():
    g = fig7()
    e = ModelEngine(g)
    t = make(g, S9, 2, targets=T40, keep=[4, 1], rounds=3, engine=e)
    assert t.history == [t.history[0]] and e.calls.count("cover_improve") == 1 and t.moves == 0 and list(t.row) == [4, 1]
    assert e.improves[0][:7] == (9, 40, 2, 2, 1, True, 32)
    one = make(g, S9[:1], targets=S9[:1], rounds=1, starts=2, engine=ModelEngine(g))
    assert one.sites == [0] and one.complete and one.count == 1 and one.unique == [[0]] and len(one.history) == 2


def test_the_chunks():
    from pathfit import Coverage
    g = fig7()
    for by, kw, unit, call in (("sight", {}, 1, "visibility_field"), ("reach", dict(radius=6.0), 8, "dist_field_batch")):
        whole = make(g, S9[:7], 3, targets=T40, by=by, starts=3, rounds=1, engine=ModelEngine(g), **kw)

        class Small(Coverage):
            CHUNK_BYTES = 3 * 400 * unit
        e = ModelEngine(g)
        t = Small(g, S9[:7], 3, targets=T40, by=by, starts=3, rounds=1, engine=e, **kw)
        assert t.chunk == 3 and whole.chunk == 7 and e.rows_asked == [3, 3, 1]
        assert e.calls == [call, "cover_pack"] * 3 + ["cover_improve"] * 2 and [x[1] for x in e.packs] == [3, 3, 1] and [x[5] for x in e.packs] == [0, 3, 6]
        assert np.array_equal(t.masks, whole.masks) and list(t.row) == list(whole.row) and t.history == whole.history
    assert Coverage.CHUNK_BYTES == 256 << 20


def test_a_target_nobody_sees():
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    g[:, 15] = 1
    e = ModelEngine(g)
    t = make(g, [(4, 2), (0, 12), (8, 3)], targets=[(0, 0), (8, 14), (4, 18), (3, 3)], engine=e)
    assert not t.complete and t.covered == 3 and not t.mask[2] and t.seen_by[2] == 0 and len(t.sites) == 2 and t.count == 3 and list(t.row).count(-1) == 1
    assert t.coverage == 0.75 and sorted(t.sites)[-1] == 1


def test_solve_masks_over_the_model():
    from pathfit import Coverage
    from pathfit.cover import pack_bits, unpack_bits
    e = ModelEngine(fig7())
    bits = np.array([cc.bits(d, 6, 90, 1) for d in cc.DENSITIES + (0.4,)])
    masks = pack_bits(bits)
    assert np.array_equal(masks, cc.pack(bits)) and np.array_equal(unpack_bits(masks, 90), bits)
    rows = [[2, -1, -1], [2, 0, 5], [2, -1, 4], [2, 1, -1]]
    out = Coverage.solve_masks(e, masks, rows, 90, fixed=1)
    assert e.improves[-1][:7] == (6, 90, 3, 1, 4, False, 48) and e.improves[-1][7].tolist() == rows
    assert out.row.shape == (4, 3) and out.covered.shape == (4, 2) and out.value.shape == (4, 4) and out.info.shape == (4, 4)
    for b in range(4):
        assert cc.same((out.row[b], out.covered[b], out.value[b], out.status[b], out.info[b]), cc.improve_numpy(masks[b], 90, rows[b], 1, 48))
    Coverage.solve_masks(e, masks[0], [[-1, -1]] * 5, 90, shared=True, max_moves=1)
    assert e.improves[-1][:7] == (6, 90, 2, 0, 5, True, 1)
    one = Coverage.solve_masks(e, masks[0], [0, 1, 2], 90)
    assert one.row.shape == (1, 3) and e.improves[-1][:7] == (6, 90, 3, 0, 1, False, 48)


def nothing_covered_map():
    """A wall between the sites and the targets: nothing is seen, and nothing lies within a radius of 1."""
    g = np.zeros((5, 9), np.uint8)
    g[:, 4] = 1
    return g, [(0, 0), (1, 1)], [(0, 8), (4, 8)]


@pytest.mark.parametrize("by,kw", [("reach", dict(radius=1.0)), ("sight", {})])
def test_no_site_covers_anything_and_every_slot_ends_empty(by, kw):
    g, sites, targets = nothing_covered_map()
    e = ModelEngine(g)
    t = make(g, sites, targets=targets, by=by, starts=2, rounds=1, engine=e, **kw)
    assert not t.masks.any() and list(t.row) == [-1, -1] and t.sites == [] and t.cells == [] and t.unique == []
    assert t.covered == 0 and t.coverage == 0.0 and not t.complete and not t.mask.any() and t.mask.shape == (2,)
    assert t.seen_by.tolist() == [0, 0] and t.seen_by.dtype == np.int32 and not t.map().any() and t.history == [(2, 0), (2, 0)]
    assert t.moves == t.drops == 2                                    # round 1 puts a site into each start; it covers nothing and is dropped
    assert t.coverage_of([]) == 0 and t.coverage_of([0, 1]) == 0
    if by == "sight":
        assert t.exposure().shape == (5, 9) and not t.exposure().any() and "visibility_count" not in e.calls
    t.refresh()
    assert t.sites == [] and t.covered == 0
    kept = make(g, sites, targets=targets, by=by, keep=[1], starts=2, rounds=1, engine=ModelEngine(g), **kw)   # a kept site that covers nothing stays
    assert kept.sites == [1] and kept.covered == 0 and kept.unique == [[]] and kept.seen_by.tolist() == [0, 0]


def test_a_failed_construction_frees_its_buffers():
    g, sites, targets = nothing_covered_map()
    freed = []

    class Tracked(Buf):
        def free(self):
            freed.append(self)

    class Failing(ModelEngine):
        def buf(self, shape, dtype):
            return Tracked(shape, dtype)

        def put(self, arr, dtype=None):
            a = np.ascontiguousarray(arr, dtype)
            return Tracked(a.shape if a.ndim else (1,), a.dtype).upload(a)

        def cover_pack(self, *a):
            raise RuntimeError("the pack failed")
    with pytest.raises(RuntimeError, match="the pack failed"):
        make(g, sites, targets=targets, by="reach", radius=1.0, engine=Failing(g))
    assert len(freed) == 3                                            # the source rows, the targets and the masks
