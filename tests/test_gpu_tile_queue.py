"""The host half of the tile-queue engine (pathfit_fields.hip: tile_call, tile_rounds, tile_finish): pf_clearance_widest,
pf_turn_field and pf_cost_field lay ONE scratch block of the handle out anew on every call, for their own B and under two tile geometries
(64 x 16 for the widest and cost fields, 32 x 16 for the turn fields).  Interleaved calls on one Engine must give, bit for bit, what the
same call gives on a fresh Engine and what the CPU models give (tests/widest_checkers.py, tests/cost_checkers.py, tests/turn_checkers.py,
as the three fields' own GPU tests use them); the work words stay each entry point's own, a refused call leaves no trace, and the small
device-to-host copies are counted as one per launch plus the seed's and the counters' (plus one per cost-map validation).  Every
output lies between canary words."""
import functools
import re

import numpy as np
import pytest

import cost_checkers as ck
import turn_checkers as tk
import widest_checkers as wc

pytestmark = pytest.mark.gpu

CANARY = -77
PAD = 64
WT = 0.3                                                             # the turn weight


def big_map():
    """33 x 65: 3 x 2 tiles of 64 x 16 and 3 x 3 tiles of 32 x 16, the last tile row and column one cell wide in both geometries;
    wall segments across the tile borders at rows 16 and 32 and columns 32 and 64."""
    g = np.zeros((33, 65), np.uint8)
    g[10, 20:46] = 1                                                  # across column 32
    g[5:29, 50] = 1                                                   # across row 16
    g[14:19, 8] = 1
    g[24, 55:65] = 1                                                  # across column 64
    g[31:33, 30:35] = 1                                               # across row 32 and column 32
    return g, dict(free=(3 * 65 + 3, 20 * 65 + 40), wall=10 * 65 + 25)


def small_map():
    """5 x 7: one tile in both geometries."""
    g = np.zeros((5, 7), np.uint8)
    g[2, 3] = 1
    return g, dict(free=(1 * 7 + 1, 3 * 7 + 5), wall=2 * 7 + 3)


MAPS = {"33x65": big_map, "5x7": small_map}


def sets_of(g, cells):
    s0, s1 = cells["free"]
    twice, on_wall, corners = [s0, s0], [cells["wall"], s1], [0, g.size - 1]   # listed twice; on an obstacle (d2 == 0); opposite corner tiles
    assert g.reshape(-1)[cells["wall"]] == 1 and not g.reshape(-1)[[s0, s1, 0, g.size - 1]].any()
    return twice, on_wall, corners


def between_canaries(e, n, dtype):
    return e.put(np.full(n + 2 * PAD, CANARY, dtype))


def inner(buf, tag):
    a = buf.download()
    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), tag
    return a[PAD:len(a) - PAD]


def view(e, buf, n, dtype):
    from pathfit.engine import _View
    return _View(e, buf.at(PAD), n, dtype)


def same(a, b):
    """bit for bit (the doubles as their words)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


class Handle:
    """An Engine on a map with the clearance field and a cost map in HBM."""

    def __init__(self, g, cost):
        from pathfit.engine import Engine
        self.g, self.e = g, Engine(g)
        self.dfield, self.dcost = self.e.buf(g.size, np.int32), self.e.put(np.ascontiguousarray(cost, np.float64).reshape(-1))
        self.e.clearance_field(self.dfield)
        self.d2 = self.dfield.download().reshape(g.shape)

    def call(self, kind, sets, ad, rs, cost=True):
        """One raw call of kind "widest" / "turn" / "cost", every output between canaries -> (the outputs with the info rows last, the
        work words, the small copies the call made).  A refused call raises after the outputs were seen untouched."""
        from pathfit._lib import PathfitError
        e, B, RC = self.e, len(sets), self.g.size
        off, src = ck.csr(sets)
        shapes = {"widest": [(B * RC, np.int32)], "cost": [(B * RC, np.float64)], "turn": [(8 * B * RC, np.float64), (B * RC, np.float64)]}[kind] + [(4 * B, np.int64)]
        bufs = [between_canaries(e, n, dt) for n, dt in shapes]
        try:
            v = [view(e, b, n, dt) for b, (n, dt) in zip(bufs, shapes)]
            before = e.d2h_counts()[0]
            try:
                if kind == "widest":
                    e.clearance_widest(self.dfield, off, src, v[0], ad, rs, v[1])
                elif kind == "cost":
                    e.cost_field(self.dcost, off, src, v[0], ad, rs, v[1])
                else:
                    e.turn_field(self.dcost if cost else None, WT, off, src, v[0], v[1], ad, rs, v[2])
            except PathfitError:
                assert all(np.all(inner(b, kind) == CANARY) for b in bufs), kind     # a refused call leaves every output untouched
                raise
            copies = e.d2h_counts()[0] - before
            work = {"widest": e.clearance_widest_work, "cost": e.cost_field_work, "turn": e.turn_field_work}[kind]()
            assert e.last_kernel_ms() > 0 and work[3] == 0 and work[0] <= work[1]
            return [inner(b, kind) for b in bufs], work, copies
        finally:
            for b in bufs:
                b.free()

    def close(self):
        self.e.close()


@functools.lru_cache(maxsize=None)
def case(name, ad, rs):
    """The six calls of the sequence on one map and policy with what the CPU models give for each, computed once.  The widest model
    wants the clearance field: the device's (pf_clearance_field has its own tests), read from a handle of its own."""
    g, cells = MAPS[name]()
    cost = ck.cost_of_kind("u50", g.shape, 11)
    twice, on_wall, corners = sets_of(g, cells)
    three = [twice, on_wall, corners]
    h = Handle(g, cost)
    d2 = h.d2
    h.close()
    calls = [("widest", [corners], True), ("turn", three, True), ("cost", three, True), ("widest", three, True), ("turn", [twice], False), ("cost", [on_wall], True)]
    want = []
    for kind, sets, with_cost in calls:
        if kind == "widest":
            w, info = wc.widest(d2, sets, ad, rs)
            want.append([w.reshape(-1), np.asarray(info).reshape(-1)])
        elif kind == "cost":
            D, _, info = ck.fields(g, cost, sets, ad, rs)
            want.append([D.reshape(-1), np.asarray(info).reshape(-1)])
        else:
            T, best, info = tk.fields(g, cost if with_cost else None, sets, WT, ad, rs)
            want.append([T.reshape(-1), best.reshape(-1), np.asarray(info).reshape(-1)])
    return g, cost, calls, want


def copies_expected(kind, with_cost, work):
    """one small copy per launch, the seed's queue length and the counters; one more for a validated cost map"""
    return work[0] + 2 + (1 if kind == "cost" or (kind == "turn" and with_cost) else 0)


def check_call(h, kind, sets, with_cost, ad, rs, want, tag):
    out, work, copies = h.call(kind, sets, ad, rs, with_cost)
    assert len(out) == len(want) and all(same(a, b) for a, b in zip(out, want)), (tag, kind, len(sets), [int((np.asarray(a) != np.asarray(b)).sum()) for a, b in zip(out, want)])
    assert copies == copies_expected(kind, with_cost, work), (tag, kind, copies, work)
    return out, work


@pytest.mark.parametrize("ad, rs", [(1, 1), (0, 0)])
@pytest.mark.parametrize("name", list(MAPS))
def test_interleaved_calls_on_one_handle(name, ad, rs):
    g, cost, calls, want = case(name, ad, rs)
    h = Handle(g, cost)
    try:
        last = {}
        for i, ((kind, sets, with_cost), w) in enumerate(zip(calls, want)):
            out, last[kind] = check_call(h, kind, sets, with_cost, ad, rs, w, (name, i))                 # against the CPU model
            fresh = Handle(g, cost)
            try:
                alone = fresh.call(kind, sets, ad, rs, with_cost)[0]                                     # against a fresh handle
            finally:
                fresh.close()
            assert all(same(a, b) for a, b in zip(out, alone)), (name, i, kind)
        # each entry point keeps the work words of its own last call
        e = h.e
        assert (e.clearance_widest_work(), e.turn_field_work(), e.cost_field_work()) == (last["widest"], last["turn"], last["cost"])
        assert last["widest"][0] >= 1 and last["turn"][0] >= 1 and last["cost"][0] >= 1
    finally:
        h.close()


@pytest.mark.parametrize("ad, rs", [(1, 1), (0, 0)])
def test_a_refused_call_in_the_sequence(ad, rs):
    from pathfit._lib import PathfitError
    g, cost, calls, want = case("33x65", ad, rs)
    where = 20 * 65 + 12                                              # a free cell of the second tile row
    assert g.reshape(-1)[where] == 0
    h = Handle(g, cost)
    try:
        check_call(h, *calls[1], ad, rs, want[1], "turn, B = 3")
        widest_work = check_call(h, *calls[3], ad, rs, want[3], "widest, B = 3")[1]
        bad = cost.copy()
        bad.reshape(-1)[where] = np.nan
        h.dcost.upload(bad.reshape(-1))
        message = re.escape(f"pf_cost_field: bad arguments (the cost of the free cell ({where // 65}, {where % 65}) is not a finite number in [1, 2^20])")
        with pytest.raises(PathfitError, match=message):
            h.call("cost", calls[2][1], ad, rs)                       # (sees the canary-filled outputs untouched before it raises again)
        assert h.e.cost_field_work() == (0, 0, 0, 0) and h.e.clearance_widest_work() == widest_work
        check_call(h, *calls[4], ad, rs, want[4], "turn without a map, after the refusal")
        check_call(h, *calls[3], ad, rs, want[3], "widest, after the refusal")
        h.dcost.upload(cost.reshape(-1))
        check_call(h, *calls[2], ad, rs, want[2], "cost, after the refusal")
    finally:
        h.close()
