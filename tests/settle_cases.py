"""Cases for the rare paths of the parallel closed-set engine (pf_settle.h), and the program that runs them against one build of the library.

    PF_LIB=maaco-path-planing_amd/lib/stress/libpathfit_<variant>.so python tests/settle_cases.py <variant|default>

The engine certifies its own answer or hands the search back to the sequential loop; comparing final paths alone never shows which of
the two happened.  The stress variants (build.py: SETTLE_VARIANTS) compile the shipped engine under a band geometry that makes its rare
branches -- bands larger than a trip, full buckets, pushes beyond the band range, a full touched list, two nodes per lane -- common, and
count them (-DPF_OPEN_PATHS, pf_selftest_settle_paths).  Maps and pairs are those of tests/open_list_cases.py.  Every search runs with
the engine forced on (astar_settle 1) and is compared with the CPU oracle, path cell for cell and status; the same batch then runs with
the engine off on the same handle (what a hand-back left in the slot must not matter).  Engine.counters() is checked against the number
of searches that reach the engine, derived on the CPU, in every build; the branch counters, where compiled in, against each other.
One JSON line comes out; the exit status is non-zero on any mismatch.

tests/test_settle_cases.py checks the cases and the CPU facts the assertions rest on; tests/test_gpu_settle_stress.py runs this program once
per build, each in a fresh child process."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

import open_list_cases as olc                  # (puts the package, the oracle and tests/ on sys.path)

# the order of pf_settle.h's ST_* (the ABI of pf_selftest_settle_paths)
COUNTERS = ["wipe", "trips", "take_one", "take_many", "take_part", "superseded", "stop_bound", "stop_empty", "back_bucket", "back_range",
            "back_touched", "back_winners", "back", "unreached", "all_regular", "irregular", "cone_goal", "cone_ancestor", "cone_queue",
            "cone_ok", "row_short"]
VARIANT_NAMES = ["st_cap4", "st_q1", "st_q96", "st_touch", "st_wide2"]
# the engine's geometry per build (pf_settle.h's defaults, and what build.py's rows change)
SHIPPED = dict(Q=64.0, WIDE=1, CAP=1024, NBK=256, TOUCH=(2, 1))
GEOMETRY = {"default": {}, "st_cap4": dict(CAP=4), "st_q1": dict(Q=1.0), "st_q96": dict(Q=96.0), "st_touch": dict(TOUCH=(1, 4)),
            "st_wide2": dict(WIDE=2, Q=1.0)}
CLOSED = (0, 2)                    # the closed-set variants: AStarSolver.solve, DijkstraSolver.solve
WIPE_LAUNCHES = 160                # one-search launches on slot 0: the label epoch runs out after 126 searches of the engine
FIT_CASES = 12
CANARY = -7777


def geometry(name):
    return dict(SHIPPED, **GEOMETRY[name])


def astar_runs(name):
    """The launches of one map: (variant, allow_diag, restrict_corner)."""
    pol = olc.POLICIES if name == "blocks128" else olc.POLICIES[:1]
    return [(v, ad, rs) for v in CLOSED for ad, rs in pol]


def reaches_engine(o, flat, s, t, av, path, variant):
    """Does the search s -> t get as far as the engine?  pf_astar.h answers beforehand: an endpoint on an obstacle, start == target,
    another component (no path without the avoid set either), and a pocket of at most FLOOD_CELLS cells around either endpoint (a
    failing closed-set search pops the start's whole side once: the oracle's pops are that side's cells)."""
    if flat[s] == 1 or flat[t] == 1 or s == t:
        return False
    if len(path):
        return True
    if av is None or not len(o.astar(s, t, None, variant)[0]):
        return False
    return min(o.astar(s, t, av, 0)[1][0], o.astar(t, s, av, 0)[1][0]) > olc.FLOOD_CELLS


def decode_reached(o, flat, start, target, wps):
    """The searches of one chained decode that reach the engine (ga_solver.py:63-76: the avoid set is the cells visited so far; a
    waypoint on an obstacle answers the whole decode before its first search, pf_decode.h)."""
    if any(flat[w] == 1 for w in wps):
        return 0
    seen = np.zeros(flat.size, np.uint8)
    seen[start] = 1
    cur, n = int(start), 0
    for goal in [int(w) for w in wps] + [int(target)]:
        p, _ = o.astar(cur, goal, seen, 0)
        n += reaches_engine(o, flat, cur, goal, seen, p, 0)
        if not len(p):
            break
        seen[p] = 1
        cur = goal
    return n


def fit_cases(ref, variant):
    """FIT_CASES pairs of blocks128 whose path has more than two cells, with their avoid sets."""
    s, t, av = ref.pairs("blocks128")
    res = ref.astar("blocks128", variant)
    idx = [i for i in range(len(s)) if len(res[i][0]) > 2][:FIT_CASES]
    return [(int(s[i]), int(t[i]), av[i], res[i][0]) for i in idx]


# ---------------------------------------------------------------------------------------------------------------- the runner
def read_counters(e):
    """The engine's branch counters since the last call (and cleared), or None when the build has none."""
    out = (C.c_int64 * len(COUNTERS))()
    rc = e.L.pf_selftest_settle_paths(e.h, out, len(COUNTERS), 1)
    if rc == 1:
        assert not any(out) and b"not compiled in" in e.L.pf_last_error(e.h)
        return None
    e._ck(rc)
    return dict(zip(COUNTERS, (int(v) for v in out)))


class Family:
    def __init__(self):
        self.d = dict(searches=0, reached=0, settled=0, sequential=0, mismatches=0, seconds=0.0, counters=None)
        self.notes = []

    def bad(self, *what):
        self.d["mismatches"] += 1
        if len(self.notes) < 8:
            self.notes.append(" ".join(str(w) for w in what))

    def account(self, e, tag, n, reached, forced=True, variant=0):
        """One launch's books: Engine.counters() against the searches that reach the engine, the branch counters against both.
        -> (settled, sequential, branch counters or None)."""
        c = e.counters()
        br = read_counters(e)
        st, sq = c["settled_searches"], c["sequential_searches"]
        self.d["searches"] += n
        if not forced:
            if st or sq or (br is not None and any(br.values())):
                self.bad(tag, "the engine ran although it is switched off", st, sq)
            return st, sq, br
        self.d["reached"] += reached; self.d["settled"] += st; self.d["sequential"] += sq
        tot = self.d.setdefault("totals", {}).setdefault(str(variant), [0, 0, 0])      # per closed-set variant: reached, settled, sequential
        tot[0] += reached; tot[1] += st; tot[2] += sq
        if st + sq != reached:
            self.bad(tag, "settled + sequential", st, sq, "searches that reach the engine:", reached)
        if br is not None:
            self.d["counters"] = olc.add_counters(self.d["counters"], br)
            if "by_variant" in self.d:
                self.d["by_variant"][str(variant)] = olc.add_counters(self.d["by_variant"][str(variant)], br)
            cone_back = br["cone_goal"] + br["cone_ancestor"] + br["cone_queue"]
            for what, a, b in (("searches in = loop exits", reached, br["stop_bound"] + br["stop_empty"] + br["back"]),
                               ("trips", br["trips"], br["take_one"] + br["take_many"] + br["take_part"] + br["stop_bound"] + br["stop_empty"]),
                               ("settled", st, br["unreached"] + br["all_regular"] + br["cone_ok"]),
                               ("sequential", sq, br["back"] + cone_back),
                               ("cone walks", br["irregular"], cone_back + br["cone_ok"]),
                               ("irregular nodes under h = 0", br["irregular"] if variant == 2 else 0, 0)):
                if a != b:
                    self.bad(tag, what, a, "!=", b, br)
            reasons = br["back_bucket"] + br["back_range"] + br["back_touched"] + br["back_winners"]
            if not (max(br["back_bucket"], br["back_range"], br["back_touched"], br["back_winners"]) <= br["back"] <= reasons):
                self.bad(tag, "hand-backs and their reasons", br)
        return st, sq, br


def check_paths(fam, tag, paths, st, want):
    for i, p in enumerate(want):
        if not np.array_equal(paths[i], p) or st[i] != (0 if len(p) else 1):
            fam.bad(tag, i, "path / status", st[i], len(paths[i]), len(p))


def run_astar(ref, name_of_build):
    from pathfit.engine import Engine
    fam = Family()
    fam.d["by_variant"] = {str(v): None for v in CLOSED}         # the branch counters of every launch of the family, per closed-set variant
    fam.d["shares"] = {}                                            # map -> variant -> [sequential, reached]
    fam.d["sealed"] = {str(v): dict(searches=0, unreached=0, back=0, settled=0, sequential=0) for v in CLOSED}
    fam.d["short_back_touched"] = 0
    for name, g in ref.maps.items():
        flat = g.reshape(-1)
        e = Engine(g)
        try:
            s, t, av = ref.pairs(name)
            sl = list(olc.SEALED)
            for variant, ad, rs in astar_runs(name):
                o = ref.oracle(name, ad, rs)
                res = ref.astar(name, variant, ad, rs)
                want = [p for p, _ in res]
                reached = sum(reaches_engine(o, flat, int(s[i]), int(t[i]), av[i], want[i], variant) for i in range(len(s)))
                kw = dict(path_cap=e.R * e.C, allow_diag=bool(ad), restrict_corner=bool(rs))
                tag = (name, variant, ad, rs)
                e.set_option("astar_settle", 1)
                paths, st = e.astar_host(variant, s, t, av, **kw)
                check_paths(fam, tag + ("forced",), paths, st, want)
                sd, sq, br = fam.account(e, tag, len(s), reached, variant=variant)
                if (ad, rs) == (1, 1):
                    fam.d["shares"].setdefault(name, {})[str(variant)] = [sq, reached]
                # the sealed pairs on their own: nothing answers them beforehand, every one leaves the engine by its own "never
                # reached" exit unless the main loop handed it back
                paths, st = e.astar_host(variant, s[sl], t[sl], [av[i] for i in sl], **kw)
                check_paths(fam, tag + ("sealed",), paths, st, [want[i] for i in sl])
                if any(len(want[i]) for i in sl):
                    fam.bad(tag, "a sealed pair has a path")
                r_sl = sum(reaches_engine(o, flat, int(s[i]), int(t[i]), av[i], want[i], variant) for i in sl)
                if r_sl != len(sl):
                    fam.bad(tag, "a sealed pair is answered before the engine")
                sd, sq, br = fam.account(e, tag + ("sealed",), len(sl), r_sl, variant=variant)
                z = fam.d["sealed"][str(variant)]
                z["searches"] += len(sl); z["settled"] += sd; z["sequential"] += sq
                if br is not None:
                    z["unreached"] += br["unreached"]; z["back"] += br["back"]
                    if br["unreached"] + br["back"] != len(sl) or sq != br["back"]:
                        fam.bad(tag, "sealed pairs: unreached + handed back", br["unreached"], br["back"], "of", len(sl))
                # the same batch on the sequential loop of the same handle, after whatever the hand-backs left behind
                e.set_option("astar_settle", 0)
                paths, st = e.astar_host(variant, s, t, av, **kw)
                check_paths(fam, tag + ("sequential after",), paths, st, want)
                fam.account(e, tag + ("off",), len(s), 0, forced=False)
            # searches a few cells long: no geometry here makes their touched list overflow
            o = ref.oracle(name)
            ss, tt = olc.short_pairs(g)
            e.set_option("astar_settle", 1)
            for variant in CLOSED:
                want = [o.astar(int(a), int(b), None, variant)[0] for a, b in zip(ss, tt)]
                paths, st = e.astar_host(variant, ss, tt, None, path_cap=e.R * e.C)
                check_paths(fam, (name, variant, "short"), paths, st, want)
                reached = sum(reaches_engine(o, flat, int(a), int(b), None, p, variant) for a, b, p in zip(ss, tt, want))
                _, _, br = fam.account(e, (name, variant, "short"), len(ss), reached, variant=variant)
                fam.d["short_back_touched"] += br["back_touched"] if br is not None else 0
            if name == "rooms64":
                # one-search launches land on slot 0: its label epoch runs out on the way and the label array is wiped
                before = e.slot_state(0)[2]
                falls = 0
                for k in range(WIPE_LAUNCHES):
                    i, variant = k % len(ss), CLOSED[(k // len(ss)) % 2]
                    want = [o.astar(int(ss[i]), int(tt[i]), None, variant)[0]]
                    paths, st = e.astar_host(variant, ss[i:i + 1], tt[i:i + 1], None, path_cap=e.R * e.C)
                    check_paths(fam, (name, variant, "wipe", k), paths, st, want)
                    fam.account(e, (name, variant, "wipe", k), 1, int(reaches_engine(o, flat, int(ss[i]), int(tt[i]), None, want[0], variant)), variant=variant)
                    ep = e.slot_state(0)[2]
                    falls += ep < before
                    before = ep
                if falls != 1:
                    fam.bad(name, "label epoch wipes on slot 0:", falls)
                fam.d["epoch_falls"] = falls
        finally:
            e.set_option("astar_settle", -1)
            e.close()
    return fam


def run_decode(ref, name_of_build):
    from pathfit.engine import Engine, score_params
    fam = Family()
    g = ref.maps["blocks128"]
    flat = g.reshape(-1)
    d = ref.decodes()
    o = ref.oracle("blocks128")
    sp = score_params(0, True, *olc.SCORE)
    e = Engine(g)
    try:
        cap = g.size + 6
        n = len(d["wp"])
        for tag, call, want, wstats, ends in (
                ("one", lambda: e.decode_host(0, g.size - 1, wp_cells=d["wp"], sp=sp, path_cap=cap), d["one"], d["one_stats"],
                 [(0, g.size - 1, d["wp"][i]) for i in range(n)]),
                ("multi", lambda: e.decode_multi_host(d["ms"], d["mt"], wp_cells=d["wpm"], sp=sp, path_cap=cap), d["multi"], d["multi_stats"],
                 [(int(d["ms"][i]), int(d["mt"][i]), d["wpm"][i]) for i in range(n)])):
            reached = sum(decode_reached(o, flat, a, b, w) for a, b, w in ends)
            for settle in (1, 0):
                e.set_option("astar_settle", settle)
                paths, st, stats = call()
                for i in range(len(want)):
                    if not np.array_equal(paths[i], want[i]) or st[i] != (0 if len(want[i]) else 1) or stats[i].tobytes() != wstats[i].tobytes():
                        fam.bad(tag, settle, i, "cells / status / stats", st[i], len(paths[i]), len(want[i]))
                fam.account(e, (tag, settle), len(want), reached, forced=bool(settle))
    finally:
        e.set_option("astar_settle", -1)
        e.close()
    return fam


class Rows:
    """n output rows of `cap` cells with a guard row before and after, and the same for the length and status columns."""

    def __init__(self, e, n, cap):
        self.n, self.cap = n, cap
        self.cells = e.put(np.full((n + 2, cap), CANARY, np.int32))
        self.len = e.put(np.full(n + 2, CANARY, np.int32))
        self.status = e.put(np.full(n + 2, CANARY, np.int32))

    def ptrs(self):
        return self.cells.at(self.cap), self.len.at(1), self.status.at(1)

    def read(self):
        """-> (cells [n][cap], len [n], status [n], the guards still hold the canary)."""
        c, l, s = self.cells.download(), self.len.download(), self.status.download()
        ok = all((a[0] == CANARY).all() and (a[-1] == CANARY).all() for a in (c, l, s))
        return c[1:-1], l[1:-1], s[1:-1], ok


def run_exact_fit(ref, name_of_build):
    """Rows of exactly L cells and of L - 1 cells with the engine forced on: the path whole, or status 3, length 0 and one overflowed
    agent; the case sits between two one-cell paths (start == target) and guard rows, which keep their canaries."""
    from pathfit.engine import Engine
    fam = Family()
    g = ref.maps["blocks128"]
    e = Engine(g)
    try:
        e.set_option("astar_settle", 1)
        for variant in CLOSED:
            for s, t, av, want in fit_cases(ref, variant):
                L = len(want)
                ds, dt = e.put(np.array([s, s, t], np.int32)), e.put(np.array([s, t, t], np.int32))
                na = len(av) if av is not None else 0
                doff, dav = e.put(np.array([0, 0, na, na], np.int64)), e.put(av if na else np.zeros(1, np.int32))
                for cap in (L, L - 1):
                    rows = Rows(e, 3, cap)
                    pc, pl, ps = rows.ptrs()
                    e._ck(e.L.pf_astar_batch(e.h, variant, 1, 1, 3, ds.ptr, dt.ptr, doff.ptr, dav.ptr, cap, pc, pl, ps, None))
                    c, l, st, guards = rows.read()
                    tag = (variant, s, t, "cap", cap, "L", L)
                    if not guards:
                        fam.bad(tag, "a guard row was written")
                    for a, cell in ((0, s), (2, t)):
                        if st[a] != 0 or l[a] != 1 or c[a, 0] != cell or (c[a, 1:] != CANARY).any():
                            fam.bad(tag, "neighbour row", a)
                    if cap == L:
                        if st[1] != 0 or l[1] != L or not np.array_equal(c[1, :L], want):
                            fam.bad(tag, "the path that fits", st[1], l[1])
                    elif st[1] != 3 or l[1] != 0:
                        fam.bad(tag, "the path that does not fit", st[1], l[1])
                    if e.counters()["overflow_agents"] != (0 if cap == L else 1):
                        fam.bad(tag, "overflow_agents", e.counters()["overflow_agents"])
                    fam.account(e, tag, 3, 1, variant=variant)
    finally:
        e.set_option("astar_settle", -1)
        e.close()
    return fam


def main(variant):
    from pathfit import _lib
    if variant not in VARIANT_NAMES + ["default"]:
        raise SystemExit("usage: PF_LIB=... python tests/settle_cases.py <%s|default>" % "|".join(VARIANT_NAMES))
    t0 = time.time()
    ref = olc.Reference.get()
    out = dict(variant=variant, lib=os.path.basename(_lib.so_path()), families={}, mismatches=0, notes=[], counters=None)
    for fname, fn in (("astar", run_astar), ("decode", run_decode), ("exact_fit", run_exact_fit)):
        t1 = time.time()
        fam = fn(ref, variant)
        fam.d["seconds"] = round(time.time() - t1, 2)
        out["families"][fname] = fam.d
        out["mismatches"] += fam.d["mismatches"]
        out["notes"] += fam.notes
        out["counters"] = olc.add_counters(out["counters"], fam.d["counters"])
    if (out["counters"] is None) != (variant == "default"):
        out["mismatches"] += 1; out["notes"].append("branch counters: compiled in = %s in build %s" % (out["counters"] is not None, variant))
    out["seconds"] = round(time.time() - t0, 2)
    print(json.dumps(out, default=int), flush=True)
    return 1 if out["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else ""))
