"""Cases for the rare paths of the A* open list (pf_astar_sw.h), and the program that runs them against one build of the library.

    PF_LIB=maaco-path-planing_amd/lib/stress/libpathfit_<variant>.so python tests/open_list_cases.py <variant|default>

The stress variants (build.py: VARIANTS) compile the shipped pop loop under a bucket geometry that makes its rare branches -- full
buckets, the spill list, refills of buckets larger than the window, window evictions -- common, and count them (-DPF_OPEN_PATHS).
The cases are the smallest at which the open list leaves its 64-lane window and its buckets; every search is compared with the CPU
oracle: paths, statuses, per-search pops and pushes; decodes and MPA runs bit for bit.  One JSON line comes out (per-family counts,
mismatches, spilled entries, the largest open list, the branch counters, seconds); the exit status is non-zero on any mismatch.

tests/test_open_list_cases.py checks the cases themselves on the CPU; tests/test_gpu_open_list_stress.py runs this program once per
variant, each in a fresh child process."""
import json
import os
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (os.path.join(_ROOT, "maaco-path-planing_amd"), os.path.join(_ROOT, "oracle"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# the order of pf_astar_sw.h's OP_* (the ABI of pf_selftest_open_paths)
COUNTERS = ["front_append", "spill_full", "spill_range", "spill_list_full", "win_plain", "win_shift", "win_evict", "front_le64",
            "front_gt64", "refill_one", "refill_many", "big_merge", "big_select", "spill_only", "spill_only_moved", "refill_ret4",
            "respill", "respill_stayed", "respill_offered", "early_refill", "rotated"]
VARIANT_NAMES = ["cap8", "wide64", "wide256", "spill256"]
WINDOW, HEADS = 64, 8              # an open list of more than 64 + 8 entries cannot live in the window alone
N_PAIRS = 48
MAP_NAMES = ["empty96", "blocks128", "sparse128", "rooms64", "g256"]
SEALED = range(40, 48)             # pairs an avoid wall separates (see pairs)
FLOOD_CELLS = 512                  # pf_astar.h PF_FLOOD_K: a pocket of at most this many cells is proven sealed without a search
POLICIES = [(1, 1), (1, 0), (0, 1)]    # (allow_diag, restrict_corner): the default, corner cutting, 4-connected
SCORE = (0.3, 0.8, 1.8, 100.0)         # w_turn, w_safe, min_safe, diag_pen of the decodes
MPA_KW = dict(num_predators=32, num_iterations=6, FADs_rate=0.5, seed=4)
TAG_LIMIT, AVOID_LIMIT = 0xFFFFFF - 2 * 0x8000, 0x3FF0   # a clean slot's solve tag / avoid epoch lie in [1, limit)


# ---------------------------------------------------------------------------------------------------------------- the maps
def maps():
    """name -> uint8 grid (1 = obstacle; the blocks map carries the start / target markers 2 / 3 in its corners)."""
    import golden_io as gio
    from pathfit import env
    out = {"empty96": np.zeros((96, 96), np.uint8),
           "blocks128": np.ascontiguousarray(env.random_blocks(128, 128, 0.25, seed=11, block=(2, 9)), np.uint8),
           "sparse128": (np.random.default_rng(8).random((128, 128)) < 0.08).astype(np.uint8)}
    g = (np.random.default_rng(9).random((64, 64)) < 0.08).astype(np.uint8)
    g[16:46, 18] = 1; g[16:46, 47] = 1; g[16, 18:48] = 1; g[45, 18:48] = 1           # a sealed 28 x 28 room
    out["rooms64"] = g
    out["g256"] = gio.grid("g256")[0]
    return out


def in_room(cells):
    r, c = np.asarray(cells) // 64, np.asarray(cells) % 64
    return (r > 16) & (r < 45) & (c > 18) & (c < 47)


def _cheb(a, b, C):
    return max(abs(a // C - b // C), abs(a % C - b % C))


def pairs(name, g, o):
    """48 (start, target, avoid set) of one map: corner to corner both ways, start == target, adjacent cells, an endpoint on an
    obstacle, and far pairs (at least a third of the map apart: their open lists outgrow the window); on the rooms map a third
    has one endpoint in the sealed room.  Avoid sets as scripts/soak_parity.py builds them: none, random, path-shaped, small.
    The pairs SEALED lie in one component, on either side of an avoid set that is a whole column or row of the map, a quarter in:
    both sides hold more than FLOOD_CELLS cells, so nothing proves the answer beforehand and the pop loop has to pop the start's
    whole side -- window, buckets and spill list drained to empty -- before it returns "no path"."""
    rnd = np.random.default_rng(1000 + sum(map(ord, name)))
    R, C = g.shape
    flat = g.reshape(-1)
    free, obst = np.flatnonzero(flat != 1), np.flatnonzero(flat == 1)
    n = N_PAIRS
    starts, targets = np.zeros(n, np.int32), np.zeros(n, np.int32)
    i = 0
    while i < n:
        s, t = (int(v) for v in rnd.choice(free, 2))
        if _cheb(s, t, C) >= max(R, C) // 3:
            starts[i], targets[i] = s, t
            i += 1
    starts[0], targets[0] = free[0], free[-1]
    starts[1], targets[1] = free[-1], free[0]
    targets[2:4] = starts[2:4]
    for i in (4, 5):                                          # a free neighbour of the start (8-neighbourhood)
        r, c = divmod(int(starts[i]), C)
        nb = [(r + dr) * C + c + dc for dr in (-1, 0, 1) for dc in (-1, 0, 1)
              if (dr or dc) and 0 <= r + dr < R and 0 <= c + dc < C and flat[(r + dr) * C + c + dc] != 1]
        targets[i] = nb[int(rnd.integers(len(nb)))] if nb else starts[i]
    if len(obst):
        targets[6] = obst[int(rnd.integers(len(obst)))]
        starts[7] = obst[int(rnd.integers(len(obst)))]
    if name == "rooms64":
        inside, outside = free[in_room(free)], free[~in_room(free)]
        for i in range(8, 24):
            a, b = int(rnd.choice(inside)), int(rnd.choice(outside))
            starts[i], targets[i] = (a, b) if i % 2 else (b, a)
    avoid = []
    for i in range(n):
        k = i % 4
        if k == 0 or i < 8:
            avoid.append(None)
        elif k == 1:
            avoid.append(rnd.choice(free, int(rnd.integers(1, 120))).astype(np.int32))
        elif k == 2:                                          # a path-like avoid set (as MPA / GA build them)
            p, _ = o.astar(int(starts[i]), int(rnd.choice(free)), None, 1)
            avoid.append(p[:-1].astype(np.int32) if len(p) > 1 else None)
        else:
            avoid.append(rnd.choice(free, 8).astype(np.int32))
    for i in SEALED:
        col = i % 2 == 0                                      # the wall: column C // 4, or row R // 4
        w = (C if col else R) // 4
        side = (free % C if col else free // C)
        wall = free[side == w].astype(np.int32)
        small, large = free[side < w], free[side > w]
        while True:
            a, b = int(rnd.choice(small)), int(rnd.choice(large))
            a, b = (a, b) if i % 4 < 2 else (b, a)            # the start's side: the small one, or the large one
            if len(o.astar(a, b, None, 0)[0]) and min(o.astar(a, b, wall, 0)[1][0], o.astar(b, a, wall, 0)[1][0]) > FLOOD_CELLS:
                break
        starts[i], targets[i], avoid[i] = a, b, wall
    return starts, targets, avoid


def short_pairs(g):
    """48 searches whose open lists stay small (endpoints at most 4 cells apart): the batch that must fit after an overflow."""
    rnd = np.random.default_rng(77)
    R, C = g.shape
    free = np.flatnonzero(g.reshape(-1) != 1)
    starts = rnd.choice(free, N_PAIRS).astype(np.int32)
    targets = starts.copy()
    for i, s in enumerate(starts):
        near = [c for c in free[np.abs(free // C - s // C) <= 4] if abs(c % C - s % C) <= 4]
        targets[i] = near[int(rnd.integers(len(near)))]
    return starts, targets


def astar_runs(name):
    """The launches of one map: (variant, allow_diag, restrict_corner, astar_settle, plateau_kernels).  astar_settle 0: the pop
    loop's pop / push counts are the reference's; one extra pass per closed-set variant under the default engine policy (-1)."""
    pol = POLICIES if name == "blocks128" else POLICIES[:1]
    plat = (0, 1) if name == "empty96" else (-1,)
    runs = [(v, ad, rs, 0, pk) for v in (0, 1, 2) for ad, rs in pol for pk in plat]
    return runs + [(v, 1, 1, -1, -1) for v in (0, 2)]


def golden_g256(variant):
    """(starts, targets, avoid, paths, pops, pushes) of the reference's own answers on g256 (tests/golden/astar_cases.npz)."""
    import golden_io as gio
    z = gio.load("astar_cases")
    gid = [str(s) for s in z["grid_names"]].index("g256")
    idx = [i for i in range(len(z["start"])) if z["grid_id"][i] == gid and z["variant"][i] == variant]
    avoid = [gio.csr_get(z["avoid_off"], z["avoid"], i) if z["has_avoid"][i] else None for i in idx]
    return (z["start"][idx].astype(np.int32), z["target"][idx].astype(np.int32), avoid,
            [gio.csr_get(z["path_off"], z["path"], i) for i in idx], z["pops"][idx], z["pushes"][idx])


def decode_cases(g):
    """64 chromosomes of W = 5 waypoints between the map's corners, and 64 more with endpoints of their own."""
    rnd = np.random.default_rng(21)
    free = np.flatnonzero(g.reshape(-1) != 1)
    wp = rnd.choice(free, (64, 5)).astype(np.int32)
    wpm = rnd.choice(free, (64, 5)).astype(np.int32)
    return wp, wpm, rnd.choice(free, 64).astype(np.int32), rnd.choice(free, 64).astype(np.int32)


class Reference:
    """The oracle's answers, computed once per process and shared."""
    _inst = None

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst

    def __init__(self):
        self.maps = maps()
        self._orc, self._pairs, self._astar, self._dec, self._mpa = {}, {}, {}, None, None

    def oracle(self, name, ad=1, rs=1):
        import pf_oracle as po
        if (name, ad, rs) not in self._orc:
            self._orc[name, ad, rs] = po.Oracle(self.maps[name], ad, rs)
        return self._orc[name, ad, rs]

    def pairs(self, name):
        if name not in self._pairs:
            self._pairs[name] = pairs(name, self.maps[name], self.oracle(name))
        return self._pairs[name]

    def astar(self, name, variant, ad=1, rs=1):
        """-> [(path, stats[6])] of the map's 48 pairs."""
        key = (name, variant, ad, rs)
        if key not in self._astar:
            s, t, av = self.pairs(name)
            o = self.oracle(name, ad, rs)
            self._astar[key] = [o.astar(int(s[i]), int(t[i]), av[i], variant) for i in range(len(s))]
        return self._astar[key]

    def decodes(self):
        if self._dec is None:
            g = self.maps["blocks128"]
            o = self.oracle("blocks128")
            wp, wpm, ms, mt = decode_cases(g)
            sc = lambda p: o.score(p, 0, SCORE[0], SCORE[1], SCORE[2], True, SCORE[3])
            one = [o.decode(0, g.size - 1, wp[i])[0] for i in range(len(wp))]
            multi = [o.decode(int(ms[i]), int(mt[i]), wpm[i])[0] for i in range(len(wpm))]
            self._dec = dict(wp=wp, wpm=wpm, ms=ms, mt=mt, one=one, multi=multi, one_stats=[sc(p) for p in one], multi_stats=[sc(p) for p in multi])
        return self._dec

    def mpa(self):
        if self._mpa is None:
            import pf_loops
            g = self.maps["blocks128"]
            kw = dict(MPA_KW)
            ref = pf_loops.MpaOracle(self.oracle("blocks128"), 0, g.size - 1, kw.pop("num_predators"), kw.pop("num_iterations"), **kw)
            best = ref.solve()
            self._mpa = dict(best=best, pop=[p for p, _ in ref.pop], fit=[s[4] for _, s in ref.pop], curve=list(ref.curve))
        return self._mpa


# ---------------------------------------------------------------------------------------------------------------- the runner
class Family:
    def __init__(self):
        # spilled / max_open: per-search numbers only the A* batch call returns (None: not read back)
        self.d = dict(searches=0, mismatches=0, status3=0, drained=0, pushes=0, spilled=None, max_open=None, seconds=0.0, counters=None)
        self.notes, self.overflowed = [], []

    def bad(self, *what):
        self.d["mismatches"] += 1
        if len(self.notes) < 8:
            self.notes.append(" ".join(str(w) for w in what))


def read_counters(e):
    """The branch counters since the last call (and cleared), or None when the build has none."""
    import ctypes as C
    out = (C.c_int64 * len(COUNTERS))()
    rc = e.L.pf_selftest_open_paths(e.h, out, len(COUNTERS), 1)
    if rc == 1:
        assert not any(out) and b"not compiled in" in e.L.pf_last_error(e.h)
        return None
    e._ck(rc)
    return dict(zip(COUNTERS, (int(v) for v in out)))


def add_counters(a, b):
    return b if a is None else (a if b is None else {k: a[k] + b[k] for k in a})


def check_astar(fam, e, tag, variant, starts, targets, avoid, want, tolerant, counts, searched=(), **kw):
    """One launch against `want` = [(path, pops, pushes, infeasible)] (pops None: not compared).  tolerant (spill256): a search may
    come back status 3 with no path instead, and the device must have counted it in overflow_agents.  -> the statuses.
    Pops and pushes are compared for every search that finds a path of more than one cell and for the failing searches `searched`
    (indices), which nothing can answer without searching.  The other searches without a path are exempt: the engine may prove
    them before the open list exists (an endpoint on an obstacle, another component, MPA's avoided goal, a pocket of at most
    FLOOD_CELLS cells: pf_astar.h), and start == target is answered without a pop."""
    paths, st, cnt = e.astar_host(variant, starts, targets, avoid, path_cap=e.R * e.C, want_counters=True, **kw)
    c = e.counters()
    fam.d["searches"] += len(starts); fam.d["spilled"] += c["candidates"]; fam.d["pushes"] += int(cnt[:, 1].sum())
    fam.d["max_open"] = max(fam.d["max_open"], int(cnt[:, 2].max()))
    n3 = int((st == 3).sum())
    fam.d["status3"] += n3
    if c["overflow_agents"] != n3:
        fam.bad(tag, "overflow_agents", c["overflow_agents"], "status 3:", n3)
    for i, (path, pops, pushes, infeasible) in enumerate(want):
        if st[i] == 3:
            if not tolerant or len(paths[i]):
                fam.bad(tag, i, "status 3")
            continue
        if not np.array_equal(paths[i], path) or (st[i] == 0) != (not infeasible):
            fam.bad(tag, i, "path / status", st[i], len(paths[i]), len(path))
        elif counts and pops is not None and (len(path) > 1 or i in searched) and (cnt[i, 0] != pops or cnt[i, 1] != pushes):
            fam.bad(tag, i, "pops / pushes", cnt[i, 0], cnt[i, 1], "want", pops, pushes)
    return st


def check_facade(fam, e, g, variant, ad, rs, s, t, av):
    """A search that came back status 3 from the batch, asked again through AStarSolver / DijkstraSolver: the facade must raise its
    overflow error, not answer "no path"."""
    import pathfit
    C = g.shape[1]
    marked = np.where(g == 1, 1, 0).astype(np.int64)
    marked.reshape(-1)[s], marked.reshape(-1)[t] = 2, 3
    cls = pathfit.AStarSolver if variant == 0 else pathfit.DijkstraSolver
    f = cls(marked, allow_diagonal_moves=bool(ad), restrict_diagonal_near_obstacle_policy=bool(rs), engine=e)
    try:
        f.solve(nodes_to_avoid=[(int(c) // C, int(c) % C) for c in av] if av is not None else None)
        fam.bad("facade did not raise", variant, s, t)
    except RuntimeError as ex:
        if "overflow" not in str(ex):
            fam.bad("facade:", ex)


def run_astar(ref, tolerant):
    from pathfit.engine import Engine
    fam = Family()
    fam.d["spilled"] = fam.d["max_open"] = 0
    facades = 0
    for name, g in ref.maps.items():
        e = Engine(g)
        try:
            s, t, av = ref.pairs(name)
            any3 = False
            for variant, ad, rs, settle, pk in astar_runs(name):
                e.set_option("astar_settle", settle); e.set_option("plateau_kernels", pk)
                want = [(p, o[0], o[1], o[5] != 0) for p, o in ref.astar(name, variant, ad, rs)]
                # (the settling engine's expansion counts are its own; MPA's variant always runs the pop loop)
                st = check_astar(fam, e, (name, variant, ad, rs, settle, pk), variant, s, t, av, want, tolerant, settle == 0 or variant == 1,
                                 searched=SEALED, allow_diag=bool(ad), restrict_corner=bool(rs))
                fam.d["drained"] += int(sum(st[i] == 1 for i in SEALED))
                any3 |= bool((st == 3).any())
                fam.overflowed += [(name, variant, ad, rs, settle, pk, int(i)) for i in np.flatnonzero(st == 3)]
                if settle == 0 and variant != 1 and (st == 3).any() and facades < 2:      # (MPA's connector has no facade of its own)
                    i = int(np.flatnonzero(st == 3)[0])
                    check_facade(fam, e, g, variant, ad, rs, int(s[i]), int(t[i]), av[i])
                    facades += 1
            e.set_option("astar_settle", 0); e.set_option("plateau_kernels", -1)
            if name == "g256":                                  # the reference's own answers
                for variant in (0, 1):
                    gs, gt, gav, gp, gpops, gpushes = golden_g256(variant)
                    want = [(gp[i], gpops[i], gpushes[i], len(gp[i]) == 0) for i in range(len(gp))]
                    st = check_astar(fam, e, (name, "golden", variant), variant, gs, gt, gav, want, tolerant, True)
                    any3 |= bool((st == 3).any())
            if tolerant and any3:
                # after an overflow: the same slots take a batch that fits, exactly, and their state words are a clean slot's
                ss, tt = short_pairs(g)
                o = ref.oracle(name)
                want = [(p, q[0], q[1], q[5] != 0) for p, q in (o.astar(int(a), int(b), None, 0) for a, b in zip(ss, tt))]
                before = e.slot_state(0)
                check_astar(fam, e, (name, "after overflow"), 0, ss, tt, None, want, False, True)
                tag, ep, _ = e.slot_state(0)
                if not (before[0] < tag < TAG_LIMIT and 1 <= ep < AVOID_LIMIT):
                    fam.bad(name, "slot state", before, (tag, ep))
            fam.d["counters"] = add_counters(fam.d["counters"], read_counters(e))
        finally:
            e.set_option("astar_settle", -1); e.set_option("plateau_kernels", -1)
            e.close()
    if tolerant and not (0 < fam.d["status3"] < fam.d["searches"]):
        fam.bad("spill256: searches of both kinds must occur; status 3:", fam.d["status3"], "of", fam.d["searches"])
    if tolerant and not facades:
        fam.bad("spill256: no overflowed closed-set search to ask the facades again")
    fam.d["overflowed"] = fam.overflowed
    return fam


def run_decode(ref, tolerant):
    from pathfit.engine import Engine, score_params
    from pathfit import solvers
    fam = Family()
    g = ref.maps["blocks128"]
    d = ref.decodes()
    sp = score_params(0, True, *SCORE)
    e = Engine(g)
    try:
        cap = g.size + 6
        for tag, call, want, wstats in (
                ("one", lambda: e.decode_host(0, g.size - 1, wp_cells=d["wp"], sp=sp, path_cap=cap), d["one"], d["one_stats"]),
                ("multi", lambda: e.decode_multi_host(d["ms"], d["mt"], wp_cells=d["wpm"], sp=sp, path_cap=cap), d["multi"], d["multi_stats"])):
            paths, st, stats = call()
            c = e.counters()
            fam.d["searches"] += len(want); fam.d["pushes"] += c["pushes"]
            n3 = int((st == 3).sum())
            fam.d["status3"] += n3
            if c["overflow_agents"] != n3:
                fam.bad(tag, "overflow_agents", c["overflow_agents"], "status 3:", n3)
            for i in range(len(want)):
                if st[i] == 3:
                    if not tolerant or len(paths[i]):
                        fam.bad(tag, i, "status 3")
                elif not np.array_equal(paths[i], want[i]) or stats[i].tobytes() != wstats[i].tobytes():
                    fam.bad(tag, i, "cells / stats")
            if n3:                                              # the facade's route (GA / PSO decode through it) must raise, not answer
                try:
                    solvers.decode_retry(e, 0, g.size - 1, e.R, e.C, wp_cells=d["wp"], sp=sp) if tag == "one" else \
                        solvers.decode_retry(e, d["ms"], d["mt"], e.R, e.C, wp_cells=d["wpm"], sp=sp)
                    fam.bad(tag, "decode_retry did not raise")
                except RuntimeError as ex:
                    if "overflow" not in str(ex):
                        fam.bad(tag, "decode_retry:", ex)
        fam.d["counters"] = read_counters(e)
    finally:
        e.close()
    return fam


def run_mpa(ref, tolerant):
    import pathfit
    fam = Family()
    g = ref.maps["blocks128"]
    want = ref.mpa()
    for look in (-1, 0):                                        # the default look-ahead, then the plain sweep
        m = pathfit.MPA(g, **MPA_KW)
        try:
            m.engine.set_option("mpa_lookahead", look)
            fam.d["searches"] += 1
            try:
                got = m.solve_path_planning()
            except RuntimeError as ex:                           # the facade's capacity-overflow error
                fam.d["status3"] += 1
                if not tolerant or "capacity overflow" not in str(ex):
                    fam.bad("mpa", look, ex)
                continue
            pop = m.population
            if [r * 128 + c for r, c in got[0]] != list(want["best"][0]) or got[5] != want["best"][1][4]:
                fam.bad("mpa", look, "best")
            if m.convergence_curve_data != want["curve"]:
                fam.bad("mpa", look, "curve")
            if len(pop) != len(want["pop"]) or any(not np.array_equal(a["path"].cells, p) or np.float64(a["fitness"]).tobytes() != np.float64(f).tobytes()
                                                   for a, p, f in zip(pop, want["pop"], want["fit"])):
                fam.bad("mpa", look, "population")
        finally:
            m.engine.set_option("mpa_lookahead", -1)
            fam.d["counters"] = add_counters(fam.d["counters"], read_counters(m.engine))
            m.engine.close()
    return fam


def main(variant):
    from pathfit import _lib
    if variant not in VARIANT_NAMES + ["default"]:
        raise SystemExit("usage: PF_LIB=... python tests/open_list_cases.py <%s|default>" % "|".join(VARIANT_NAMES))
    t0 = time.time()
    ref = Reference.get()
    tolerant = variant == "spill256"
    out = dict(variant=variant, lib=os.path.basename(_lib.so_path()), families={}, mismatches=0, notes=[])
    for fname, fn in (("astar", run_astar), ("decode", run_decode), ("mpa", run_mpa)):
        t1 = time.time()
        fam = fn(ref, tolerant)
        fam.d["seconds"] = round(time.time() - t1, 2)
        out["families"][fname] = fam.d
        out["mismatches"] += fam.d["mismatches"]
        out["notes"] += fam.notes
    fams = out["families"].values()
    out["spilled"] = out["families"]["astar"]["spilled"]
    out["max_open"] = out["families"]["astar"]["max_open"]
    out["counters"] = None
    for f in fams:
        out["counters"] = add_counters(out["counters"], f["counters"])
    if (out["counters"] is None) != (variant == "default"):
        out["mismatches"] += 1; out["notes"].append("branch counters: compiled in = %s in build %s" % (out["counters"] is not None, variant))
    out["seconds"] = round(time.time() - t0, 2)
    print(json.dumps(out, default=int), flush=True)
    return 1 if out["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else ""))
