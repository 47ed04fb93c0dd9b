"""Cost-field repair (pf_cost_field_repair) per (map, policy, cost map, change): the kernel ms and the work counters of one repair of
one field from one source, against pf_cost_field from nothing on the same handle and the same new map.

    python scripts/probe_cost_repair.py [--maps g256,up2,up4] [--policies "1,1"] [--costs ones,margin4] [--reps 5] [--json OUT]

Every map gets a wall along its middle row with two doors, the westernmost and the easternmost column that joins the source's side to
the far corner's (walled); the source is the first free cell (north-west).  The changes, each from the map as built:
  near    one cell next to the source closes
  far     one cell next to the last free cell (south-east) closes
  door-   the west door closes: everything south of the wall is reached by the east door only, a long detour
  door+   the west door opens again (from the map with the door closed)
  mix16   16 seeded cells toggle between free and obstacle
Per row, after one untimed run of both, `reps` repeats alternating in one process on one handle, median (min ... max): the rows of the
old map are copied back (device to device, untimed), then
  repair   pf_cost_field_repair with d_info: pf_last_kernel_ms (HIP events round the whole call: the validation kernel, both phases
           with the host's queue-length reads, the info kernels) and pf_cost_field_work's launches / tile visits / words lowered /
           words raised (the first three depend on the schedule)
  fresh    pf_cost_field from nothing with d_info on the new map, kernel ms, launches / tile visits
and the two rows and infos must be bit-equal (asserted).  Cost maps: ones (c == 1), margin4 (Clearance.cost_map(margin=4) of the OLD
map, kept for the new one; a cell that opens costs 1)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from probe_clearance import clear_map  # noqa: E402
from probe_dist_field import med  # noqa: E402


def walled(g):
    """The map with the two-door wall -> (grid, the west door's cell).  A door may stand in the columns where the cell north of the wall
    is reached from the first free cell and the cell south of it from the last one, both by straight moves alone with the wall shut
    (two fields on the device): the westernmost and the easternmost such column."""
    import pathfit
    g = np.array(g, np.uint8)
    R, C = g.shape
    g[R // 2, :] = 1
    free = np.flatnonzero(g.reshape(-1) != 1)
    e = pathfit.Engine(g)
    ones, out = e.put(np.ones(g.size)), e.buf(2 * g.size, np.float64)
    e.cost_field(ones, [0, 1, 2], [int(free[0]), int(free[-1])], out, 0, 1, None)
    D = out.download().reshape(2, R, C)
    ones.free()
    out.free()
    e.close()
    ok = np.flatnonzero(np.isfinite(D[0, R // 2 - 1]) & np.isfinite(D[1, R // 2 + 1]))
    if len(ok) < 2:
        raise SystemExit("no two columns for the doors")
    g[R // 2, ok[0]] = g[R // 2, ok[-1]] = 0
    return g, (R // 2) * C + int(ok[0])


def free_neighbour(g, v):
    R, C = g.shape
    r, c = divmod(int(v), C)
    for dr, dc in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)):
        if 0 <= r + dr < R and 0 <= c + dc < C and g[r + dr, c + dc] != 1:
            return (r + dr) * C + c + dc
    raise SystemExit("the cell has no free neighbour")


def changes_of(g, door, src):
    def closed(*cells):
        out = g.copy()
        out.reshape(-1)[list(cells)] = 1
        return out
    last = int(np.flatnonzero(g.reshape(-1) != 1)[-1])
    mix = g.copy()
    pick = np.random.default_rng(g.size).choice(np.setdiff1d(np.arange(g.size), [src]), 16, replace=False)
    mix.reshape(-1)[pick] = np.where(mix.reshape(-1)[pick] == 1, 0, 1)
    shut = closed(door)
    return [("near", g, closed(free_neighbour(g, src))), ("far", g, closed(free_neighbour(g, last))), ("door-", g, shut), ("door+", shut, g),
            ("mix16", g, mix)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="g256,up2,up4")
    ap.add_argument("--policies", default="1,1")
    ap.add_argument("--costs", default="ones,margin4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    policies = [tuple(int(v) for v in p.split(",")) for p in a.policies.split(";")]
    rows = []
    print("| map | policy | cost map | change | repair, kernel ms | launches / tile visits / words lowered / words raised | fresh, kernel ms | "
          "fresh launches / tile visits | repair / fresh |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g, door = walled(clear_map(name))
        R, C = g.shape
        RC = g.size
        src = int(np.flatnonzero(g.reshape(-1) != 1)[0])
        e = pathfit.Engine(g)
        cl = pathfit.Clearance(g, engine=e)
        costs = {c: np.ascontiguousarray(np.ones(g.shape) if c == "ones" else cl.cost_map(margin=float(c[6:])), np.float64) for c in a.costs.split(",")}
        cl.close()
        off, ids = np.array([0, 1], np.int32), np.array([src], np.int32)
        dcost, old, out, ref = e.buf(RC, np.float64), e.buf(RC, np.float64), e.buf(RC, np.float64), e.buf(RC, np.float64)
        info, rinfo = e.buf(4, np.int64), e.buf(4, np.int64)
        for ad, rs in policies:
            for cname, cost in costs.items():
                for change, g0, g1 in changes_of(g, door, src):
                    c1 = np.where((g0 == 1) & (g1 != 1), 1.0, cost)
                    changed = np.flatnonzero((g0.reshape(-1) == 1) != (g1.reshape(-1) == 1)).astype(np.int32)
                    e.update_grid(g0)
                    dcost.upload(cost.reshape(-1))
                    e.cost_field(dcost, off, ids, old, ad, rs, None)
                    e.update_grid(g1)
                    dcost.upload(c1.reshape(-1))

                    def repair():
                        out.copy_from(0, old, 0, RC)
                        e.cost_field_repair(dcost, changed, off, ids, out, ad, rs, info)
                        return e.last_kernel_ms(), e.cost_field_work()

                    def fresh():
                        e.cost_field(dcost, off, ids, ref, ad, rs, rinfo)
                        return e.last_kernel_ms(), e.cost_field_work()

                    repair(), fresh()                                 # untimed: code objects, scratch
                    P, W, F, V = [], [], [], []
                    for _ in range(a.reps):
                        ms, work = repair()
                        P.append(ms)
                        W.append(work)
                        ms, work = fresh()
                        F.append(ms)
                        V.append(work)
                        assert np.array_equal(out.download().view(np.uint64), ref.download().view(np.uint64)), (name, ad, rs, cname, change, "rows differ")
                        assert np.array_equal(info.download(), rinfo.download()), (name, ad, rs, cname, change, "infos differ")
                    wk = " / ".join(f"{int(np.median([w[i] for w in W]))}" for i in range(4))
                    vk = " / ".join(f"{int(np.median([w[i] for w in V]))}" for i in range(2))
                    rows.append(dict(map=name, shape=[R, C], policy=[ad, rs], cost=cname, change=change, repair_ms=P, repair_work=[list(w) for w in W],
                                     fresh_ms=F, fresh_work=[list(w) for w in V]))
                    print(f"| {name} {R}x{C} | {ad},{rs} | {cname} | {change} | {med(P)} | {wk} | {med(F)} | {vk} | {np.median(P) / np.median(F):.2f} |", flush=True)
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
