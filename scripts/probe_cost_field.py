"""Cost fields (pf_cost_field) per (map, policy, cost map): the kernel ms and the work counters of one field from one source, against
(a) pf_dist_field_merged on the same handle at cost == 1 and (b) a host heap Dijkstra over the same cost map.

    python scripts/probe_cost_field.py [--maps fig7,g256,up4,open1400,serp255] [--policies "1,1"] [--costs ones,margin4,rand50] [--reps 3]
                                       [--no-host] [--json OUT]

Per (map, policy, cost map), after one untimed run of everything, `reps` repeats alternating in one process on one handle, median
(min ... max):
  field    pf_cost_field, one set of one source (the first free cell), with d_info: pf_last_kernel_ms (HIP events round the whole call:
           the validation kernel, the fill, the seeds, every round with the host's queue-length read, the info kernels) and
           pf_cost_field_work's launches / tile visits / words lowered (these depend on the schedule)
  parents  pf_cost_field_parents on that row, kernel ms
  (a)      pf_dist_field_merged, the level-synchronous unit-cost kernel, one set of that source, kernel ms; at cost == 1 the two rows
           are compared and must be bit-equal (asserted)
  (b)      the wall ms of tests/cost_checkers.dijkstra (a Python heap) over the same cost map, run ONCE per row (it is the slow side);
           its labels and parents are compared with the device's and must be equal (asserted).  --no-host skips it.
Cost maps: ones (c == 1), margin4 (Clearance.cost_map(margin=4)), rand50 (seeded uniform costs in [1, 50])."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from probe_clearance import clear_map  # noqa: E402
from probe_dist_field import med  # noqa: E402


def cost_of(name, g, cl):
    if name == "ones":
        return np.ones(g.shape)
    if name.startswith("margin"):
        return cl.cost_map(margin=float(name[6:]))
    if name.startswith("rand"):
        return 1.0 + np.random.default_rng(g.size).random(g.shape) * (float(name[4:]) - 1.0)
    raise SystemExit(f"unknown cost map {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="fig7,g256,up4,open1400,serp255")
    ap.add_argument("--policies", default="1,1")
    ap.add_argument("--costs", default="ones,margin4,rand50")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    import cost_checkers as ck
    import field_checkers as fc
    policies = [tuple(int(v) for v in p.split(",")) for p in a.policies.split(";")]
    rows = []
    print("| map | policy | cost map | largest label | field, kernel ms | launches / tile visits / words lowered | parents, kernel ms | "
          "(a) pf_dist_field_merged, kernel ms | field / (a) | (b) host heap, wall ms | (b) / field |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = clear_map(name)
        R, C = g.shape
        RC = g.size
        e = pathfit.Engine(g)
        cl = pathfit.Clearance(g, engine=e)
        src = int(np.flatnonzero(g.reshape(-1) != 1)[0])
        off, ids = np.array([0, 1], np.int32), np.array([src], np.int32)
        dcost, out, info, par = e.buf(RC, np.float64), e.buf(RC, np.float64), e.buf(4, np.int64), e.buf(RC, np.uint8)
        dist, dinfo = e.buf(RC, np.float64), e.buf(4, np.int64)
        for ad, rs in policies:
            mm = fc.move_masks(g, ad, rs)
            for cname in a.costs.split(","):
                cost = np.ascontiguousarray(cost_of(cname, g, cl), np.float64)
                dcost.upload(cost.reshape(-1))

                def field():
                    e.cost_field(dcost, off, ids, out, ad, rs, info)
                    ms, work = e.last_kernel_ms(), e.cost_field_work()
                    e.cost_field_parents(dcost, 1, out, par, ad, rs)
                    return ms, work, e.last_kernel_ms()

                def merged():
                    e.dist_field_merged(off, ids, dist, ad, rs, dinfo)
                    return e.last_kernel_ms()

                field(), merged()                                     # untimed: code objects, scratch
                F, W, P, M = [], [], [], []
                for _ in range(a.reps):
                    ms, work, pms = field()
                    F.append(ms)
                    W.append(work)
                    P.append(pms)
                    M.append(merged())
                D = out.download()
                if cname == "ones":
                    assert np.array_equal(D.view(np.uint64), dist.download().view(np.uint64)), (name, ad, rs, "the unit-cost rows differ")
                host_ms = None
                if not a.no_host:
                    t0 = time.perf_counter()
                    hd, hp = ck.dijkstra(g, mm, cost, [src])
                    host_ms = (time.perf_counter() - t0) * 1e3
                    assert np.array_equal(hd.reshape(-1).view(np.uint64), D.view(np.uint64)), (name, ad, rs, cname, "labels differ from the host's")
                    assert np.array_equal(hp.reshape(-1), par.download()), (name, ad, rs, cname, "parents differ from the host's")
                far = int(info.download()[2])
                wk = " / ".join(f"{int(np.median([w[i] for w in W]))}" for i in range(3))
                rows.append(dict(map=name, shape=[R, C], policy=[ad, rs], cost=cname, largest=float(D[far]) if far >= 0 else None, field_ms=F,
                                 work=[list(w) for w in W], parents_ms=P, merged_ms=M, host_ms=host_ms))
                print(f"| {name} {R}x{C} | {ad},{rs} | {cname} | {D[far] if far >= 0 else float('nan'):.1f} | {med(F)} | {wk} | {med(P)} | {med(M)} | "
                      f"{np.median(F) / np.median(M):.2f} | {'-' if host_ms is None else f'{host_ms:.0f}'} | "
                      f"{'-' if host_ms is None else f'{host_ms / np.median(F):.0f}'} |", flush=True)
        cl.close()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
