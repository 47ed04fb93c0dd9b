"""Turn-field repair (pf_turn_field_repair) per (map, policy, cost map, change): the kernel ms and the work counters of one repair of
one field from one source, against pf_turn_field from nothing on the same handle and the same new map.

    python scripts/probe_turn_repair.py [--maps g256,up2,up4] [--policies "1,1"] [--costs none,margin4] [--weight 0.3] [--reps 5] [--json OUT]

Maps, doors and changes are scripts/probe_cost_repair.py's (g256, 512 x 512 and 1024 x 1024 with the middle wall and two doors; near /
far / door- / door+ / mix16).  Per row, after one untimed run of both, `reps` repeats alternating in one process on one handle,
median (min ... max): the states and best of the old map are copied back (device to device, untimed), then
  repair   pf_turn_field_repair with d_info: pf_last_kernel_ms (HIP events round the whole call: the validation kernel when there is a
           cost map, both phases with the host's queue-length reads, the info kernels) and pf_turn_field_work's launches / tile visits
           / state words lowered / state words raised (the first three depend on the schedule)
  fresh    pf_turn_field from nothing with d_info on the new map, kernel ms, launches / tile visits
and the states, best and infos must be bit-equal in every repeat (asserted).  Cost maps: none (no buffer: c == 1), margin4
(Clearance.cost_map(margin=4) of the OLD map, kept for the new one; a cell that opens costs 1).

One process, one handle, host work on one thread.  On a shared machine run one map per command, each under a time limit of its own,
chained so that a failure ends the chain:
    timeout -k 10 300 python scripts/probe_turn_repair.py --maps g256 && timeout -k 10 600 python scripts/probe_turn_repair.py --maps up2 && \\
    timeout -k 10 900 python scripts/probe_turn_repair.py --maps up4"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from probe_clearance import clear_map  # noqa: E402
from probe_cost_repair import changes_of, walled  # noqa: E402
from probe_dist_field import med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="g256,up2,up4")
    ap.add_argument("--policies", default="1,1")
    ap.add_argument("--costs", default="none,margin4")
    ap.add_argument("--weight", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    policies = [tuple(int(v) for v in p.split(",")) for p in a.policies.split(";")]
    wt = a.weight
    rows = []
    print("| map | policy | cost map | change | repair, kernel ms | launches / tile visits / state words lowered / state words raised | fresh, kernel ms | "
          "fresh launches / tile visits | repair / fresh |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g, door = walled(clear_map(name))
        R, C = g.shape
        RC = g.size
        src = int(np.flatnonzero(g.reshape(-1) != 1)[0])
        e = pathfit.Engine(g)
        cl = pathfit.Clearance(g, engine=e)
        costs = {c: None if c == "none" else np.ascontiguousarray(cl.cost_map(margin=float(c[6:])), np.float64) for c in a.costs.split(",")}
        cl.close()
        off, ids = np.array([0, 1], np.int32), np.array([src], np.int32)
        dbuf = e.buf(RC, np.float64)
        old_s, out_s, ref_s = (e.buf(8 * RC, np.float64) for _ in range(3))
        old_b, out_b, ref_b = (e.buf(RC, np.float64) for _ in range(3))
        info, rinfo = e.buf(4, np.int64), e.buf(4, np.int64)
        for ad, rs in policies:
            for cname, cost in costs.items():
                dcost = None if cost is None else dbuf
                for change, g0, g1 in changes_of(g, door, src):
                    changed = np.flatnonzero((g0.reshape(-1) == 1) != (g1.reshape(-1) == 1)).astype(np.int32)
                    e.update_grid(g0)
                    if cost is not None:
                        dcost.upload(cost.reshape(-1))
                    e.turn_field(dcost, wt, off, ids, old_s, old_b, ad, rs, None)
                    e.update_grid(g1)
                    if cost is not None:
                        dcost.upload(np.where((g0 == 1) & (g1 != 1), 1.0, cost).reshape(-1))

                    def repair():
                        out_s.copy_from(0, old_s, 0, 8 * RC)
                        out_b.copy_from(0, old_b, 0, RC)
                        e.turn_field_repair(dcost, wt, changed, off, ids, out_s, out_b, ad, rs, info)
                        return e.last_kernel_ms(), e.turn_field_work()

                    def fresh():
                        e.turn_field(dcost, wt, off, ids, ref_s, ref_b, ad, rs, rinfo)
                        return e.last_kernel_ms(), e.turn_field_work()

                    repair(), fresh()                                 # untimed: code objects, scratch
                    P, W, F, V = [], [], [], []
                    for _ in range(a.reps):
                        ms, work = repair()
                        P.append(ms)
                        W.append(work)
                        ms, work = fresh()
                        F.append(ms)
                        V.append(work)
                        where = (name, ad, rs, cname, change)
                        assert np.array_equal(out_s.download().view(np.uint64), ref_s.download().view(np.uint64)), (where, "states differ")
                        assert np.array_equal(out_b.download().view(np.uint64), ref_b.download().view(np.uint64)), (where, "best differs")
                        assert np.array_equal(info.download(), rinfo.download()), (where, "infos differ")
                    wk = " / ".join(f"{int(np.median([w[i] for w in W]))}" for i in range(4))
                    vk = " / ".join(f"{int(np.median([w[i] for w in V]))}" for i in range(2))
                    rows.append(dict(map=name, shape=[R, C], policy=[ad, rs], cost=cname, weight=wt, change=change, repair_ms=P,
                                     repair_work=[list(w) for w in W], fresh_ms=F, fresh_work=[list(w) for w in V]))
                    print(f"| {name} {R}x{C} | {ad},{rs} | {cname} | {change} | {med(P)} | {wk} | {med(F)} | {vk} | {np.median(P) / np.median(F):.2f} |", flush=True)
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
