"""Nearest-source queries: ONE merged field with its owner map (pathfit.NearestSourceField) against the route that existed before,
one DistanceField with K = S rows and paths(k=None).

    python scripts/probe_nearest_field.py [--maps up2,up4,open1024,serp256] [--ss 4,64,1024] [--targets 4096] [--policy 1,1] [--reps 3] [--json OUT]

Per (map, S): S seeded free cells as sources, `--targets` seeded free cells as targets; one untimed run of each route, then `--reps`
repeats alternating in ONE process.  A repeat of a route builds the object (the field kernel), forces its maps (parents, and owners
for the merged route), asks for the paths and closes it:
  kernel ms   HIP-event ms of the field + the parent maps (+ the owner map: links, ranks, the doubling rounds, the counts);
  paths ms    host wall clock around paths(targets): the trace, the copies back and the CellPath objects (and, for the K = S route,
              the K-way scan in front of the trace).
levels = the largest "levels that held a live cell" of the route's fields; device bytes = what the route keeps in HBM (labels,
parent maps, owners) plus the level lists it needs while the field runs.  Where the K = S rows cannot be allocated the row says so."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maaco-path-planing_amd"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from probe_dist_field import make_map, med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="up2,up4,open1024,serp256")
    ap.add_argument("--ss", default="4,64,1024")
    ap.add_argument("--targets", type=int, default=4096)
    ap.add_argument("--policy", default="1,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    ad, rs = (int(v) for v in a.policy.split(","))
    rows = []
    print("| map | S | levels merged / K = S | merged: kernel ms (field + parents + owners) | merged: paths ms | K = S: kernel ms (field + parents) | K = S: paths ms "
          "| kernel K = S / merged | paths K = S / merged | MiB merged / K = S |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = make_map(name)
        R, C = g.shape
        RC = g.size
        free = np.flatnonzero(g.reshape(-1) != 1)
        e = pathfit.Engine(g)
        cus = 256
        tg = [(int(v) // C, int(v) % C) for v in np.random.default_rng(7000).choice(free, a.targets, replace=a.targets > len(free))]
        for S in (int(v) for v in a.ss.split(",")):
            src = [(int(v) // C, int(v) % C) for v in np.random.default_rng(7100 + S).choice(free, S, replace=False)]

            def merged():
                n = pathfit.NearestSourceField(g, [src], ad, rs, engine=e)
                n._owner_buf()
                k = n.kernel_ms, n.parents_kernel_ms, n.owners_kernel_ms
                t0 = time.perf_counter()
                paths = n.paths(tg)
                wall = (time.perf_counter() - t0) * 1e3
                out = k, wall, int(n.info[0][0]), [len(p) for p in paths]
                n.close()
                return out

            def many():
                d = pathfit.DistanceField(g, src, ad, rs, engine=e)
                d._parent_buf()
                k = d.kernel_ms, d.parents_kernel_ms
                t0 = time.perf_counter()
                paths = d.paths(tg)
                wall = (time.perf_counter() - t0) * 1e3
                d.close()
                return k, wall, [len(p) for p in paths]

            bytes_m = 13 * RC + 12 * RC                               # labels, parents, owners; one workgroup's lists
            bytes_k = 9 * RC * S + 12 * RC * min(S, cus)
            m0 = merged()
            try:
                info = e.buf((S, 4), np.int64)                        # the levels of the K = S route: its kernel once more, with the counters
                rowsbuf = e.buf((S, RC), np.float64)
                e.dist_field_batch([r * C + c for r, c in src], rowsbuf, ad, rs, info)
                levels_k = int(info.download()[:, 0].max())
                rowsbuf.free(), info.free()
                k0 = many()
            except pathfit.PathfitError as ex:
                k0 = None
                why = str(ex)
            M, K = [], []
            for _ in range(a.reps):
                M.append(merged())
                if k0 is not None:
                    K.append(many())
            km, wm = [sum(r[0]) for r in M], [r[1] for r in M]
            row = dict(map=name, shape=[R, C], policy=[ad, rs], S=S, targets=a.targets, levels_merged=m0[2], merged_kernel_ms=[list(r[0]) for r in M],
                       merged_paths_ms=wm, bytes_merged=bytes_m, bytes_many=bytes_k)
            head = f"| {name} {R}x{C} | {S} | {m0[2]} / "
            if k0 is None:
                row.update(many="does not fit", why=why)
                print(head + f"- | {med(km)} | {med(wm)} | the K = S rows do not fit ({bytes_k / 2 ** 20:.0f} MiB) | - | - | - | {bytes_m / 2 ** 20:.0f} / - |", flush=True)
            else:
                kk, wk = [sum(r[0]) for r in K], [r[1] for r in K]
                agree = [bool(x) for x in M[-1][3]] == [bool(x) for x in K[-1][2]]
                row.update(levels_many=levels_k, many_kernel_ms=[list(r[0]) for r in K], many_paths_ms=wk, same_targets_reached=agree)
                print(head + f"{levels_k} | {med(km)} | {med(wm)} | {med(kk)} | {med(wk)} | {np.median(kk) / np.median(km):.2f} | {np.median(wk) / np.median(wm):.2f} | "
                      f"{bytes_m / 2 ** 20:.0f} / {bytes_k / 2 ** 20:.0f} |" + ("" if agree else " ROUTES DISAGREE"), flush=True)
            rows.append(row)
            if a.json:
                with open(a.json, "w") as fh:
                    json.dump(rows, fh, indent=1)
        e.close()


if __name__ == "__main__":
    main()
