"""M Dijkstra paths from one source: the routing tree (one distance field, one parent map, one trace, one score batch) against one
variant-2 search batch and the same score batch over the same M queries.

    python scripts/probe_field_paths.py [--maps up2,up4,serp256] [--ms 256,4096,65536] [--policy 1,1] [--reps 3] [--json OUT]

Per (map, M) and repeat, alternating in ONE process after one untimed run of each route:
  tree route    pf_dist_field_batch + pf_dist_field_parents + pf_dist_field_paths + pf_score_batch: the kernel ms of each (HIP events,
                pf_last_kernel_ms) and the host wall clock around the four synchronous calls;
  search route  pf_astar_batch(variant 2) + pf_score_batch: the host wall clock around the two synchronous calls (the batch may make
                several launches).
The source is cell (0, 0); the targets are M seeded free cells (drawn with replacement where the map has fewer).  Both routes write
rows of the engine's default capacity (R * C on the serpentine, whose paths are that long) into the same buffer; after the timed
repeats the lengths, statuses and stats of the two routes are compared (they must be equal).  The table gives the median and
min .. max of the repeats.  The serpentine map serialises the field (one cell per level) and takes M <= 4096 (a
row holds R * C cells there)."""
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
    ap.add_argument("--maps", default="up2,up4,serp256")
    ap.add_argument("--ms", default="256,4096,65536")
    ap.add_argument("--policy", default="1,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    from pathfit.engine import score_params
    ad, rs = (int(v) for v in a.policy.split(","))
    sp = score_params(0, rs)
    rows = []
    print("| map | M | field ms | parents ms | trace ms | score ms | tree route, wall ms | search batch + score, wall ms | search / tree | cells per path (mean) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = make_map(name)
        RC = g.size
        serp = name.startswith("serp")
        free = np.flatnonzero(g.reshape(-1) != 1)
        e = pathfit.Engine(g)
        cap = RC if serp else e.default_path_cap()
        f, p = e.buf((1, RC), np.float64), e.buf((1, RC), np.uint8)
        for M in (int(v) for v in a.ms.split(",")):
            if serp and M > 4096:
                continue
            tg = np.random.default_rng(5000 + M).choice(free, M, replace=M > len(free)).astype(np.int32)
            dt, ds0, dk = e.put(tg), e.put(np.zeros(M, np.int32)), e.put(np.zeros(M, np.int32))
            dc, dl, dst, dstat = e.buf((M, cap), np.int32), e.buf(M, np.int32), e.buf(M, np.int32), e.buf((M, 5), np.float64)

            def tree():
                t0 = time.perf_counter()
                e.dist_field_batch([0], f, ad, rs); k0 = e.last_kernel_ms()
                e.dist_field_parents(1, f, p, ad, rs); k1 = e.last_kernel_ms()
                e.dist_field_paths(1, p, dt, M, cap, dc, dl, dst, dk); k2 = e.last_kernel_ms()
                e.score_batch(M, cap, dc, dl, dstat, sp); k3 = e.last_kernel_ms()
                return k0, k1, k2, k3, (time.perf_counter() - t0) * 1e3

            def search():
                t0 = time.perf_counter()
                e.astar_batch(2, ds0, dt, M, cap, dc, dl, dst, allow_diag=ad, restrict_corner=rs)
                e.score_batch(M, cap, dc, dl, dstat, sp)
                return (time.perf_counter() - t0) * 1e3

            tree(), search()                                           # warm-up: code objects, level lists, search slots
            T, S = [], []
            for _ in range(a.reps):
                T.append(tree())
                got = (dl.download(), dst.download(), dstat.download())
                S.append(search())
                want = (dl.download(), dst.download(), dstat.download())
            same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, want))
            T = np.array(T)
            row = dict(map=name, shape=list(g.shape), policy=[ad, rs], M=M, path_cap=cap, field_ms=T[:, 0].tolist(), parents_ms=T[:, 1].tolist(),
                       trace_ms=T[:, 2].tolist(), score_ms=T[:, 3].tolist(), tree_wall_ms=T[:, 4].tolist(), search_wall_ms=S, routes_agree=bool(same),
                       mean_cells=float(want[0].mean()))
            rows.append(row)
            print(f"| {name} {g.shape[0]}x{g.shape[1]} | {M} | {med(T[:, 0])} | {med(T[:, 1])} | {med(T[:, 2])} | {med(T[:, 3])} | {med(T[:, 4])} | {med(S)} | "
                  f"{np.median(S) / np.median(T[:, 4]):.2f} | {row['mean_cells']:.1f} |" + ("" if same else " ROUTES DISAGREE"), flush=True)
            for b in (dt, ds0, dk, dc, dl, dst, dstat):
                b.free()
        f.free(), p.free()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
