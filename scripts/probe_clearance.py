"""Clearance fields (pf_clearance_field) per (map, border): the kernel ms of the call, against what the only exact obstacle distance
of today costs: the scorer's windowed pair k_edt_rows / k_edt_cols driven to W = max(R, C).

    python scripts/probe_clearance.py [--maps fig7,g256,up4,dense4096,open4096] [--reps 3] [--rows 4096] [--row-maps g256,up4] [--other SO] [--json OUT]

Per (map, border), after one untimed run of everything, `reps` repeats alternating in one process on one handle, median (min … max):
  field    pf_clearance_field with d_near and d_info (pf_last_kernel_ms: HIP events round the launches)
  other    with --other, the same call on a second build of the library loaded into the SAME process (a build with another
           -DPF_CLEAR_SCAN_ROWS: 0 is the pure envelope pass, a value >= R the pure outward scan); the outputs are compared
  (a)      the windowed pair as a user reaches it: pf_update_grid, then the wall ms of the first one-row pf_score_batch with
           min_safe_distance = max(R, C), minus a second such call
  (b)      the host's share of (a): the penalty table of W^2 + 2 doubles, rebuilt alone by a call with min_safe_distance =
           max(R, C) - 0.5 (the same W, so the distance table stands), minus a plain call.  (a) - (b) is the pair itself with its
           two allocations.
The open map (one obstacle in a corner) is probed with the border off only.  Then, per map of --row-maps: pf_clearance_paths over `rows` traced
Dijkstra rows (one field from the first free cell, seeded targets) and pf_clearance_segments over their smoothed waypoints."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from probe_dist_field import make_map, med  # noqa: E402
from probe_smooth import second_engine  # noqa: E402


def clear_map(name):
    if name in ("fig7", "g256"):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import golden_io as gio
        g = gio.grid(name)[0].copy()
        g[(g == 2) | (g == 3)] = 0
        return g
    if name.startswith("dense"):
        n = int(name[5:])
        return (np.random.default_rng(n).random((n, n)) < 0.3).astype(np.uint8)
    if name.startswith("open"):
        g = np.zeros((int(name[4:]),) * 2, np.uint8)
        g[0, 0] = 1
        return g
    return make_map(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="fig7,g256,up4,dense4096,open4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--row-maps", default="g256,up4", help="the maps whose path rows and segments are probed")
    ap.add_argument("--other", default=None, help="a second build of the library")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    from pathfit.engine import score_params
    out_rows = []
    print("| map | border | obstacles | largest d2 | field, kernel ms | other build | (a) windowed pair as reached today, wall ms | (b) its host table, wall ms "
          "| field / ((a) − (b)) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = clear_map(name)
        R, C = g.shape
        RC, W = g.size, max(g.shape)
        e = pathfit.Engine(g)
        e2 = second_engine(a.other, g) if a.other else None
        d2, near, info = e.buf(RC, np.int32), e.buf(RC, np.int32), e.buf(4, np.int64)
        o2, n2, i2 = (e2.buf(RC, np.int32), e2.buf(RC, np.int32), e2.buf(4, np.int64)) if e2 else (None, None, None)
        row, ln, stats = e.put([0, 1], np.int32), e.put([2 if RC > 1 else 1], np.int32), e.buf((1, 5), np.float64)

        def score(min_safe):
            t0 = time.perf_counter()
            e.score_batch(1, 2, row, ln, stats, score_params(0, True, 0.1, 0.05, float(min_safe), 1000.0))
            return (time.perf_counter() - t0) * 1e3

        def todays():
            e.update_grid(g)
            first = score(W)
            return first - score(W)

        def table():
            first = score(W - 0.5)
            again = score(W - 0.5)
            score(W)                                                  # (the table of `todays` again)
            return first - again

        def field(eng, bufs, border):
            eng.clearance_field(bufs[0], border, bufs[1], bufs[2])
            return eng.last_kernel_ms()

        for border in ((0,) if name.startswith("open") else (0, 1)):
            field(e, (d2, near, info), border), todays(), table()        # untimed: code objects, scratch, tables
            if e2:
                field(e2, (o2, n2, i2), border)
            F, O, A, B = [], [], [], []
            for _ in range(a.reps):
                F.append(field(e, (d2, near, info), border))
                if e2:
                    O.append(field(e2, (o2, n2, i2), border))
                A.append(todays())
                B.append(table())
            inf = info.download()
            ok = True
            if e2:
                ok = all(np.array_equal(x.download(), y.download()) for x, y in ((d2, o2), (near, n2), (info, i2)))
            pair = np.median(A) - np.median(B)
            out_rows.append(dict(map=name, shape=[R, C], border=border, obstacles=int(inf[0]), largest_d2=int(inf[2]), field_ms=F, other_ms=O,
                                 todays_ms=A, table_ms=B, agree=bool(ok)))
            print(f"| {name} {R}x{C} | {border} | {int(inf[0])} | {int(inf[2])} | {med(F)} | {med(O) if O else '-'} | {med(A)} | {med(B)} | "
                  f"{np.median(F) / pair:.4f} |" + ("" if ok else " DISAGREE"), flush=True)

        if name not in a.row_maps.split(","):
            if e2:
                e2.close()
            e.close()
            continue
        # path rows and segments against the border-off field
        e.clearance_field(d2, False)
        free = np.flatnonzero(g.reshape(-1) != 1)
        df = pathfit.DistanceField(g, [(int(free[0]) // C, int(free[0]) % C)], engine=e)
        n = a.rows
        targets = np.random.default_rng(5).choice(free, n).astype(np.int32)
        dc, dl, dst, dch, cap = df._trace(targets, np.zeros(n, np.int32), False, None)
        po, ps = e.buf((n, 4), np.int32), e.buf(n, np.int32)
        P = []
        for _ in range(a.reps + 1):
            e.clearance_paths(d2, n, cap, dc, dl, 4, po, ps)
            P.append(e.last_kernel_ms())
        lens = dl.download()
        sm = pathfit.PathSmoother(g, engine=e)
        dw, dwl, dss, dws, wcap = sm.smooth_device(dc, dl, n, cap)
        way, wl = dw.download().reshape(n, wcap), dwl.download()
        fa = np.concatenate([way[i, :wl[i] - 1] for i in range(n) if wl[i] > 1] or [np.zeros(0, np.int32)])
        fb = np.concatenate([way[i, 1:wl[i]] for i in range(n) if wl[i] > 1] or [np.zeros(0, np.int32)])
        S = []
        if len(fa):
            da, db, dm, dat = e.put(fa), e.put(fb), e.buf(len(fa), np.int32), e.buf(len(fa), np.int32)
            for _ in range(a.reps + 1):
                e.clearance_segments(d2, da, db, len(fa), dm, dat, True)
                S.append(e.last_kernel_ms())
        print(f"|   {name}: pf_clearance_paths, {n} rows, {int(lens.sum())} cells: {med(P[1:])} ms; pf_clearance_segments, {len(fa)} segments (touched): "
              f"{med(S[1:]) if S else '-'} ms |", flush=True)
        out_rows.append(dict(map=name, rows=n, cells=int(lens.sum()), paths_ms=P[1:], segments=int(len(fa)), segments_ms=S[1:]))
        df.close()
        if e2:
            e2.close()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out_rows, fh, indent=1)


if __name__ == "__main__":
    main()
