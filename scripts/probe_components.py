"""Connected components (pf_components) per (map, policy): the kernel ms of each phase and of the whole call, against what the same
answer costs today.

    python scripts/probe_components.py [--maps g128crop,up2,up4,open1024,serp1024,checker1024,rand1024] [--policies 11,10,01,00]
                                       [--reps 3] [--other SO | --other build] [--json OUT]

Per (map, policy), after one untimed run of everything, `reps` repeats alternating in one process, median (min … max):
  phases   pf_components with d_info under pf_set_option "components_phases" = 1: init + link, flatten, rank, labels, sizes + info (HIP
           events between the launches) and their span; and the span of a call without the phase events (pf_last_kernel_ms)
  other    with --other, the same call on a second build of the library loaded into the SAME process, alternating with the first
           (`--other build` compiles lib/ab/libpathfit_cc_other.so with PF_CC_OTHER_FLAGS, default -DPF_CC_TILED=0); the labels of the
           two builds are compared
  (a)      what the handle pays today for the same labels (ensure_comp: masks to the host, a serial flood fill, labels back): the wall
           ms of the first one-pair pf_astar_batch on two adjacent free cells after pf_update_grid, minus the second such call
  (b)      one pf_dist_field_batch row from the first cell of the largest component: today's only public reachability mask
The labels are checked against (b): the cells (b) reaches are the cells of the largest component."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from probe_dist_field import make_map, med  # noqa: E402
from probe_smooth import second_engine  # noqa: E402

OTHER_SO = os.path.join(PKG, "lib", "ab", "libpathfit_cc_other.so")
PHASES = ("init + link", "flatten", "rank", "labels", "sizes + info")


def build_other():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    os.makedirs(os.path.dirname(OTHER_SO), exist_ok=True)
    subprocess.check_call(mod._cmd(OTHER_SO, os.environ.get("PF_CC_OTHER_FLAGS", "-DPF_CC_TILED=0").split()))
    return OTHER_SO


def cc_map(name):
    if name.startswith("checker"):
        n = int(name[7:])
        rr, cc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        return ((rr + cc) % 2 == 1).astype(np.uint8)
    if name.startswith("rand"):
        n = int(name[4:])
        return (np.random.default_rng(41).random((n, n)) < 0.41).astype(np.uint8)
    return make_map(name)


def adjacent_pair(g):
    """Two free cells side by side in a row; on a map without such a pair (the checkerboard) two that touch diagonally."""
    C = g.shape[1]
    for dr, dc in ((0, 1), (1, 1)):
        ok = (g[:g.shape[0] - dr, :-1] != 1) & (g[dr:, 1:] != 1)
        if ok.any():
            r, c = (int(v[0]) for v in np.nonzero(ok))
            return r * C + c, (r + dr) * C + c + dc
    raise SystemExit("no two neighbouring free cells")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="g128crop,up2,up4,open1024,serp1024,checker1024,rand1024")
    ap.add_argument("--policies", default="11,10,01,00")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--other", default=None, help="a second build of the library, or `build`")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    other_so = build_other() if a.other == "build" else a.other
    rows = []
    print("| map | policy | components | largest | " + " | ".join(PHASES) + " | phases' span | call without phase events | other build | "
          "(a) first search after a map change − second, wall ms | (b) one field row, kernel ms | call / (a) | call / (b) |")
    print("|---|---|---|---|" + "---|" * (len(PHASES) + 7))
    for name in a.maps.split(","):
        g = cc_map(name)
        RC = g.size
        e = pathfit.Engine(g)
        e2 = second_engine(other_so, g) if other_so else None
        lab, info = e.buf(RC, np.int32), e.buf(4, np.int64)
        lab2, info2 = (e2.buf(RC, np.int32), e2.buf(4, np.int64)) if e2 else (None, None)
        field = e.buf((1, RC), np.float64)
        s, t = adjacent_pair(g)
        ds, dt = e.put([s], np.int32), e.put([t], np.int32)
        dc, dl, dst = e.buf((1, 64), np.int32), e.buf(1, np.int32), e.buf(1, np.int32)
        for pol in a.policies.split(","):
            ad, rs = int(pol[0]), int(pol[1])

            def phases():
                e.set_option("components_phases", 1)
                e.components(lab, ad, rs, info)
                span = e.last_kernel_ms()
                e.set_option("components_phases", 0)
                return list(e.components_phase_ms()) + [span]

            def call(eng, lb, ib):
                eng.components(lb, ad, rs, ib)
                return eng.last_kernel_ms()

            def search():
                t0 = time.perf_counter()
                e.astar_batch(0, ds, dt, 1, 64, dc, dl, dst, None, None, None, ad, rs)
                return (time.perf_counter() - t0) * 1e3

            def todays():
                e.update_grid(g)
                first = search()
                return first - search()

            def row_b(cell):
                e.dist_field_batch([cell], field, ad, rs)
                return e.last_kernel_ms()

            phases(), call(e, lab, info), todays()                    # untimed: code objects, scratch, records
            if e2:
                call(e2, lab2, info2)
            inf = info.download()
            count, big = int(inf[0]), int(inf[3])
            labels = lab.download()
            src = int(np.flatnonzero(labels == big)[0])
            row_b(src)
            P, T, O, A, B = [], [], [], [], []
            for _ in range(a.reps):
                P.append(phases())
                T.append(call(e, lab, info))
                if e2:
                    O.append(call(e2, lab2, info2))
                A.append(todays())
                B.append(row_b(src))
            ok = np.array_equal(np.isfinite(field.download().reshape(-1)), labels == big)
            if e2:
                ok = ok and np.array_equal(labels, lab2.download()) and np.array_equal(inf, info2.download())
            P = np.array(P)
            rows.append(dict(map=name, shape=list(g.shape), policy=[ad, rs], components=count, largest=int(inf[2]), free=int(inf[1]),
                             phases_ms={k: P[:, i].tolist() for i, k in enumerate(PHASES)}, phases_span_ms=P[:, 5].tolist(), call_ms=T, other_ms=O,
                             todays_ms=A, field_row_ms=B, agree=bool(ok)))
            print(f"| {name} {g.shape[0]}x{g.shape[1]} | ({ad}, {rs}) | {count} | {int(inf[2])} | " + " | ".join(med(P[:, i]) for i in range(5)) +
                  f" | {med(P[:, 5])} | {med(T)} | {med(O) if O else '-'} | {med(A)} | {med(B)} | {np.median(T) / np.median(A):.3f} | "
                  f"{np.median(T) / np.median(B):.4f} |" + ("" if ok else " DISAGREE"), flush=True)
        for b in (lab, info, field, ds, dt, dc, dl, dst, lab2, info2):
            if b is not None:
                b.free()
        if e2:
            e2.close()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
