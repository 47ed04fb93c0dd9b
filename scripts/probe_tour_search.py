"""pf_tour_improve's kernel time, moves and time per sweep on shared matrices, in the library's form and in other builds of it.

    python scripts/probe_tour_search.py [build] [--ns 64,256,1024] [--bs 1,32,256] [--reps 5] [--model-starts 4] [--json OUT]

Per n: seeded points in the unit square, their Euclidean matrix, the nearest-neighbour order.  Rows: the nearest-neighbour start
(B = 1), then B double-bridge perturbations of its 2-opt optimum (what one round of TourSearch uploads).  Per row the kernel ms
(HIP events, pf_last_kernel_ms: the two validation kernels and the search) of every library given, alternating `reps` times in one
process after one untimed call of each, all outputs compared word for word; the moves and sweeps of the batch; the microseconds per
sweep of the longest start (kernel time / its sweeps: the starts run side by side); and the wall time of the numpy model
(tests/tour_search_checkers.two_opt_numpy) on the first `model-starts` starts, scaled to B, its outputs compared too.
The libraries: the shipped one and, with `build`, three more in lib/ab/: 256 threads a workgroup instead of 1024, and one or eight
pairs a thread in flight instead of four.  (The forms that were dropped -- the matrix in LDS, the threads chosen by n -- and their
numbers: docs/experiments/.)"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

AB = {"t256": ["-DPF_TOUR_SEARCH_GROUP=256"], "unroll1": ["-DPF_TOUR_SEARCH_UNROLL=1"], "unroll8": ["-DPF_TOUR_SEARCH_UNROLL=8"]}


def build_mod():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ab_path(name):
    return os.path.join(PKG, "lib", "ab", "libpathfit_ts_%s.so" % name)


def build_all():
    mod = build_mod()
    mod.build()
    os.makedirs(os.path.dirname(ab_path("x")), exist_ok=True)
    procs = [subprocess.Popen(mod._cmd(ab_path(k), v)) for k, v in AB.items()]
    if any(p.wait() for p in procs):
        raise SystemExit("hipcc failed")


def second_engine(so, grid):
    """An Engine on another build of the library, in this process."""
    from pathfit import _lib
    from pathfit.engine import Engine
    L = ctypes.CDLL(os.path.abspath(so))
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    keep, _lib._LIB = _lib._LIB, L
    try:
        return Engine(grid)
    finally:
        _lib._LIB = keep


def improve(e, n, dm, starts, cap):
    B = len(starts)
    do = e.put(np.ascontiguousarray(starts, np.int32).reshape(-1))
    dv, ds, di = e.buf((B, 2), np.float64), e.buf(B, np.int32), e.buf((B, 4), np.int64)
    try:
        e.tour_improve(1, n, B, True, dm, cap, do, dv, ds, di)
        return e.last_kernel_ms(), (do.download().reshape(B, n), dv.download().reshape(B, 2), ds.download(), di.download().reshape(B, 4))
    finally:
        for b in (do, dv, ds, di):
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("build", nargs="?", choices=["build"])
    ap.add_argument("--ns", default="64,256,1024")
    ap.add_argument("--bs", default="1,32,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-starts", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.build:
        build_all()
    import pathfit
    import tour_search_checkers as ts
    from pathfit.tour_search import double_bridge, nearest_neighbour
    grid = np.zeros((4, 4), np.uint8)
    libs = {"shipped": pathfit.Engine(grid)}
    for name, so in [(k, ab_path(k)) for k in AB]:
        if os.path.exists(so):
            libs[name] = second_engine(so, grid)
    names = list(libs)
    print("| n | B | start | " + " | ".join("ms (%s)" % k for k in names) + " | moves | sweeps | longest start's sweeps | us per sweep (shipped) | numpy model s |")
    print("|---|---|---|" + "---|" * (len(names) + 5))
    rows = []
    for n in (int(v) for v in a.ns.split(",")):
        p = np.random.default_rng(n).random((n, 2))
        d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
        cap = 16 * n
        bufs = {k: e.put(d.reshape(-1)) for k, e in libs.items()}
        start = nearest_neighbour(ts.mirror(d), 1)
        best = improve(libs["shipped"], n, bufs["shipped"], [start], cap)[1][0][0]
        rng = np.random.default_rng(n + 1)
        jobs = [("nn", [start])]
        for B in (int(v) for v in a.bs.split(",")):
            jobs.append(("perturbed", [double_bridge(best, *np.sort(rng.choice(np.arange(1, n + 1), 3, replace=False))) for _ in range(B)]))
        for kind, starts in jobs:
            B = len(starts)
            ms = {k: [] for k in names}
            ref = None
            same = True
            for rep in range(a.reps + 1):
                for k in names:
                    t, out = improve(libs[k], n, bufs[k], starts, cap)
                    if rep:
                        ms[k].append(t)
                    if ref is None:
                        ref = out
                    same = same and all(x.tobytes() == y.tobytes() for x, y in zip(out, ref))
            m = min(B, a.model_starts)
            t0 = time.perf_counter()
            for b in range(m):
                o, v, st, info = ts.two_opt_numpy(d, starts[b], 1, cap)
                same = same and o == list(ref[0][b]) and np.array(v).tobytes() == ref[1][b].tobytes() and st == ref[2][b] and list(info) == list(ref[3][b])
            model_s = (time.perf_counter() - t0) * B / m
            med = {k: float(np.median(v)) for k, v in ms.items()}
            longest = int(ref[3][:, 1].max())
            row = dict(n=n, B=B, start=kind, ms=ms, moves=int(ref[3][:, 0].sum()), sweeps=int(ref[3][:, 1].sum()), longest=longest,
                       us_per_sweep=1000.0 * med["shipped"] / longest, model_s=model_s, model_starts=m, agree=bool(same))
            rows.append(row)
            print(f"| {n} | {B} | {kind} | " + " | ".join("%.3f" % med[k] for k in names) + f" | {row['moves']} | {row['sweeps']} | {longest} | "
                  f"{row['us_per_sweep']:.1f} | {model_s:.2f} |" + ("" if same else " OUTPUTS DISAGREE"), flush=True)
        for k in names:
            bufs[k].free()
    for e in libs.values():
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    if not all(r["agree"] for r in rows):
        raise SystemExit("outputs disagree")


if __name__ == "__main__":
    main()
