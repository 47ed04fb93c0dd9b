"""pf_place_improve's kernel time, moves and time per sweep on shared matrices, in the deals of the candidates the source holds.

    python scripts/probe_place.py [build] [--shapes 64x256x4,256x1024x8,1024x4096x16,1024x4096x64] [--bs 1,256] [--reps 3] [--long-moves 4]
                                  [--model-moves 1] [--json OUT]

Per (m, n, p): seeded points in the unit square, the Euclidean site-by-demand matrix, objective "sum".  Rows: the empty row (B = 1:
the greedy construction and the swaps behind it), then B perturbations of its result (what one round of Placement uploads).
Per row the kernel ms (HIP events, pf_last_kernel_ms: the validation kernels and the search) of every library given, alternating
`reps` times in one process after one untimed call of each, all outputs compared word for word; the moves and sweeps of the batch;
the microseconds per sweep of the longest start (kernel time / its sweeps: the starts run side by side); and the wall time of the
numpy model (tests/place_checkers.improve_numpy): the first start under a cap of `model-moves` moves, compared word for word with a
device call under the same cap, its time per sweep scaled to the sweeps of the batch.  Where m n p exceeds 2^26 the moves of a
start are capped at `long-moves` (the table says so): a sweep costs the same whichever move it follows.
The libraries: the shipped one (64 / P sites share a wavefront, P the power of two >= p, a lane reading its own row) and, with
`build`, lib/ab/libpathfit_pl_lanes.so (-DPF_PLACE_PACK=0: a wavefront per site and a lane per slot at every p, the terms' operands
broadcast lane by lane) and lib/ab/libpathfit_pl_mixed.so (-DPF_PLACE_PACK=1: the shipped form for p <= 32, the other above)."""
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

AB = {"lanes": ["-DPF_PLACE_PACK=0"], "mixed": ["-DPF_PLACE_PACK=1"]}
LONG = 1 << 26


def build_mod():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ab_path(name):
    return os.path.join(PKG, "lib", "ab", "libpathfit_pl_%s.so" % name)


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


def improve(e, m, n, dm, rows, limit):
    rows = np.ascontiguousarray(rows, np.int32)
    B, p = rows.shape
    ds = e.put(rows.reshape(-1))
    do, dv, dst, di = e.buf((B, n), np.int32), e.buf((B, 4), np.float64), e.buf(B, np.int32), e.buf((B, 4), np.int64)
    try:
        e.place_improve(0, m, n, p, 0, B, True, dm, limit, ds, do, dv, dst, di)
        return e.last_kernel_ms(), (ds.download().reshape(B, p), do.download().reshape(B, n), dv.download().reshape(B, 4), dst.download(), di.download().reshape(B, 4))
    finally:
        for b in (ds, do, dv, dst, di):
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("build", nargs="?", choices=["build"])
    ap.add_argument("--shapes", default="64x256x4,256x1024x8,1024x4096x16,1024x4096x64")
    ap.add_argument("--bs", default="1,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long-moves", type=int, default=4)
    ap.add_argument("--model-moves", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.build:
        build_all()
    import pathfit
    import place_checkers as pc
    from pathfit.placement import perturbations
    grid = np.zeros((4, 4), np.uint8)
    libs = {"shipped": pathfit.Engine(grid)}
    for name, so in [(x, ab_path(x)) for x in AB]:
        if os.path.exists(so):
            libs[name] = second_engine(so, grid)
    names = list(libs)
    print("| m | n | p | B | start | cap | " + " | ".join("ms (%s)" % x for x in names) + " | moves | sweeps | longest start's sweeps | us per sweep (shipped) | numpy model s |")
    print("|---|---|---|---|---|---|" + "---|" * (len(names) + 5))
    out_rows = []
    for m, n, p in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        rng = np.random.default_rng([m, n, p])
        s, d = rng.random((m, 2)), rng.random((n, 2))
        mat = np.ascontiguousarray(np.sqrt(((s[:, None, :] - d[None, :, :]) ** 2).sum(-1)))
        long_ = m * n * p > LONG
        limit = a.long_moves if long_ else 16 * p
        bufs = {x: e.put(mat.reshape(-1)) for x, e in libs.items()}
        jobs = [("empty", [[-1] * p])]
        # the incumbent the perturbed rows start from: the search's result, or under the cap a row of the p sites nearest to the demands' centre
        best = improve(libs["shipped"], m, n, bufs["shipped"], [[-1] * p], limit)[1][0][0] if not long_ else np.argsort(((s - d.mean(0)) ** 2).sum(1))[:p]
        for B in (int(v) for v in a.bs.split(",")):
            jobs.append(("perturbed", perturbations(rng, [int(v) for v in best], 0, m, B)))
        for kind, rows in jobs:
            B = len(rows)
            ms = {x: [] for x in names}
            ref, same = None, True
            for rep in range(a.reps + 1):
                for x in names:
                    t, out = improve(libs[x], m, n, bufs[x], rows, limit)
                    if rep:
                        ms[x].append(t)
                    if ref is None:
                        ref = out
                    same = same and all(u.tobytes() == v.tobytes() for u, v in zip(out, ref))
            capped = improve(libs["shipped"], m, n, bufs["shipped"], rows[:1], a.model_moves)[1]
            t0 = time.perf_counter()
            row, owner, v, st, info = pc.improve_numpy(mat, rows[0], 0, 0, a.model_moves)
            per_sweep = (time.perf_counter() - t0) / info[1]
            same = same and row == list(capped[0][0]) and owner == list(capped[1][0]) and np.array(v).tobytes() == capped[2][0].tobytes() \
                and st == capped[3][0] and list(info) == list(capped[4][0])
            med = {x: float(np.median(t)) for x, t in ms.items()}
            longest, sweeps = int(ref[4][:, 1].max()), int(ref[4][:, 1].sum())
            r = dict(m=m, n=n, p=p, B=B, start=kind, cap=limit, ms=ms, moves=int(ref[4][:, 0].sum()), sweeps=sweeps, longest=longest, capped=int((ref[3] == 2).sum()),
                     us_per_sweep=1000.0 * med["shipped"] / longest, model_s=per_sweep * sweeps, model_sweeps=int(info[1]), agree=bool(same))
            out_rows.append(r)
            print(f"| {m} | {n} | {p} | {B} | {kind} | {limit} | " + " | ".join("%.3f" % med[x] for x in names) + f" | {r['moves']} | {sweeps} | {longest} | "
                  f"{r['us_per_sweep']:.1f} | {r['model_s']:.2f} |" + ("" if same else " OUTPUTS DISAGREE"), flush=True)
        for x in names:
            bufs[x].free()
    for e in libs.values():
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out_rows, fh, indent=1)
    if not all(r["agree"] for r in out_rows):
        raise SystemExit("outputs disagree")


if __name__ == "__main__":
    main()
