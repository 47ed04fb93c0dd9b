"""pf_cover_improve's kernel time per sweep on shared masks, in the two deals of the candidates the source holds.

    python scripts/probe_cover.py [build] [--shapes 64x4096x4,256x65536x8,1024x1048576x16] [--bs 1,256] [--reps 3] [--moves 3] [--json OUT]

Per (m, n, p): seeded masks of density 1/8 (the AND of three random words), B full seeded rows over the one mask set, every start
capped at `moves` moves, so that every sweep is a swap sweep with p evaluated slots (a sweep costs the same whichever move it
follows).  Per row of the table the kernel ms (HIP events, pf_last_kernel_ms: the two validation kernels and the search) of every
library given, alternating `reps` times in one process after one untimed call of each, all outputs compared word for word; the
sweeps of the longest start; the ms per sweep (kernel time / the longest start's sweeps: the starts run side by side); and the
wall time per sweep of the numpy model (tests/cover_checkers.improve_numpy) on the first start, compared word for word with the
device's first start.
The libraries: the shipped one (PF_COVER_DEAL = 1: a wavefront per site, the words strided over the lanes, eight slots a pass)
and, with `build`, lib/ab/libpathfit_cv_deal0.so (-DPF_COVER_DEAL=0: lane = (site group, slot), a lane walks the words)."""
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

AB = {"deal0": ["-DPF_COVER_DEAL=0"]}


def build_mod():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ab_path(name):
    return os.path.join(PKG, "lib", "ab", "libpathfit_cv_%s.so" % name)


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
    W = (n + 63) // 64
    ds = e.put(rows.reshape(-1))
    dc, dv, dst, di = e.buf((B, W), np.uint64), e.buf((B, 4), np.int64), e.buf(B, np.int32), e.buf((B, 4), np.int64)
    try:
        e.cover_improve(m, n, p, 0, B, True, dm, limit, ds, dc, dv, dst, di)
        return e.last_kernel_ms(), (ds.download().reshape(B, p), dc.download().reshape(B, W), dv.download().reshape(B, 4), dst.download(), di.download().reshape(B, 4))
    finally:
        for b in (ds, dc, dv, dst, di):
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("build", nargs="?", choices=["build"])
    ap.add_argument("--shapes", default="64x4096x4,256x65536x8,1024x1048576x16")
    ap.add_argument("--bs", default="1,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--moves", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.build:
        build_all()
    import pathfit
    import cover_checkers as cc
    grid = np.zeros((4, 4), np.uint8)
    libs = {"shipped": pathfit.Engine(grid)}
    for name, so in [(x, ab_path(x)) for x in AB]:
        if os.path.exists(so):
            libs[name] = second_engine(so, grid)
    names = list(libs)
    print("| m | n | p | B | cap | " + " | ".join("ms (%s)" % x for x in names) + " | sweeps | longest start's sweeps | " +
          " | ".join("ms per sweep (%s)" % x for x in names) + " | numpy model s per sweep |")
    print("|---|---|---|---|---|" + "---|" * (2 * len(names) + 3))
    out_rows = []
    for m, n, p in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        rng = np.random.default_rng([m, n, p])
        W = (n + 63) // 64
        M = rng.integers(0, 2 ** 64, (m, W), dtype=np.uint64) & rng.integers(0, 2 ** 64, (m, W), dtype=np.uint64) & rng.integers(0, 2 ** 64, (m, W), dtype=np.uint64)
        if n % 64:
            M[:, -1] &= np.uint64((1 << (n % 64)) - 1)
        bufs = {x: e.put(M.reshape(-1)) for x, e in libs.items()}
        for B in (int(v) for v in a.bs.split(",")):
            rows = [[int(v) for v in rng.permutation(m)[:p]] for _ in range(B)]
            ms = {x: [] for x in names}
            ref, same = None, True
            for rep in range(a.reps + 1):
                for x in names:
                    t, out = improve(libs[x], m, n, bufs[x], rows, a.moves)
                    if rep:
                        ms[x].append(t)
                    if ref is None:
                        ref = out
                    same = same and all(u.tobytes() == v.tobytes() for u, v in zip(out, ref))
            t0 = time.perf_counter()
            want = cc.improve_numpy(M, n, rows[0], 0, a.moves)
            model = (time.perf_counter() - t0) / want[4][1]
            same = same and cc.same(tuple(x[0] for x in ref), want)
            med = {x: float(np.median(t)) for x, t in ms.items()}
            longest, sweeps = int(ref[4][:, 1].max()), int(ref[4][:, 1].sum())
            r = dict(m=m, n=n, p=p, B=B, cap=a.moves, ms=ms, sweeps=sweeps, longest=longest, ms_per_sweep={x: med[x] / longest for x in names}, model_s_per_sweep=model,
                     agree=bool(same))
            out_rows.append(r)
            print(f"| {m} | {n} | {p} | {B} | {a.moves} | " + " | ".join("%.3f" % med[x] for x in names) + f" | {sweeps} | {longest} | " +
                  " | ".join("%.3f" % r["ms_per_sweep"][x] for x in names) + f" | {model:.3f} |" + ("" if same else " OUTPUTS DISAGREE"), flush=True)
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
