"""Assignments: kernel time of pf_assign_solve per (n = m, B, matrix kind), the time per tree step in each form of the kernel, the
forms against each other, and the numpy model (and scipy, where it imports) on the same matrices.

    python scripts/probe_assign.py [--sizes 16,64,65,256,1024] [--batches 1,64,1024] [--kinds real,sqrt2,product] [--reps 5]
                                   [--forms group,t1024] [--json OUT]
    python scripts/probe_assign.py build --forms group,t1024      # compiles the other forms into lib/ab/ (no device needed)

Per row: pf_assign_solve (mode 0; seeded random, k1 + k2 sqrt(2) and the product matrix (i + 1)(j + 1), whose trees are the longest)
in the library's own form -- a wavefront per problem up to m = 64, a 256-thread workgroup per problem above -- and in every --forms
build loaded into the SAME process: group = -DPF_ASSIGN_WAVE_M=0 (the workgroup form at every m), t1024 = -DPF_ASSIGN_THREADS=1024
(a column a thread).  The forms alternate `reps` times after one untimed run of each, all on one device; kernel ms are HIP events
(pf_last_kernel_ms, the validation kernel included); the table gives the median and min .. max, the tree steps of the batch and each
form's microseconds per tree step (kernel time over the steps of the LONGEST problem: the problems of a batch run side by side).
B is cut so that a batch holds at most 2^24 entries (16 problems at 1024).  Every form's outputs are compared with the library's as
bytes, and the library's with the numpy model (tests/assign_checkers.solve_np) on the first 2 problems (1 from n = 512 on), whose wall time per problem
is the next column; the last is scipy.optimize.linear_sum_assignment's wall time per problem (its total compared within 1e-9
relative), or "-" where scipy does not import."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from probe_dist_field import med  # noqa: E402
from probe_smooth import second_engine  # noqa: E402

FORMS = {"group": ["-DPF_ASSIGN_WAVE_M=0"], "t1024": ["-DPF_ASSIGN_THREADS=1024"], "t256": ["-DPF_ASSIGN_THREADS=256"]}
ENTRIES_MAX = 1 << 24


def so_of(form):
    return os.path.join(PKG, "lib", "ab", f"libpathfit_assign_{form}.so")


def build_form(form):
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    os.makedirs(os.path.dirname(so_of(form)), exist_ok=True)
    subprocess.check_call(mod._cmd(so_of(form), FORMS[form]))
    return so_of(form)


def matrices(ac, kind, n, B):
    if kind == "product":
        return np.repeat(ac.product(n)[None], B, 0)
    return np.array([ac.matrix(kind, n, n, b) for b in range(B)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", nargs="?", default="run")
    ap.add_argument("--sizes", default="16,64,65,256,1024")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--kinds", default="real,sqrt2,product")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--forms", default="")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    forms = [f for f in a.forms.split(",") if f]
    if a.cmd == "build":
        for f in forms:
            print(build_form(f))
        return
    import pathfit
    import assign_checkers as ac
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        linear_sum_assignment = None
    g = np.zeros((4, 4), np.uint8)
    engines = {"lib": pathfit.Engine(g)}
    for f in forms:
        engines[f] = second_engine(so_of(f), g)
    names = list(engines)
    out_rows, models = [], {}
    print("| n = m | kind | B | " + " | ".join(f"{k} ms" for k in names) + " | tree steps (batch / longest) | µs / step (" + " / ".join(names) + ") | numpy model ms | scipy ms |")
    print("|---" * (7 + len(names)) + "|")
    for n in (int(v) for v in a.sizes.split(",")):
        for kind in a.kinds.split(","):
            done = set()
            for B in (int(v) for v in a.batches.split(",")):
                B = max(1, min(B, ENTRIES_MAX // (n * n)))
                if B in done:
                    continue
                done.add(B)
                mats = matrices(ac, kind, n, B)
                bufs, ms = {}, {k: [] for k in names}
                for k, e in engines.items():
                    bufs[k] = (e.put(mats.reshape(-1)), e.buf((B, n), np.int32), e.buf((B, 2), np.float64), e.buf(B, np.int32), e.buf((B, 2 * n), np.float64),
                               e.buf((B, 4), np.int64))
                for rep in range(a.reps + 1):
                    for k, e in engines.items():
                        dm, dc, dv, ds, dd, di = bufs[k]
                        e.assign_solve(0, n, n, B, dm, dc, dv, ds, dd, di)
                        if rep:
                            ms[k].append(e.last_kernel_ms())
                got = [b.download() for b in bufs["lib"][1:]]
                for k in forms:
                    for x, y in zip(got, (b.download() for b in bufs[k][1:])):
                        assert x.tobytes() == y.tobytes(), (n, kind, B, k)
                if (n, kind) not in models:                           # (problem b is the same matrix at every B)
                    t0 = time.perf_counter()
                    want = [ac.solve_np(d, 0) for d in mats[:1 if n >= 512 else 2]]
                    models[(n, kind)] = (want, (time.perf_counter() - t0) * 1e3 / len(want))
                want, model_ms = models[(n, kind)]
                want = want[:B]
                for b, w in enumerate(want):
                    have = ac.Result([int(c) for c in got[0][b]], got[1][b, 0], got[1][b, 1], got[3][b], [int(x) for x in got[4][b]], int(got[2][b]))
                    assert ac.words(have) == ac.words(w), (n, kind, B, b)
                scipy_ms = None
                if linear_sum_assignment is not None:
                    t0 = time.perf_counter()
                    r, c = linear_sum_assignment(mats[0])
                    scipy_ms = (time.perf_counter() - t0) * 1e3
                    assert abs(mats[0][r, c].sum() - got[1][0, 0]) <= 1e-9 * max(1.0, abs(got[1][0, 0])), (n, kind)
                for bs in bufs.values():
                    for b in bs:
                        b.free()
                steps = got[4][:, 0]
                per_step = " / ".join(f"{float(np.median(ms[k])) * 1e3 / max(int(steps.max()), 1):.2f}" for k in names)
                print(f"| {n} | {kind} | {B} | " + " | ".join(med(ms[k]) for k in names) +
                      f" | {int(steps.sum())} / {int(steps.max())} | {per_step} | {model_ms:.1f} | " +
                      ("-" if scipy_ms is None else f"{scipy_ms:.2f}") + " |", flush=True)
                out_rows.append(dict(n=n, kind=kind, B=B, ms=ms, steps=int(steps.sum()), longest=int(steps.max()), model_ms=model_ms, scipy_ms=scipy_ms))
    for e in engines.values():
        e.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out_rows, f, indent=1)


if __name__ == "__main__":
    main()
