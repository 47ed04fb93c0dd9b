"""Tours: kernel time of pf_tour_solve per (m, B), the table's two homes against each other, and the numpy layer model on the same
matrices.

    python scripts/probe_tour.py [--m 8,12,16] [--batches 1,64,1024] [--reps 5] [--forms hbm] [--json OUT]
    python scripts/probe_tour.py build --forms hbm        # compiles the other form into lib/ab/ (no device needed)

Per row: pf_tour_solve (mode 0, no needs, seeded asymmetric matrices) in the library's own form -- the table in LDS with the layer
loop in the kernel up to m = 9, in HBM with one launch per layer above -- and in every --forms build loaded into the SAME process:
hbm = -DPF_TOUR_LDS_M=0 (the table in HBM and a launch per layer at every m).  The forms alternate `reps` times after one untimed
run of each, all on one device; kernel ms are HIP events (pf_last_kernel_ms, the validation kernel included); the table gives the
median and min .. max.  m = 16 runs only up to the B whose tables fit the library's budget (256 MiB: 32 problems).  Every form's
totals, orders, statuses and info are compared with the library's, and the library's with the numpy layer model
(tests/tour_checkers.held_karp_layers) on the first 4 problems, whose wall time per problem is the last column."""
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

FORMS = {"hbm": ["-DPF_TOUR_LDS_M=0"]}
TABLE_BYTES = 256 << 20


def so_of(form):
    return os.path.join(PKG, "lib", "ab", f"libpathfit_tour_{form}.so")


def build_form(form):
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    os.makedirs(os.path.dirname(so_of(form)), exist_ok=True)
    subprocess.check_call(mod._cmd(so_of(form), FORMS[form]))
    return so_of(form)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", nargs="?", default="run")
    ap.add_argument("--m", default="8,12,16")
    ap.add_argument("--batches", default="1,64,1024")
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
    import tour_checkers as tc
    g = np.zeros((4, 4), np.uint8)
    engines = {"lib": pathfit.Engine(g)}
    for f in forms:
        engines[f] = second_engine(so_of(f), g)
    names = list(engines)
    out_rows = []
    print("| m | B | " + " | ".join(f"{n} ms" for n in names) + " | problems / ms (lib) | numpy layer model, one problem, wall ms |")
    print("|---" * (4 + len(names)) + "|")
    for m in (int(v) for v in a.m.split(",")):
        n = m + 1
        fit = max(TABLE_BYTES // ((1 << m) * m * 8), 1)
        done = set()
        for B in (int(v) for v in a.batches.split(",")):
            B = min(B, fit) if m >= 16 else B
            if B in done:
                continue
            done.add(B)
            mats = np.array([tc.matrix("asym", n, b) for b in range(B)])
            bufs, ms = {}, {k: [] for k in names}
            for k, e in engines.items():
                bufs[k] = (e.put(mats.reshape(-1)), e.buf(B, np.float64), e.buf((B, n), np.int32), e.buf(B, np.int32), e.buf((B, 4), np.int64))
            for rep in range(a.reps + 1):
                for k, e in engines.items():
                    dm, dt, do, ds, di = bufs[k]
                    e.tour_solve(0, n, B, dm, dt, do, ds, None, di)
                    if rep:
                        ms[k].append(e.last_kernel_ms())
            got = [b.download() for b in bufs["lib"][1:]]
            for k in forms:
                for x, y in zip(got, (b.download() for b in bufs[k][1:])):
                    assert x.tobytes() == y.tobytes(), (m, B, k)
            t0 = time.perf_counter()
            want = [tc.held_karp_layers(d, 0) for d in mats[:4]]
            model_ms = (time.perf_counter() - t0) * 1e3 / len(want)
            for b, w in enumerate(want):
                assert (tc.bits(got[0][b]), list(got[1][b]), int(got[3][b, 0]), int(got[3][b, 1])) == (tc.bits(w[0]), w[1], w[2], w[3]), (m, B, b)
            for bs in bufs.values():
                for b in bs:
                    b.free()
            lib = float(np.median(ms["lib"]))
            print(f"| {m} | {B} | " + " | ".join(med(ms[k]) for k in names) + f" | {B / lib:.1f} | {model_ms:.1f} |", flush=True)
            out_rows.append(dict(m=m, B=B, ms=ms, model_ms=model_ms))
    for e in engines.values():
        e.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out_rows, f, indent=1)


if __name__ == "__main__":
    main()
