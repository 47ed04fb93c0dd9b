"""Turn fields (pf_turn_field) per (map, policy, turn weight): the kernel ms and the work counters of one field from one source, against
(a) pf_cost_field on the same handle at turn weight 0 and (b) a host heap Dijkstra over the states -- for the shipped tile geometry and
for candidate geometries built into libraries of their own and loaded into the same process.

    python scripts/probe_turn_field.py [--maps fig7,g256,up4,open1400,serp255] [--policies "1,1"] [--weights 0,0.3,3] [--reps 3]
                                       [--host-weights 0.3] [--geometries 32x16,64x16] [--json OUT]

Per (map, policy, turn weight), after one untimed run of everything, `reps` repeats alternating in one process, median (min ... max):
  field    pf_turn_field, one set of one source (the first free cell), no cost map, with d_info: pf_last_kernel_ms (HIP events round
           the whole call: the fills, the seeds, every round with the host's queue-length read, the info kernels) and
           pf_turn_field_work's launches / tile visits / state words lowered (these depend on the schedule)
  (a)      pf_cost_field over a map of ones on the same handle, kernel ms; at turn weight 0 `best` and its rows are compared and must
           be bit-equal (asserted)
  (b)      the wall ms of tests/turn_checkers.dijkstra_fast (a Python heap over the states), run ONCE for the weights of --host-weights
           (it is the slow side); its labels are compared with the device's and must be equal (asserted)
  geometry one column per candidate: the same field from lib/probe/libpathfit_tf<TW>x<TH>.so (built here on first use with
           -DPF_TF_TW / -DPF_TF_TH, build.py's flags otherwise) on a handle of its own, alternating with the shipped one; its states
           must equal the shipped build's bit for bit (asserted)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from probe_clearance import clear_map  # noqa: E402
from probe_dist_field import med  # noqa: E402


def geometry_lib(geo):
    """lib/probe/libpathfit_tf<geo>.so, built on first use."""
    import build
    tw, th = (int(v) for v in geo.split("x"))
    out = os.path.join(PKG, "lib", "probe", f"libpathfit_tf{geo}.so")
    if build._stale(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(build._cmd(out, [f"-DPF_TF_TW={tw}", f"-DPF_TF_TH={th}"]))
    return out


def engine_on(path, g):
    """An Engine whose calls go to the library at `path` (a second build in this process)."""
    import pathfit
    from pathfit import _lib
    L = ctypes.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    keep, _lib._LIB = _lib._LIB, L
    try:
        return pathfit.Engine(g)
    finally:
        _lib._LIB = keep


class Run:
    def __init__(self, e, g, src):
        self.e, RC = e, g.size
        self.off, self.ids = np.array([0, 1], np.int32), np.array([src], np.int32)
        self.states, self.best, self.info = e.buf(8 * RC, np.float64), e.buf(RC, np.float64), e.buf(4, np.int64)

    def field(self, wt, ad, rs):
        self.e.turn_field(None, wt, self.off, self.ids, self.states, self.best, ad, rs, self.info)
        return self.e.last_kernel_ms(), self.e.turn_field_work()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="fig7,g256,up4,open1400,serp255")
    ap.add_argument("--policies", default="1,1")
    ap.add_argument("--weights", default="0,0.3,3")
    ap.add_argument("--host-weights", default="0.3")
    ap.add_argument("--geometries", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    import field_checkers as fc
    import turn_checkers as tk
    policies = [tuple(int(v) for v in p.split(",")) for p in a.policies.split(";")]
    weights = [float(v) for v in a.weights.split(",")]
    host_weights = [float(v) for v in a.host_weights.split(",")] if a.host_weights else []
    geos = [v for v in a.geometries.split(",") if v]
    libs = {geo: geometry_lib(geo) for geo in geos}
    rows = []
    print("| map | policy | w_t | largest best | field, kernel ms | launches / tile visits / state words lowered | (a) pf_cost_field, kernel ms | field / (a) | "
          "(b) host heap, wall ms | (b) / field |" + "".join(f" {geo}: kernel ms; launches / visits |" for geo in geos))
    print("|---|---|---|---|---|---|---|---|---|---|" + "---|" * len(geos))
    for name in a.maps.split(","):
        g = clear_map(name)
        R, C = g.shape
        RC = g.size
        src = int(np.flatnonzero(g.reshape(-1) != 1)[0])
        e = pathfit.Engine(g)
        main_run = Run(e, g, src)
        alts = {geo: Run(engine_on(path, g), g, src) for geo, path in libs.items()}
        ones, cout = e.put(np.ones(RC)), e.buf(RC, np.float64)
        for ad, rs in policies:
            mm = fc.move_masks(g, ad, rs)
            for wt in weights:
                def cost_field():
                    e.cost_field(ones, main_run.off, main_run.ids, cout, ad, rs)
                    return e.last_kernel_ms()

                main_run.field(wt, ad, rs), cost_field(), [r.field(wt, ad, rs) for r in alts.values()]   # untimed: code objects, scratch
                F, W, M, G = [], [], [], {geo: [] for geo in geos}
                for _ in range(a.reps):
                    ms, work = main_run.field(wt, ad, rs)
                    F.append(ms)
                    W.append(work)
                    M.append(cost_field())
                    for geo, r in alts.items():
                        G[geo].append(r.field(wt, ad, rs))
                T, best = main_run.states.download(), main_run.best.download()
                if wt == 0.0:
                    assert np.array_equal(best.view(np.uint64), cout.download().view(np.uint64)), (name, ad, rs, "best differs from the cost field's rows")
                for geo, r in alts.items():
                    assert np.array_equal(r.states.download().view(np.uint64), T.view(np.uint64)), (name, ad, rs, wt, geo, "the geometries disagree")
                host_ms = None
                if wt in host_weights:
                    t0 = time.perf_counter()
                    hT = tk.dijkstra_fast(g, mm, None, [src], wt)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    assert np.array_equal(hT.reshape(-1).view(np.uint64), T.view(np.uint64)), (name, ad, rs, wt, "labels differ from the host's")
                far = int(main_run.info.download()[2])
                wk = " / ".join(f"{int(np.median([w[i] for w in W]))}" for i in range(3))
                rows.append(dict(map=name, shape=[R, C], policy=[ad, rs], turn_weight=wt, largest=float(best[far]) if far >= 0 else None, field_ms=F,
                                 work=[list(w) for w in W], cost_field_ms=M, host_ms=host_ms,
                                 geometries={geo: dict(ms=[x[0] for x in v], work=[list(x[1]) for x in v]) for geo, v in G.items()}))
                alt = "".join(f" {med([x[0] for x in v])}; {int(np.median([x[1][0] for x in v]))} / {int(np.median([x[1][1] for x in v]))} |" for v in G.values())
                print(f"| {name} {R}x{C} | {ad},{rs} | {wt:g} | {best[far] if far >= 0 else float('nan'):.1f} | {med(F)} | {wk} | {med(M)} | "
                      f"{np.median(F) / np.median(M):.2f} | {'-' if host_ms is None else f'{host_ms:.0f}'} | "
                      f"{'-' if host_ms is None else f'{host_ms / np.median(F):.0f}'} |" + alt, flush=True)
        for r in alts.values():
            r.e.close()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
