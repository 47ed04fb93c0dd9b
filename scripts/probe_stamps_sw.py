"""Diagnostic (-DPF_STAMPS build): shader-clock time per section of a trip of the sorted-window loop, lone wave, and of the floods and
the parent walk around the loop.  `sweep [predators [iterations [pops]]]` (a -DPF_STAMPS -DPF_TRACE build): the same two for the long
items of real sweeps of the bench configuration."""
import sys, os, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maaco-path-planing_amd"), os.path.join(ROOT, "tests")]
import numpy as np
from pathfit import _lib
_lib._SO = os.environ.get("PF_STAMPS_LIB") or os.path.join(ROOT, "maaco-path-planing_amd", "lib", "libpathfit_stamps.so")   # (A/B: another stamps build)
import golden_io as gio
from pathfit.engine import Engine
g = gio.upsample(gio.grid("g256")[0], 2)
e = Engine(g)
e.L.pf_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
e.L.pf_debug_stamps_fw.argtypes = [C.c_void_p, C.c_void_p, C.c_int]


def fw_line(fw, whole, what):
    """Floods and parent walk of astar() (pf_astar.h: FW_*) against `whole` shader clocks of the searches or items they belong to."""
    fl, fr, wk, wc, wr = (float(fw[i]) for i in range(5))
    return (f"      {what}: floods {fl:.0f} clocks = {100 * fl / whole:.2f} % ({fr:.0f} rounds, {fl / max(fr, 1):.0f} clocks a round); "
            f"walk + reverse {wk:.0f} clocks = {100 * wk / whole:.2f} % ({wc:.0f} cells in {wr:.0f} rounds, {wk / max(wc, 1):.0f} clocks a cell, "
            f"{wk / max(wr, 1):.0f} a round); together {100 * (fl + wk) / whole:.2f} % of {whole:.0f} clocks")


def sweep(n_pred, iters, long_pops):
    """One real sweep per iteration of the bench configuration (a build with -DPF_STAMPS -DPF_TRACE): the items of at least
    `long_pops` pops from the item table, their floods and walks against their own shader clocks."""
    sys.path.insert(0, ROOT)
    import pathfit, bench
    from pathfit import env
    from pathfit.dist import Comm, ShardedMPA
    grid = env.bench_grid(512)
    eng = pathfit.Engine(grid)
    eng.L.pf_debug_trace.argtypes = [C.c_void_p, C.c_void_p]
    eng.L.pf_debug_trace_fw.argtypes = [C.c_void_p, C.c_void_p]
    sm = ShardedMPA(Comm(), lambda n: pathfit.MPA(grid, n_pred, 15, engine=eng, seed=0, n_local=n, **bench.MPA_MAIN), n_pred)
    for it in range(1, iters + 1):
        sm.step(it)
        tr, fw = np.zeros(12 * 16384, np.uint64), np.zeros(8 * 16384, np.uint64)
        eng.L.pf_debug_trace(eng.h, tr.ctypes.data)
        eng.L.pf_debug_trace_fw(eng.h, fw.ctypes.data)
        t = tr[: 4 * 16384].reshape(-1, 4)[: 2 * n_pred].astype(np.int64)
        fw = fw.reshape(-1, 8)[: 2 * n_pred].astype(np.int64)
        long_ = (t[:, 1] > 0) & (t[:, 2] >= long_pops)
        ms = (t[long_, 1] - t[long_, 0]) / 1e5
        print(f"iter {it}: kernel {eng.last_kernel_ms():.1f} ms; items of at least {long_pops} pops: {long_.sum()}, "
              f"{ms.mean():.2f} ms each (longest {ms.max():.2f}), {fw[long_, 7].mean():.0f} shader clocks each, searches that reached the loop {fw[long_, 6].sum()}")
        print(fw_line(fw[long_, :5].sum(0), float(fw[long_, 7].sum()), "all of them"))
        worst = np.flatnonzero(long_)[np.argmax(ms)]
        print(fw_line(fw[worst, :5], float(fw[worst, 7]), f"the longest (item {worst}, {t[worst, 2]} pops)"))


if len(sys.argv) > 1 and sys.argv[1] == "sweep":     # probe_stamps_sw.py sweep [predators [iterations [pops of a long item]]]
    a = [int(v) for v in sys.argv[2:]] + [4096, 1, 78000][len(sys.argv) - 2:]
    sweep(*a)
    sys.exit(0)
names = ["refill", "heads+address+load issue", "wait for the loads", "relax+viol+chain", "meta/record stores+pool atomic", "window inserts", "pool stores+tail"]
for n in ((int(sys.argv[1]),) if len(sys.argv) > 1 else (1,)):
    rnd = np.random.default_rng(1)
    free = np.flatnonzero(g.reshape(-1) != 1)
    starts = rnd.choice(free, n).astype(np.int32); targets = rnd.choice(free, n).astype(np.int32)
    starts[0], targets[0] = 0, g.size - 1
    if os.environ.get("PF_SAME"):      # n copies of the corner-to-corner search (shader clocks per trip under load)
        starts[:] = 0; targets[:] = g.size - 1
    for v in (1, 0):
        out, fw = np.zeros(24, np.uint64), np.zeros(8, np.uint64)
        e.L.pf_debug_stamps(e.h, out.ctypes.data, 1)
        e.L.pf_debug_stamps_fw(e.h, fw.ctypes.data, 1)
        paths, st, cnt = e.astar_host(v, starts, targets, None, path_cap=8192, want_counters=True)
        e.L.pf_debug_stamps(e.h, out.ctypes.data, 1)
        e.L.pf_debug_stamps_fw(e.h, fw.ctypes.data, 1)
        trips = int(out[7]); pops = int(cnt[:, 0].sum())
        print(f"us per trip (kernel time / trips of one search) {1e3 * e.last_kernel_ms() / (trips / n):.3f}")
        print(f"n={n} v{v}: {e.last_kernel_ms():.1f} ms pops {pops} trips {trips} pops/trip {pops / trips:.2f} clocks/trip {out[:7].sum() / trips:.0f}: " +
              "; ".join(f"{names[i]} {out[i] / trips:.0f}" for i in range(7)))
        if fw[6] > 0:
            print(fw_line(fw, float(fw[5]), f"outside the pop loop, {int(fw[6])} searches, clocks of the whole astar() calls"))
        if out[23] > 0:     # rotated trips: their load goes out in the tail of the trip before; their pool appends are in the "pool" column
            print(f"      rotated trips: {int(out[23])} of {trips} ({100.0 * out[23] / trips:.1f} %), rotated issue site (heads + addresses + load issue) "
                  f"{out[22] / out[23]:.0f} clocks each = {out[22] / trips:.0f} per trip on top of the columns above")
        c = out[8:16].astype(float); er = out[16:22].astype(float)
        if er[0] > 0:
            print(f"      early refills: {int(er[0])} (every {trips / er[0]:.1f} trips), entries avg {er[1] / er[0]:.1f}, buckets avg {er[3] / er[0]:.1f}, largest bucket avg {er[2] / er[0]:.1f}; "
                  f"clocks per early refill: waiting for the pool entries {er[4] / er[0]:.0f}, sort {er[5] / er[0]:.0f}")
        print(f"      refills: front small {int(c[0])} (avg {c[1] / max(c[0], 1):.1f}), front big {int(c[2])} (avg size {c[3] / max(c[2], 1):.1f}), "
              f"regular {int(c[6])} (avg {c[7] / max(c[6], 1):.1f}), regular big {int(c[4])} (avg size {c[5] / max(c[4], 1):.1f})")
