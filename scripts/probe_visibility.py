"""Visibility fields against the pairwise line-of-sight call they replace, and the exposure counts against summed masks.

    python scripts/probe_visibility.py [--maps g128crop,up2,up4,open1024] [--reps 3] [--wave SO] [--loop SO] [--count-k 1024] [--json OUT]

Table 1, per map: pf_visibility_field for one viewpoint (the free cell nearest the centre) and for K = 64 seeded free viewpoints, in
the library's own form (a lane per target) and, with --wave, in the form of a second build loaded into the SAME process (a library
built with -DPF_VIS_WAVE_PER_TARGET=1 -DPF_VIS_COUNT_PER=0: a wavefront per target, and a count kernel whose threads walk a chunk of the
viewpoints each, the viewpoints split until about 2^20 threads exist);
the baseline pf_line_of_sight_batch over the R C pairs of the one viewpoint on the same handle, its kernel ms and, apart, the wall ms of
building and uploading the pairs; the cells seen; and the major indices examined (from the baseline's first blockers: the blocker's
major offset + 1, or span + 1 for a seen target, 0 for the free early answers).  Table 2: pf_visibility_count at K = --count-k against
the same viewpoints through pf_visibility_field in slices of 64 (the kernel ms summed; the sum of the masks itself is not counted),
and the count kernel's other forms (the library's own is one atomic per seen pair): --wave's chunk form and, with --loop, a build
with -DPF_VIS_COUNT_PER=1000000 (a plain loop over all viewpoints per cell).  `build` for --wave / --loop compiles them into lib/ab/ first.  Forms alternate `reps` times after one
untimed run of each, all on one device; kernel ms are HIP events (pf_last_kernel_ms); the tables give the median and min .. max.
Every form's output is compared with the library's (they must be equal)."""
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

FORMS = {"wave": ["-DPF_VIS_WAVE_PER_TARGET=1", "-DPF_VIS_COUNT_PER=0"], "loop": ["-DPF_VIS_COUNT_PER=1000000"]}


def so_of(form):
    return os.path.join(PKG, "lib", "ab", f"libpathfit_vis_{form}.so")


def build_form(form):
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    os.makedirs(os.path.dirname(so_of(form)), exist_ok=True)
    subprocess.check_call(mod._cmd(so_of(form), FORMS[form]))
    return so_of(form)


def examined(g, a, vis, fb):
    """Major indices a lane-per-target walk examines from viewpoint a, from the pair kernel's answers."""
    R, C = g.shape
    rr, cc = np.mgrid[0:R, 0:C]
    span = np.maximum(np.abs(rr - a[0]), np.abs(cc - a[1])).reshape(-1)
    colmaj = (np.abs(cc - a[1]) >= np.abs(rr - a[0])).reshape(-1)
    f = np.where(fb >= 0, fb, 0)
    off = np.where(colmaj, np.abs(f % C - a[1]), np.abs(f // C - a[0]))
    walk = np.where(vis != 0, span + 1, off + 1)
    walk[g.reshape(-1) == 1] = 0                                       # a target on an obstacle: no walk
    return int(walk.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="g128crop,up2,up4,open1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wave", default=None)
    ap.add_argument("--loop", default=None)
    ap.add_argument("--count-k", type=int, default=1024)
    ap.add_argument("--count-maps", default="g128crop,up2,up4")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    sos = {f: (build_form(f) if v == "build" else v) for f, v in (("wave", a.wave), ("loop", a.loop))}
    rows = []
    print("| map | field K=1 ms | field K=64 ms | pair call ms (R C pairs) | pair build + upload wall ms | wave-per-target K=1 ms | wave-per-target K=64 ms | "
          "cells seen | major indices examined |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = make_map(name)
        R, C = g.shape
        RC = R * C
        free = np.flatnonzero(g.reshape(-1) != 1)
        fr, fc = free // C, free % C
        centre = int(free[np.argmin((fr - R // 2) ** 2 + (fc - C // 2) ** 2)])
        views = {1: np.array([centre], np.int32), 64: np.random.default_rng(64).choice(free, 64, replace=False).astype(np.int32)}
        e = pathfit.Engine(g)
        ew = second_engine(sos["wave"], g) if sos["wave"] else None
        seen = {K: [e.buf(K * RC, np.uint8), e.buf(K * RC, np.uint8)] for K in views}
        info = e.buf(4 * 64, np.int64)
        t0 = time.perf_counter()
        dfrom, dto = e.put(np.full(RC, centre, np.int32)), e.put(np.arange(RC, dtype=np.int32))
        upload_ms = (time.perf_counter() - t0) * 1e3
        dvis, dfb = e.buf(RC, np.int32), e.buf(RC, np.int32)

        def field(eng, K, which):
            eng.visibility_field(views[K], seen[K][which], True, -1, info)
            return eng.last_kernel_ms()

        def pairs():
            e.line_of_sight_batch(dfrom, dto, RC, dvis, dfb, True)
            return e.last_kernel_ms()

        field(e, 1, 0), field(e, 64, 0), pairs()                      # untimed: code objects, scratch
        if ew:
            field(ew, 1, 1), field(ew, 64, 1)
        T = {k: [] for k in ("f1", "f64", "pair", "w1", "w64")}
        for _ in range(a.reps):
            T["f1"].append(field(e, 1, 0))
            T["pair"].append(pairs())
            if ew:
                T["w1"].append(field(ew, 1, 1))
            T["f64"].append(field(e, 64, 0))
            if ew:
                T["w64"].append(field(ew, 64, 1))
        m1, vis, fb = seen[1][0].download(), dvis.download(), dfb.download()
        same = np.array_equal(m1, vis.astype(np.uint8))
        if ew:
            same = same and all(np.array_equal(seen[K][0].download(), seen[K][1].download()) for K in views)
        row = dict(map=name, shape=[R, C], field1_ms=T["f1"], field64_ms=T["f64"], pair_ms=T["pair"], pair_upload_wall_ms=upload_ms, wave1_ms=T["w1"],
                   wave64_ms=T["w64"], cells_seen=int(m1.sum()), examined=examined(g, (centre // C, centre % C), vis, fb), agree=bool(same))
        rows.append(row)
        print(f"| {name} {R}x{C} | {med(T['f1'])} | {med(T['f64'])} | {med(T['pair'])} | {upload_ms:.2f} | {med(T['w1']) if ew else '-'} | "
              f"{med(T['w64']) if ew else '-'} | {row['cells_seen']} | {row['examined']} |" + ("" if same else " OUTPUTS DISAGREE"), flush=True)
        for b in [info, dfrom, dto, dvis, dfb] + [x for v in seen.values() for x in v]:
            b.free()
        if ew:
            ew.close()
        e.close()

    K = a.count_k
    print()
    print(f"| map | count K={K} ms | field K={K} ms (slices of 64, summed) | count, a chunk of viewpoints per thread ms | count, plain loop per cell ms | viewpoints per thread of the chunk form | coverage |")
    print("|---|---|---|---|---|---|---|")
    for name in a.count_maps.split(","):
        g = make_map(name)
        R, C = g.shape
        RC = R * C
        free = np.flatnonzero(g.reshape(-1) != 1)
        view = np.random.default_rng(K).choice(free, K, replace=K > len(free)).astype(np.int32)
        engines = {"lib": pathfit.Engine(g)}
        for f in ("wave", "loop"):
            if sos[f]:
                engines[f] = second_engine(sos[f], g)
        e = engines["lib"]
        cnt = {f: e.buf(RC, np.int32) for f in engines}
        info, seen = e.buf(4, np.int64), e.buf(64 * RC, np.uint8)

        def count(f):
            engines[f].visibility_count(view, cnt[f], True, -1, info)
            return engines[f].last_kernel_ms()

        def masks(total=None):
            ms = 0.0
            for i in range(0, K, 64):
                e.visibility_field(view[i:i + 64], seen, True, -1, None)
                ms += e.last_kernel_ms()
                if total is not None:
                    total += seen.download()[:len(view[i:i + 64]) * RC].reshape(-1, RC).sum(axis=0, dtype=np.int32)
            return ms

        total = np.zeros(RC, np.int32)
        masks(total)
        for f in engines:
            count(f)
        T = {f: [] for f in engines}
        M = []
        for _ in range(a.reps):
            for f in engines:
                T[f].append(count(f))
            M.append(masks())
        same = all(np.array_equal(cnt[f].download(), total) for f in engines)
        iv = info.download()
        per = -(-K // min(K, 65535, -(-(1 << 20) // RC)))
        row = dict(map=name, shape=[R, C], K=K, count_ms=T["lib"], masks_ms=M, atomic_ms=T.get("wave", []), loop_ms=T.get("loop", []), per=per,
                   coverage=float(iv[0]) / float(iv[1]), agree=bool(same))
        rows.append(row)
        print(f"| {name} {R}x{C} | {med(T['lib'])} | {med(M)} | {med(T['wave']) if 'wave' in T else '-'} | {med(T['loop']) if 'loop' in T else '-'} | {per} | "
              f"{row['coverage']:.3f} |" + ("" if same else " OUTPUTS DISAGREE"), flush=True)
        for b in list(cnt.values()) + [info, seen]:
            b.free()
        for eng in engines.values():
            eng.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
