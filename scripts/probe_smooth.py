"""Any-angle smoothing of M Dijkstra paths (DistanceField.paths' rows, still in HBM) against the kernels that produced them.

    python scripts/probe_smooth.py [--maps g128crop,up2,up4,open1024] [--ms 64,4096] [--reps 3] [--plain SO] [--json OUT]

Per (map, M): one distance field from cell (0, 0) (the first free cell where that one is an obstacle), its parent map, one trace of M
seeded free targets -- the kernel ms of each (HIP events, pf_last_kernel_ms) -- and then pf_smooth_batch over the traced rows where they
lie: its kernel ms in the library's own form and, with --plain, in the form of a second build loaded into the SAME process (a library
built with -DPF_SMOOTH_SPEC=0; `--plain build` compiles it into lib/ab/ first).  The two forms alternate `reps` times after one untimed
run of each and work on the same device buffers; their outputs are compared (they must be equal).  The table gives the median and
min .. max of the repeats, the waypoints kept per path and the major indices examined per path (the sum, over the tests the rule
makes, of the tested segment's span + 1, computed on the host from the kept positions)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from probe_dist_field import make_map, med  # noqa: E402

PLAIN_SO = os.path.join(PKG, "lib", "ab", "libpathfit_smooth_plain.so")


def build_plain():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    os.makedirs(os.path.dirname(PLAIN_SO), exist_ok=True)
    subprocess.check_call(mod._cmd(PLAIN_SO, ["-DPF_SMOOTH_SPEC=0"]))
    return PLAIN_SO


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


def examined(cells, lens, idx, wl, C, sample):
    """Mean over the sampled paths of sum(span + 1) over the tests of the rule, from the kept positions."""
    tot = []
    for i in sample:
        L, k = int(lens[i]), idx[i, :wl[i]]
        if L < 3:
            tot.append(0)
            continue
        r, c = cells[i, :L] // C, cells[i, :L] % C
        n = 0
        for a, nxt in zip(k[:-1], k[1:]):
            j = np.arange(a + 2, min(int(nxt) + 1, L - 1) + 1)
            n += int((np.maximum(np.abs(r[j] - r[a]), np.abs(c[j] - c[a])) + 1).sum())
        tot.append(n)
    return float(np.mean(tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="g128crop,up2,up4,open1024")
    ap.add_argument("--ms", default="64,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain", default=None, help="a library built with -DPF_SMOOTH_SPEC=0, or `build`")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    plain_so = build_plain() if a.plain == "build" else a.plain
    rows = []
    print("| map | M | field ms | parents ms | trace ms | smooth ms (library) | smooth ms (plain build) | smooth / trace | smooth / (field + parents + trace) | "
          "cells per path | waypoints per path | major indices examined per path |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = make_map(name)
        RC, C = g.size, g.shape[1]
        free = np.flatnonzero(g.reshape(-1) != 1)
        e = pathfit.Engine(g)
        e2 = second_engine(plain_so, g) if plain_so else None
        cap = e.default_path_cap()
        f, p = e.buf((1, RC), np.float64), e.buf((1, RC), np.uint8)
        for M in (int(v) for v in a.ms.split(",")):
            tg = np.random.default_rng(7000 + M).choice(free, M, replace=M > len(free)).astype(np.int32)
            dt, dk = e.put(tg), e.put(np.zeros(M, np.int32))
            dc, dl, dst = e.buf((M, cap), np.int32), e.buf(M, np.int32), e.buf(M, np.int32)
            out = [[e.buf((M, cap), np.int32), e.buf((M, cap), np.int32), e.buf(M, np.int32), e.buf((M, 2), np.float64), e.buf(M, np.int32)] for _ in range(2)]

            def front():
                e.dist_field_batch([int(free[0])], f, 1, 1); k0 = e.last_kernel_ms()
                e.dist_field_parents(1, f, p, 1, 1); k1 = e.last_kernel_ms()
                e.dist_field_paths(1, p, dt, M, cap, dc, dl, dst, dk); k2 = e.last_kernel_ms()
                return k0, k1, k2

            def smooth(eng, o):
                eng.smooth_batch(M, cap, dc, dl, cap, o[0], o[2], o[4], o[1], o[3], True)
                return eng.last_kernel_ms()

            front(), smooth(e, out[0])                                 # warm-up: code objects, level lists
            if e2:
                smooth(e2, out[1])
            F, S, P = [], [], []
            for _ in range(a.reps):
                F.append(front())
                S.append(smooth(e, out[0]))
                if e2:
                    P.append(smooth(e2, out[1]))
            got = [b.download() for b in out[0]]
            same = not e2 or all(np.array_equal(x, b.download()) for x, b in zip(got[2:], out[1][2:]))
            if e2 and same:
                other = [b.download() for b in out[1][:2]]
                same = all(np.array_equal(got[j][i, :got[2][i]], other[j][i, :got[2][i]]) for j in (0, 1) for i in range(M))
            cells, lens = dc.download(), dl.download()
            sample = np.random.default_rng(1).choice(M, min(M, 256), replace=False)
            F = np.array(F)
            front_ms = float(np.median(F.sum(axis=1)))
            row = dict(map=name, shape=list(g.shape), M=M, path_cap=cap, field_ms=F[:, 0].tolist(), parents_ms=F[:, 1].tolist(), trace_ms=F[:, 2].tolist(),
                       smooth_ms=S, smooth_plain_ms=P, forms_agree=bool(same), mean_cells=float(lens.mean()), mean_waypoints=float(got[2].mean()),
                       mean_examined=examined(cells, lens, got[1], got[2], C, sample), ok=int((got[4] == 0).sum()))
            rows.append(row)
            print(f"| {name} {g.shape[0]}x{g.shape[1]} | {M} | {med(F[:, 0])} | {med(F[:, 1])} | {med(F[:, 2])} | {med(S)} | {med(P) if P else '-'} | "
                  f"{np.median(S) / np.median(F[:, 2]):.2f} | {np.median(S) / front_ms:.3f} | {row['mean_cells']:.1f} | {row['mean_waypoints']:.1f} | "
                  f"{row['mean_examined']:.0f} |" + ("" if same else " FORMS DISAGREE"), flush=True)
            for b in [dt, dk, dc, dl, dst] + out[0] + out[1]:
                b.free()
        f.free(), p.free()
        if e2:
            e2.close()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
