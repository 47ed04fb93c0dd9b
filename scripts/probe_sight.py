"""The sight graph: pf_sight_pack and pf_sight_field on the device against the host's heap Dijkstra over the same graph.

    python scripts/probe_sight.py [--maps fig7,seed64,seed128,g256corners] [--reps 3] [--hbm SO] [--model-sets 2] [--json OUT]

Per map and B in (1, 64): the kernel ms of pf_sight_pack (once per map: it does not depend on B) and of pf_sight_field with its parents
(HIP events, pf_last_kernel_ms), the rounds and candidate sums the field took (pf_sight_field_work), and the wall ms of the model of
tests/sight_checkers.py -- a heap Dijkstra over the device's own adjacency bits with the same fp64 sums -- on the same source sets.
The model is the yardstick, not a competitor: it is single-threaded Python over numpy.  At B = 64 the model runs the first
--model-sets sets only (the rest would take minutes on the larger maps) and its wall ms is scaled to 64 sets; the column says so.
--hbm names a second build loaded into the SAME process, the form with the labels of a set in the output row instead of LDS
(lib/stress/libpathfit_sg_hbm.so, which build.py --variants makes, switches at 65 nodes: every map here runs its HBM form); default:
that file when it exists.  Forms and the model alternate `reps` times after one untimed run of each, all on one device; the
tables give the median and min .. max.  Every output of every form is compared as bytes, and the labels with the model's words.
nodes = "free" on fig7, on a seeded 64 x 64 map (8 % obstacles) and on a seeded 128 x 128 map (12 %: at most 16 384 free cells by
construction); "corners" on g256 (1 587 corner cells)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from probe_dist_field import med  # noqa: E402
from probe_smooth import second_engine  # noqa: E402


def make(name):
    """-> (grid, node cells)"""
    import sight_checkers as sc
    from pathfit import env
    if name == "fig7":
        import golden_io as gio
        g = gio.grid("fig7")[0]
        return g, sc.free_nodes(g)
    if name.startswith("seed"):
        n = int(name[4:])
        g = (np.random.default_rng(n).random((n, n)) < (0.08 if n <= 64 else 0.12)).astype(np.uint8)
        return g, sc.free_nodes(g)
    if name == "g256corners":
        g = np.array(env.g256())
        return g, sc.corner_nodes(g)
    raise SystemExit(f"unknown map {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="fig7,seed64,seed128,g256corners")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm", default=None)
    ap.add_argument("--model-sets", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    import sight_checkers as sc
    hbm = a.hbm or os.path.join(PKG, "lib", "stress", "libpathfit_sg_hbm.so")
    hbm = hbm if os.path.exists(hbm) else None
    rows = []
    print("| map | M | set bits | B | pack ms | field ms, labels in LDS | field ms, labels in HBM | rounds (most of a set) | candidate sums | model wall ms | model sets run |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g, nodes = make(name)
        M, ld, C = len(nodes), (len(nodes) + 63) // 64, g.shape[1]
        if M > 16384:
            print(f"| {name} | {M} | - | - | does not fit 16 384 nodes | | | | | | |")
            continue
        e = pathfit.Engine(g)
        eh = second_engine(hbm, g) if hbm else None
        dadj, dinfo = e.buf((M, ld), np.uint64), e.buf(4, np.int64)
        dadj_h = eh.buf((M, ld), np.uint64) if eh else None

        def pack(eng, buf):
            eng.sight_pack(nodes, buf, ld, True, -1, dinfo if eng is e else None)
            return eng.last_kernel_ms()

        pack(e, dadj)
        if eh:
            pack(eh, dadj_h)
        P = [pack(e, dadj) for _ in range(a.reps)]
        words = dadj.download().reshape(M, ld)
        same = eh is None or words.tobytes() == dadj_h.download().tobytes()
        adj = sc.unpack_bits(words, M)[0]
        w = sc.RowWeights(nodes, C)
        usable = np.flatnonzero(np.diag(adj))
        for B in (1, 64):
            src = np.random.default_rng(B).choice(usable, B, replace=B > len(usable)).astype(np.int32)
            off = np.arange(B + 1, dtype=np.int32)
            out = {f: (eng.buf((B, M), np.float64), eng.buf((B, M), np.int32), eng.buf((B, 4), np.int64)) for f, eng in (("lds", e), ("hbm", eh)) if eng}

            def field(f):
                eng, abuf = (e, dadj) if f == "lds" else (eh, dadj_h)
                eng.sight_field(nodes, abuf, ld, off, src, *out[f])
                return eng.last_kernel_ms()

            def model(k):
                t0 = time.perf_counter()
                d = [sc.dijkstra(adj, w, [int(s)]) for s in src[:k]]
                return (time.perf_counter() - t0) * 1e3, np.array(d)

            k = B if B == 1 else min(B, a.model_sets)
            for f in out:
                field(f)
            T, Tm = {f: [] for f in out}, []
            for _ in range(a.reps):
                for f in out:
                    T[f].append(field(f))
                ms, md = model(k)
                Tm.append(ms * B / k)
            got = {f: [b.download() for b in out[f]] for f in out}
            agree = same and all(x.tobytes() == y.tobytes() for f in out for x, y in zip(got[f], got["lds"]))
            agree = agree and got["lds"][0].reshape(B, M)[:k].view(np.uint64).tobytes() == md.view(np.uint64).tobytes()
            work = e.sight_field_work()
            row = dict(map=name, M=M, bits=int(adj.sum()), B=B, pack_ms=P, field_lds_ms=T["lds"], field_hbm_ms=T.get("hbm", []), rounds=work[0], sums=work[2],
                       model_wall_ms=Tm, model_sets=k, agree=bool(agree))
            rows.append(row)
            print(f"| {name} | {M} | {row['bits']} | {B} | {med(P)} | {med(T['lds'])} | {med(T['hbm']) if eh else '-'} | {work[0]} | {work[2]} | {med(Tm)} | "
                  f"{k} of {B}{' (scaled)' if k < B else ''} |" + ("" if agree else " OUTPUTS DISAGREE"), flush=True)
            for f in out:
                for b in out[f]:
                    b.free()
        for b in (dadj, dinfo, dadj_h):
            if b is not None:
                b.free()
        if eh:
            eh.close()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    if not all(r["agree"] for r in rows):
        raise SystemExit("outputs disagree")


if __name__ == "__main__":
    main()
