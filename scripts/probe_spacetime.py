"""Space-time fields: kernel time per (map, policy, horizon, sets), the forms of the field kernel against each other, and the
word-parallel numpy model on the same input.

    python scripts/probe_spacetime.py [--maps fig7,g256,up4] [--policies 1,1;0,1] [--sets 1,8,64] [--reps 5] [--forms hbm,t256,t512] [--json OUT]
    python scripts/probe_spacetime.py build --forms hbm,t256,t512        # compiles the other forms into lib/ab/ (no device needed)

Per row: pf_spacetime_field with the reach planes written and, apart, with d_reach NULL (arrive only), in the library's own form
and in every --forms build loaded into the SAME process: hbm = -DPF_STF_LDS_BYTES=0 (the live planes in HBM on every map), t256 /
t512 = -DPF_STF_THREADS=256 / 512 (smaller workgroups, more words a thread).  The forms alternate `reps` times after one untimed
run of each, all on one device; kernel ms are HIP events (pf_last_kernel_ms); the table gives the median and min .. max, and
ticks / ms of the library's own form.  Every form's arrive, reach words and info are compared with the library's, and the
library's with the numpy model (tests/spacetime_checkers.field_words), whose wall time for ONE set is the last column.  The
planes hold 16 seeded patrols (king walks with waits, half of them parking at their end), stamped by pf_spacetime_stamp."""
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

from probe_dist_field import make_map, med  # noqa: E402
from probe_smooth import second_engine  # noqa: E402

FORMS = {"hbm": ["-DPF_STF_LDS_BYTES=0"], "t256": ["-DPF_STF_THREADS=256"], "t512": ["-DPF_STF_THREADS=512"]}
HORIZON = {"fig7": 64, "g256": 512, "up4": 256}


def so_of(form):
    return os.path.join(PKG, "lib", "ab", f"libpathfit_st_{form}.so")


def build_form(form):
    import importlib.util
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    os.makedirs(os.path.dirname(so_of(form)), exist_ok=True)
    subprocess.check_call(mod._cmd(so_of(form), FORMS[form]))
    return so_of(form)


def map_of(name):
    if name in ("fig7", "g256"):
        import golden_io as gio
        return (gio.grid(name)[0] == 1).astype(np.uint8)
    return (make_map(name) == 1).astype(np.uint8)


def patrol_rows(g, T, n, seed):
    import spacetime_checkers as sc
    R, C = g.shape
    rnd = np.random.default_rng(seed)
    free = np.flatnonzero(g.reshape(-1) != 1)
    rows = []
    for _ in range(n):
        v = int(rnd.choice(free))
        row = [v]
        for _ in range(T):
            k = int(rnd.integers(-1, 8))
            r, c = v // C + (0 if k < 0 else sc.DR[k]), v % C + (0 if k < 0 else sc.DC[k])
            if 0 <= r < R and 0 <= c < C and g[r, c] != 1:
                v = r * C + c
            row.append(v)
        rows.append(np.array(row, np.int32))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", nargs="?", default="run")
    ap.add_argument("--maps", default="fig7,g256,up4")
    ap.add_argument("--policies", default="1,1;0,1")
    ap.add_argument("--sets", default="1,8,64")
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
    import spacetime_checkers as sc
    out_rows = []
    names = ["lib"] + forms
    print("| map | policy | T | B | " + " | ".join(f"{n} ms" for n in names) + " | lib, arrive only ms | ticks / ms (lib) | cells reached, set 0 | numpy model, one set, wall ms |")
    print("|---" * (8 + len(names)) + "|")
    for name in a.maps.split(","):
        g = map_of(name)
        R, C = g.shape
        T = HORIZON.get(name, 256)
        engines = {"lib": pathfit.Engine(g)}
        for f in forms:
            engines[f] = second_engine(so_of(f), g)
        rows = patrol_rows(g, T, 16, 7)
        host = pathfit.SpaceTime(g, T, engine=engines["lib"])
        host.add(rows[::2], after_end="stay").add(rows[1::2], after_end="vanish", corners=True)
        Dw = host.occupancy()
        Dw = sc.pack(Dw)
        host.close()
        free = np.flatnonzero(g.reshape(-1) != 1)
        W = R * ((C + 63) // 64)
        for pol in a.policies.split(";"):
            ad, rs = (int(v) for v in pol.split(","))
            for B in (int(v) for v in a.sets.split(",")):
                src = np.random.default_rng(B).choice(free, B).astype(np.int32)
                off = np.arange(B + 1, dtype=np.int32)
                bufs, ms, ms_a = {}, {n: [] for n in names}, []
                for n, e in engines.items():
                    bufs[n] = (e.put(Dw), e.buf((B, R * C), np.int32), e.buf((B, T + 1, W), np.uint64), e.buf((B, 4), np.int64))
                for rep in range(a.reps + 1):
                    for n, e in engines.items():
                        occ, da, dr, di = bufs[n]
                        e.spacetime_field(T, occ, off, src, da, bool(ad), bool(rs), dr, di)
                        if rep:
                            ms[n].append(e.last_kernel_ms())
                    e = engines["lib"]
                    e.spacetime_field(T, bufs["lib"][0], off, src, bufs["lib"][1], bool(ad), bool(rs), None, None)
                    if rep:
                        ms_a.append(e.last_kernel_ms())
                got = [b.download() for b in bufs["lib"][1:]]
                for n in forms:
                    for x, y in zip(got, (b.download() for b in bufs[n][1:])):
                        assert np.array_equal(x, y), (name, pol, B, n)
                t0 = time.perf_counter()
                wa, wr = sc.field_words(g == 1, Dw, [int(src[0])], ad, rs)
                model_ms = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(got[0][0].reshape(R, C), wa) and np.array_equal(got[1][0].reshape(T + 1, R, -1), wr), (name, pol, B)
                for bs in bufs.values():
                    for b in bs:
                        b.free()
                lib = float(np.median(ms["lib"]))
                print(f"| {name} {R}x{C} | {ad},{rs} | {T} | {B} | " + " | ".join(med(ms[n]) for n in names) +
                      f" | {med(ms_a)} | {T / lib:.0f} | {int(got[2][0, 0])} | {model_ms:.1f} |", flush=True)
                out_rows.append(dict(map=name, R=R, C=C, policy=pol, T=T, B=B, ms={n: ms[n] for n in names}, arrive_only_ms=ms_a, model_ms=model_ms))
        for e in engines.values():
            e.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out_rows, f, indent=1)


if __name__ == "__main__":
    main()
