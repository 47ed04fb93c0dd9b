"""pf_dist_field_batch against the host Dijkstra that builds the same tables (the MPA bound tables of pf_mpa_batch_create).

    python scripts/probe_dist_field.py [--maps g128crop,up2,up4,open1024,serp256] [--ks 1,2,32] [--policy 1,1] [--reps 3] [--json OUT]

Per (map, policy, K) and repeat, alternating in ONE process:
  kernel ms    HIP events around the distance-field kernel (pf_last_kernel_ms) of one launch for the K sources, with levels and
               list appends from d_info (max and sum over the sources);
  host ms      create_ms[1] ("bound tables") of a pf_mpa_batch_create whose schools' distinct cells are exactly the K sources, option
               "mpa_bounds_device" 0: K host Dijkstras one after another, each with its host-to-device copy;
  device ms    the same create with the option 1: one launch into the batch's rows, host wall time.
Every cell is warmed by one untimed launch and one untimed create of each kind.  The table gives the median and min .. max of the
repeats.  Sources: the two corner markers, then seeded free cells.  The serpentine map (every other row a wall with one gap, at
alternating ends) is the worst case of the level count: about R C / 2 levels."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maaco-path-planing_amd")]
import numpy as np  # noqa: E402


def make_map(name):
    from pathfit import env
    if name == "g128crop":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import golden_io as gio
        g = gio.grid("g128crop")[0].copy()
        g[(g == 2) | (g == 3)] = 0
        return g
    if name.startswith("up"):
        g = np.array(env.bench_grid(256 * int(name[2:])))
        g[(g == 2) | (g == 3)] = 0
        return g.astype(np.uint8)
    if name.startswith("open"):
        n = int(name[4:])
        return np.zeros((n, n), np.uint8)
    if name.startswith("serp"):
        n = int(name[4:])
        g = np.zeros((n, n), np.uint8)
        for i, r in enumerate(range(1, n, 2)):
            g[r, :] = 1
            g[r, n - 1 if i % 2 == 0 else 0] = 0
        return g
    raise SystemExit(f"unknown map {name}")


def sources_of(g, K):
    flat = g.reshape(-1)
    out = [c for c in (0, g.size - 1) if flat[c] != 1][:K]
    free = np.flatnonzero(flat != 1)
    rnd = np.random.default_rng(4000 + K)
    while len(out) < K:
        c = int(rnd.choice(free))
        if c not in out:
            out.append(c)
    return np.array(out, np.int32)


def create_tables_ms(e, src, ad, rs, device):
    """create_ms[1] of a batch of ceil(K / 2) one-predator schools whose distinct start / target cells are `src`"""
    from pathfit._lib import MpaParams
    from pathfit.engine import score_params
    from pathfit.mpa import levy_sigma
    K = len(src)
    starts = np.ascontiguousarray(src[0::2], np.int32)
    targets = np.ascontiguousarray([src[i + 1] if i + 1 < K else src[i] for i in range(0, K, 2)], np.int32)
    seeds = np.arange(len(starts), dtype=np.uint64)
    sp = score_params(1)
    mp = MpaParams(0.5, 1.5, levy_sigma(1.5), 0.2, 1, int(starts[0]), int(targets[0]), int(ad), int(rs))
    e.set_option("mpa_bounds_device", device)
    b = C.c_void_p()
    try:
        e._ck(e.L.pf_mpa_batch_create(e.h, C.byref(mp), C.byref(sp), len(starts), starts.ctypes.data, targets.ctypes.data, seeds.ctypes.data, C.byref(b)))
    finally:
        e.set_option("mpa_bounds_device", 0)
    out = np.zeros(3)
    e.L.pf_mpa_batch_create_ms(b, out.ctypes.data)
    e.L.pf_mpa_batch_destroy(b)
    return float(out[1])


def med(v):
    return f"{np.median(v):.3f} ({min(v):.3f} … {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="g128crop,up2,up4,open1024,serp256")
    ap.add_argument("--ks", default="1,2,32")
    ap.add_argument("--policy", default="1,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    ad, rs = (int(v) for v in a.policy.split(","))
    rows = []
    print("| map | policy | K | kernel ms | levels max / sum | appends sum | cells reached sum | host tables ms (option 0) | device tables ms (option 1) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = make_map(name)
        e = pathfit.Engine(g)
        for K in (int(v) for v in a.ks.split(",")):
            src = sources_of(g, K)
            out, info = e.buf((K, g.size), np.float64), e.buf((K, 4), np.int64)
            e.dist_field_batch(src, out, ad, rs, info)                    # warm-up: code object, level lists
            create_tables_ms(e, src, ad, rs, 0)
            create_tables_ms(e, src, ad, rs, 1)
            kms, hms, dms = [], [], []
            for _ in range(a.reps):
                e.dist_field_batch(src, out, ad, rs, info)
                kms.append(e.last_kernel_ms())
                hms.append(create_tables_ms(e, src, ad, rs, 0))
                dms.append(create_tables_ms(e, src, ad, rs, 1))
            inf = info.download()
            out.free(), info.free()
            row = dict(map=name, shape=list(g.shape), policy=[ad, rs], K=K, kernel_ms=kms, host_ms=hms, device_ms=dms,
                       levels_max=int(inf[:, 0].max()), levels_sum=int(inf[:, 0].sum()), reached=int(inf[:, 1].sum()),
                       offered=int(inf[:, 2].sum()), appends=int(inf[:, 3].sum()))
            rows.append(row)
            print(f"| {name} {g.shape[0]}x{g.shape[1]} | ({ad}, {rs}) | {K} | {med(kms)} | {row['levels_max']} / {row['levels_sum']} | {row['appends']} | "
                  f"{row['reached']} | {med(hms)} | {med(dms)} |", flush=True)
        e.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
