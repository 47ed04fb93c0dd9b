"""MAACOBatch against the same K colonies run one after another as solo MAACOs on one Engine: wall time per iteration
(host clock around iterate_dev, ended by a sync; 2 warm-up, 10 timed iterations) and ant-walks/s, at cfg-2 (G128, 256 ants a
colony) and G512 (1 024 ants a colony), K in {1, 4, 16, 64}.

    python scripts/probe_maaco_batch.py [--sizes 128,512] [--ks 1,4,16,64] [--json OUT]

For the kernel split run it once under `rocprofv3 --kernel-trace --stats -- python scripts/probe_maaco_batch.py ...`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maaco-path-planing_amd")]
import numpy as np  # noqa: E402
import pathfit  # noqa: E402
from pathfit import env  # noqa: E402

KW = dict(alpha=1.0, beta=7.0, rho=0.1, Q=2.5, a_turn_coef=1.0, wh_max=0.9, wh_min=0.2, k_h_adaptive=0.9, q0_initial=0.5,
          C0_initial_pheromone=0.1)        # main.py:34-38
WARM, TIMED = 2, 10


def pairs(g, K):
    """colony 0 runs between the map's markers, the others between seeded random free cells"""
    rnd = np.random.default_rng(K)
    free = np.argwhere(g != 1)
    s0, t0 = (tuple(int(v) for v in np.argwhere(g == m)[0]) for m in (2, 3))
    out = [(s0, t0)]
    while len(out) < K:
        i, j = rnd.choice(len(free), 2, replace=False)
        out.append((tuple(int(v) for v in free[i]), tuple(int(v) for v in free[j])))
    return out


def sync(eng):
    eng._ck(eng.L.pf_sync(eng.h))


def moved(g, s, t):
    h = np.array(g, dtype=int)
    h[(h == 2) | (h == 3)] = 0
    h[s], h[t] = 2, 3
    return h


def run(size, K, n):
    g = env.bench_grid(size)
    eng = pathfit.Engine(g)
    pr = pairs(g, K)
    iters = WARM + TIMED
    b = pathfit.MAACOBatch(g, n, iters, engine=eng, seeds=list(range(K)), starts=[p[0] for p in pr], targets=[p[1] for p in pr], **KW)
    ts = []
    for it in range(1, iters + 1):
        t0 = time.perf_counter()
        b.iterate_dev(it)
        sync(eng)
        ts.append(time.perf_counter() - t0)
    t_batch = float(np.mean(ts[WARM:]))
    b.close()
    # the same colonies one after another as solo MAACOs on one engine (each set up in turn): an iteration of all K costs the sum
    # of the K solo iterations
    t_solo = 0.0
    for k, (s, t) in enumerate(pr):
        m = pathfit.MAACO(moved(g, s, t), n, iters, engine=eng, seed=k, **KW)
        ts = []
        for it in range(1, iters + 1):
            t0 = time.perf_counter()
            m.iterate_dev(it)
            sync(eng)
            ts.append(time.perf_counter() - t0)
        t_solo += float(np.mean(ts[WARM:]))
    eng.close()
    walks = K * n
    return dict(size=size, K=K, ants_per_colony=n, batch_ms=1e3 * t_batch, solo_ms=1e3 * t_solo, speedup=t_solo / t_batch,
                batch_walks_per_s=walks / t_batch, solo_walks_per_s=walks / t_solo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for size in (int(v) for v in a.sizes.split(",")):
        n = {128: 256, 512: 1024}[size]
        for K in (int(v) for v in a.ks.split(",")):
            r = run(size, K, n)
            rows.append(r)
            print(f"G{size} K={K:3d} x {n} ants: batch {r['batch_ms']:8.2f} ms/it  solo x K {r['solo_ms']:8.2f} ms/it  "
                  f"speedup {r['speedup']:5.2f}  walks/s batch {r['batch_walks_per_s'] / 1e6:.3f} M  solo {r['solo_walks_per_s'] / 1e6:.3f} M",
                  flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
