"""MPABatch against the same K schools run one after another as solo MPAs: aggregate evals/s = K * N * 20 / wall time of the 20
timed iterations (after 5 warm-up iterations; every step ends in a host read of the best rows, so the clock stops on a finished
sweep), the search kernel's share of a sweep (HIP events around k_mpa_search), and what pf_mpa_batch_create costs.

    python scripts/probe_mpa_batch.py [--configs 512:1:4096,512:2:4096,512:4:1024,512:16:256,128:16:256] [--reps 3]
                                      [--solo-lib PATH] [--json OUT]

Every measurement runs in a fresh child process (a process loads one library), batch and solo alternating, `--reps` times each:
the table gives the median and the min .. max of the repeats.  --solo-lib names the library the solo runs load (PF_LIB): give it
a build of the PARENT commit to measure the batch against what the project did before (the yardstick of DESIGN.md 4.7); without
it the solo runs use the current build.  School 0 runs between the map's markers (the mpa512 bench workload), the others between
seeded random free cells.

For the kernel split run one role under `rocprofv3 --kernel-trace --stats -- python scripts/probe_mpa_batch.py --role batch
--config 512:2:4096`."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maaco-path-planing_amd")]
import numpy as np  # noqa: E402

KW = dict(FADs_rate=0.2, P_const=0.5, levy_beta=1.5)        # main.py's MPA settings
WARM, TIMED = 5, 20


def pairs(g, K):
    rnd = np.random.default_rng(1000 + K)
    free = np.argwhere(g != 1)
    s0, t0 = (tuple(int(v) for v in np.argwhere(g == m)[0]) for m in (2, 3))
    out = [(s0, t0)]
    while len(out) < K:
        i, j = rnd.choice(len(free), 2, replace=False)
        out.append((tuple(int(v) for v in free[i]), tuple(int(v) for v in free[j])))
    return out


def moved(g, s, t):
    h = np.array(g, dtype=int)
    h[(h == 2) | (h == 3)] = 0
    h[s], h[t] = 2, 3
    return h


def timed_steps(obj, eng):
    """5 warm-up + 20 timed iterations -> (wall seconds of the timed ones, mean search-kernel ms per timed sweep)"""
    for it in range(1, WARM + 1):
        obj.step(it)
    kms = []
    t0 = time.perf_counter()
    for it in range(WARM + 1, WARM + TIMED + 1):
        obj.step(it)
        kms.append(eng.last_kernel_ms())
    return time.perf_counter() - t0, float(np.mean(kms))


def child(role, size, K, N):
    if role == "solo":
        # (a parent-commit library has no pf_mpa_batch_* symbols: the solo runs do not need them)
        import ctypes
        from pathfit import _lib
        so = ctypes.CDLL(_lib.so_path())
        for name in [n for n in _lib.SYMBOLS if n.startswith("pf_mpa_batch_") and not hasattr(so, n)]:
            del _lib.SYMBOLS[name]
    import pathfit
    from pathfit import env
    g = env.bench_grid(size)
    eng = pathfit.Engine(g)
    pr = pairs(g, K)
    iters = WARM + TIMED
    out = dict(role=role, size=size, K=K, N=N, lib=os.path.basename(pathfit._lib.so_path()))
    if role == "batch":
        b = pathfit.MPABatch(g, N, iters, seeds=list(range(K)), starts=[p[0] for p in pr], targets=[p[1] for p in pr], engine=eng, **KW)
        out["create_ms"] = b.create_ms()
        b.begin()
        wall, kms = timed_steps(b, eng)
        out.update(wall_s=wall, search_ms_per_sweep=kms, sweeps=TIMED)
        out["fitness"] = [b.school(k).best_fitness_overall for k in range(K)]
    else:
        wall, kms, fit = 0.0, [], []
        for k, (s, t) in enumerate(pr):                             # one after another on one engine, each set up in turn
            m = pathfit.MPA(moved(g, s, t), N, iters, seed=k, engine=eng, **KW)
            w, km = timed_steps(m, eng)
            wall += w
            kms.append(km)
            fit.append(m.best_fitness_overall)
        out.update(wall_s=wall, search_ms_per_sweep=float(np.mean(kms)), sweeps=TIMED * K, fitness=fit)
    out["evals_per_s"] = K * N * TIMED / out["wall_s"]
    eng.close()
    print("PROBE " + json.dumps(out), flush=True)


def spawn(role, cfg, solo_lib):
    envv = dict(os.environ)
    if role == "solo" and solo_lib:
        envv["PF_LIB"] = os.path.abspath(solo_lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", role, "--config", cfg], env=envv, capture_output=True,
                       text=True, timeout=900)
    for line in p.stdout.splitlines():
        if line.startswith("PROBE "):
            return json.loads(line[6:])
    raise RuntimeError(f"{role} {cfg} failed (exit {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="512:1:4096,512:2:4096,512:4:1024,512:16:256,128:16:256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solo-lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--role", default=None, choices=["batch", "solo"])
    ap.add_argument("--config", default=None)
    a = ap.parse_args()
    if a.role:
        size, K, N = (int(v) for v in a.config.split(":"))
        return child(a.role, size, K, N)
    rows = []
    for cfg in a.configs.split(","):
        runs = {"batch": [], "solo": []}
        for _ in range(a.reps):                                      # alternating: both see the same box at the same time
            for role in ("batch", "solo"):
                runs[role].append(spawn(role, cfg, a.solo_lib))
        if runs["batch"][0]["fitness"] != runs["solo"][0]["fitness"]:
            raise RuntimeError(f"{cfg}: the batch and the solo runs found different best fitnesses")
        r = dict(config=cfg, runs=runs)
        for role in ("batch", "solo"):
            v = sorted(x["evals_per_s"] for x in runs[role])
            r[role] = dict(median=float(np.median(v)), lo=v[0], hi=v[-1],
                           search_ms_per_sweep=float(np.median([x["search_ms_per_sweep"] for x in runs[role]])),
                           ms_per_sweep=float(np.median([1e3 * x["wall_s"] / x["sweeps"] for x in runs[role]])))
        r["speedup"] = r["batch"]["median"] / r["solo"]["median"]
        r["create_ms"] = runs["batch"][0]["create_ms"]
        rows.append(r)
        size, K, N = cfg.split(":")
        print(f"G{size} K={K:>2} x {N:>4}: batch {r['batch']['median'] / 1e3:7.1f} k evals/s ({r['batch']['lo'] / 1e3:.1f} .. {r['batch']['hi'] / 1e3:.1f})  "
              f"solo x K [{runs['solo'][0]['lib']}] {r['solo']['median'] / 1e3:7.1f} k ({r['solo']['lo'] / 1e3:.1f} .. {r['solo']['hi'] / 1e3:.1f})  "
              f"x{r['speedup']:.2f} | sweep ms batch {r['batch']['ms_per_sweep']:.2f} (search {r['batch']['search_ms_per_sweep']:.2f}) "
              f"solo {r['solo']['ms_per_sweep']:.2f} (search {r['solo']['search_ms_per_sweep']:.2f}) | create ms "
              f"{r['create_ms'][2]:.0f} (paths {r['create_ms'][0]:.0f}, bounds {r['create_ms'][1]:.0f})", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
