"""PSOBatch against the same K swarms run one after another as solo PSOSolvers: wall time per sweep (host clock around a
sweep, which ends in the host's read of the last round's scan record(s); 1 warm-up + 4 timed sweeps), aggregate evals/s = K * N *
4 / wall time of the timed sweeps, the repair rounds per sweep (batch: the max over the swarms = its decode launches; solo x K:
the sum), the decode kernel's time per round (HIP events around the decode launch), and what the initialisation costs
(PSOBatch.begin() against the K solo initialisations).

    python scripts/probe_pso_batch.py [--configs 512:1:2048,512:2:2048,512:4:512,512:16:128,512:64:50,128:16:64] [--reps 3]
                                      [--solo-lib PATH] [--json OUT]

Every measurement runs in a fresh child process (a process loads one library), batch and solo alternating, `--reps` times each:
the table gives the median and the min .. max of the repeats.  --solo-lib names the library the solo runs load (PF_LIB): give it
a build of the PARENT commit to measure the batch against what the project did before (the yardstick of DESIGN.md 4.10); without
it the solo runs use the current build.  Swarm 0 runs between the map's markers (the pso512 bench workload), the others between
seeded random cells that can reach each other.  W = 5, main.py's weights (W_MAIN of bench.py), asynchronous.

For the kernel split run one role under `rocprofv3 --kernel-trace --stats -- python scripts/probe_pso_batch.py --role batch
--config 512:16:128`."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maaco-path-planing_amd")]
import numpy as np  # noqa: E402

KW = dict(num_waypoints_per_particle=5, w=0.7, c1=1.5, c2=1.5, turn_penalty_factor=0.3, safety_penalty_factor=0.8, min_safe_distance=1.8,
          diagonal_obstacle_penalty_value=100.0)
WARM, TIMED = 1, 4
NEW_SYMBOLS = ("pf_pso_update_batch", "pf_pso_scan_batch", "pf_pso_commit_batch")


def reachable_from(g, s):
    """mask of the cells 4-connected to s through free cells (reachable under every move policy)"""
    free = np.asarray(g) != 1
    seen = np.zeros_like(free)
    seen[s] = True
    while True:
        grow = seen.copy()
        grow[1:] |= seen[:-1]; grow[:-1] |= seen[1:]; grow[:, 1:] |= seen[:, :-1]; grow[:, :-1] |= seen[:, 1:]
        grow &= free
        if (grow == seen).all():
            return seen
        seen = grow


def pairs(g, K):
    """the map's markers, then K - 1 seeded random pairs of cells that can reach each other (an unreachable pair would leave
    the batch for a solo run and measure nothing)"""
    rnd = np.random.default_rng(2000 + K)
    s0, t0 = (tuple(int(v) for v in np.argwhere(g == m)[0]) for m in (2, 3))
    free = np.argwhere(reachable_from(g, s0))
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


def child(role, size, K, N):
    if role == "solo":
        # (a parent-commit library has none of the batch's symbols: the solo runs do not need them)
        import ctypes
        from pathfit import _lib
        so = ctypes.CDLL(_lib.so_path())
        for name in [n for n in NEW_SYMBOLS if n in _lib.SYMBOLS and not hasattr(so, n)]:
            del _lib.SYMBOLS[name]
    import pathfit
    from pathfit import env
    g = env.bench_grid(size)
    eng = pathfit.Engine(g)
    pr = pairs(g, K)
    its = WARM + TIMED
    out = dict(role=role, size=size, K=K, N=N, lib=os.path.basename(os.path.dirname(os.path.dirname(pathfit._lib.so_path()))) + "/" +
               os.path.basename(pathfit._lib.so_path()))
    if role == "batch":
        b = pathfit.PSOBatch(g, its, N, seeds=list(range(K)), starts=[p[0] for p in pr], targets=[p[1] for p in pr], engine=eng, **KW)
        t0 = time.perf_counter()
        b.begin()
        init = time.perf_counter() - t0
        kms, wall, rounds = [], 0.0, 0
        for it in range(its):
            eng.klog = []
            t0 = time.perf_counter()
            b.sweep()
            if it >= WARM:
                wall += time.perf_counter() - t0
                kms += [ms for name, ms, _ in eng.klog if name == "decode"]
                rounds += len(eng.klog)
        eng.klog = None
        out.update(wall_s=wall, init_s=init, decode_ms_per_round=float(np.mean(kms)), rounds_per_sweep=rounds / TIMED,
                   init_launches=b.init_launches, fitness=[b.swarm(k).convergence_curve[-1] for k in range(K)], batched=len(b.live))
        b.close()
    else:
        wall, init, kms, fit, rounds = 0.0, 0.0, [], [], 0
        for k, (s, t) in enumerate(pr):                                 # one after another on one engine
            ps = pathfit.PSOSolver(moved(g, s, t), its, N, engine=eng, seed=k, **KW)
            t0 = time.perf_counter()
            ok = ps.begin()
            init += time.perf_counter() - t0
            for it in range(its if ok else 0):
                eng.klog = []
                t0 = time.perf_counter()
                ps.sweep()
                if it >= WARM:
                    wall += time.perf_counter() - t0
                    kms += [ms for name, ms, _ in eng.klog if name == "decode"]
                    rounds += len(eng.klog)
            eng.klog = None
            fit.append(ps.convergence_curve[-1] if ok else float("inf"))
        out.update(wall_s=wall, init_s=init, decode_ms_per_round=float(np.mean(kms)) if kms else 0.0, rounds_per_sweep=rounds / TIMED, fitness=fit)
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
    ap.add_argument("--configs", default="512:1:2048,512:2:2048,512:4:512,512:16:128,512:64:50,128:16:64")
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
            ms = sorted(1e3 * x["wall_s"] / TIMED for x in runs[role])          # ms per sweep of ALL K swarms
            r[role] = dict(median=float(np.median(v)), lo=v[0], hi=v[-1], ms_per_sweep=float(np.median(ms)), ms_lo=ms[0], ms_hi=ms[-1],
                           decode_ms_per_round=float(np.median([x["decode_ms_per_round"] for x in runs[role]])),
                           rounds_per_sweep=float(np.median([x["rounds_per_sweep"] for x in runs[role]])),
                           init_ms=float(np.median([1e3 * x["init_s"] for x in runs[role]])))
        r["speedup"] = r["batch"]["median"] / r["solo"]["median"]
        r["wins"] = r["batch"]["ms_hi"] < r["solo"]["ms_lo"]                   # the batch's slowest repeat beats solo x K's fastest
        rows.append(r)
        size, K, N = cfg.split(":")
        b, s = r["batch"], r["solo"]
        print(f"G{size} K={K:>2} x {N:>4}: batch {b['median'] / 1e3:7.1f} k evals/s ({b['lo'] / 1e3:.1f} .. {b['hi'] / 1e3:.1f})  "
              f"solo x K [{runs['solo'][0]['lib']}] {s['median'] / 1e3:7.1f} k ({s['lo'] / 1e3:.1f} .. {s['hi'] / 1e3:.1f})  x{r['speedup']:.2f} | "
              f"ms / sweep batch {b['ms_per_sweep']:.2f} ({b['ms_lo']:.2f} .. {b['ms_hi']:.2f}; {b['rounds_per_sweep']:.2f} rounds, decode {b['decode_ms_per_round']:.2f} each) "
              f"solo x K {s['ms_per_sweep']:.2f} ({s['ms_lo']:.2f} .. {s['ms_hi']:.2f}; {s['rounds_per_sweep']:.2f} rounds, decode {s['decode_ms_per_round']:.2f} each) | "
              f"init ms batch {b['init_ms']:.0f} solo x K {s['init_ms']:.0f}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
