"""How many candidates does an MPA iteration accept?  The CPU probe behind the look-ahead of DESIGN.md 4.9 (oracle only, no GPU).

    python scripts/probe_mpa_acceptance.py [--grid 512] [--predators 4096] [--iterations 20] [--seed 0] [--upto K] [--json OUT]
    python scripts/probe_mpa_acceptance.py --map door --predators 20 --iterations 48      (a small map of tests/lookahead_cases.py)

Runs oracle/pf_loops.MpaOracle (bit-exact with the device by the parity tests) on the mpa512 bench workload by default (G512,
4 096 predators, K = 20, seed 0, bench.py's MPA_MAIN parameters) and prints, per iteration:
  searching   items whose gates let them search at all (a phase item whose gate draw passes, a FADs item that is drawn --
              detour or re-initialisation; the device prunes some of the former and memoises the latter);
  accepted    predators that end the iteration as another individual (phase candidate through the memory step, or FADs);
  distinct    distinct fitness values in the population after the iteration.
An iteration with accepted = 0 leaves the population, the list order and the elite untouched: the next iteration's sweep could
have run with it.  The full-size run takes a long time on one core (every predator is up to two A* searches on 512 x 512).
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maaco-path-planing_amd"), os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402

MPA_MAIN = dict(FADs_rate=0.2, P_const=0.5, levy_beta=2.0, w_turn=0.1, w_safe=0.8, min_safe=1.8, diag_pen=100.0)   # bench.py MPA_MAIN


def searching(ref, it, CF):
    """Items of iteration `it` whose gating draws pass, on the population as sorted at its start (replays the draws only)."""
    import pf_loops
    L, o = ref.L, ref.o
    phase = 1 if it <= ref.K / 3 else (2 if it <= 2 * ref.K / 3 else 3)
    elite_len = len(ref.pop[0][0])
    n = 0
    for i in range(ref.N):
        if phase == 1:
            modL, gate = len(ref.pop[i][0]), ref.P
        elif phase == 2:
            levy = i < ref.N // 2
            modL, gate = (len(ref.pop[i][0]), ref.P) if levy else (elite_len, ref.P * CF)
        else:
            modL, gate = elite_len, ref.P * CF
        if modL > 1:
            g = o.rng(ref.seed, pf_loops.DOM_MPA, it, i)
            L.orc_rng_randint(C.byref(g), 0, modL - 2)
            n += L.orc_rng_random(C.byref(g)) < gate
        g = o.rng(ref.seed, pf_loops.DOM_MPA_FADS, it, i)
        n += L.orc_rng_random(C.byref(g)) < ref.fads_rate
    return int(n)


def acceptance_rows(ref, upto=None, progress=None):
    """Step `ref` (an MpaOracle that has not run yet) through iterations 1 .. upto -> [(it, searching, accepted, distinct)]."""
    rows = []
    ref._sort()
    ref.best = ref.pop[0]
    ref.curve.append(ref.best[1][4])
    for it in range(1, (upto or ref.K) + 1):
        ratio = it / ref.K
        CF = 0.0 if ratio >= 1.0 else (1.0 - ratio) ** (2.0 * ratio)
        ref._sort()
        s = searching(ref, it, CF)
        before = list(ref.pop)                           # (kept alive: identity below must not meet a recycled id)
        ids = {id(x) for x in before}
        ref.step(it)
        accepted = sum(id(x) not in ids for x in ref.pop)
        row = (it, s, int(accepted), len({float(x[1][4]) for x in ref.pop}))
        rows.append(row)
        if progress:
            progress(row)
    return rows


def quiet_runs(rows):
    """Longest run of consecutive iterations with accepted == 0, and the first iteration of the first such run (or None)."""
    best = cur = 0
    first = None
    for it, _, acc, _ in rows:
        cur = cur + 1 if acc == 0 else 0
        if cur == 1 and first is None:
            first = it
        best = max(best, cur)
    return best, first


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=512, choices=[128, 256, 512, 1024])
    ap.add_argument("--map", default="", choices=["", "door", "open12", "fig7"],
                    help="a small map of tests/lookahead_cases.py instead of the bench grid (the look-ahead tests' cases)")
    ap.add_argument("--predators", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--upto", type=int, default=0, help="stop after this iteration (default: the whole run)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import pf_loops
    import pf_oracle as po
    from pathfit import env
    if a.map:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import lookahead_cases
        g, s, t = lookahead_cases.grid(a.map)
    else:
        g = env.bench_grid(a.grid)
        s, t = (int(np.flatnonzero(g.reshape(-1) == m)[0]) for m in (2, 3))
    ref = pf_loops.MpaOracle(po.Oracle(g), s, t, a.predators, a.iterations, seed=a.seed, **MPA_MAIN)
    print("| it | searching | accepted | distinct fitness values after it |\n|---|---|---|---|", flush=True)
    rows = acceptance_rows(ref, a.upto or None, lambda r: print("| %d | %d | %d | %d |" % r, flush=True))
    longest, first = quiet_runs(rows)
    print(f"longest run of quiet iterations: {longest}; first quiet iteration: {first}")
    if a.json:
        json.dump(dict(grid=a.grid, predators=a.predators, iterations=a.iterations, seed=a.seed, rows=rows), open(a.json, "w"))


if __name__ == "__main__":
    main()
