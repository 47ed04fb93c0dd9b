"""Widest-path fields (pf_clearance_widest) per (map, policy): the kernel ms and the work counters of one field from one source,
against (a) what one PAIR costs today and (b) one pf_components call and one pf_dist_field_merged row on the same map.

    python scripts/probe_widest.py [--maps fig7,g256,up4,dense4096,open4096,serp256] [--policies "1,1;0,1"] [--reps 3] [--other SO] [--json OUT]

Per (map, policy), after one untimed run of everything, `reps` repeats alternating in one process on one handle, median (min … max):
  field    pf_clearance_widest, one set of one source (the free cell furthest from any obstacle), with d_info: pf_last_kernel_ms (HIP
           events round the whole call, the host's queue-length reads between the launches included) and
           pf_clearance_widest_work's launches / tile visits / words raised (these depend on the schedule)
  other    with --other, the same call on a second build of the library loaded into the SAME process (-DPF_WD_ROW_SCAN=0: neighbour
           sweeps alone, without the wave-wide row scan); the rows and the info words are compared
  (a)      the largest margin_sq of ONE pair (that source, the last free cell) as a user finds it today: a bisection over margin_sq
           in [1, min(d2[source], d2[target])], each step Clearance.inflated (numpy on the downloaded field) + Engine.update_grid +
           Components.refresh + Components.same; wall ms of the whole bisection and the steps it took.  Its answer is compared with
           the field's word for the target.
  (b)      pf_components (labels and info) and pf_dist_field_merged (one set of that source), kernel ms each
The clearance field is computed with the border off; the open map carries one obstacle in a corner."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG, os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from probe_clearance import clear_map  # noqa: E402
from probe_dist_field import med  # noqa: E402
from probe_smooth import second_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="fig7,g256,up4,dense4096,open4096,serp256")
    ap.add_argument("--policies", default="1,1;0,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--other", default=None, help="a second build of the library")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import pathfit
    policies = [tuple(int(v) for v in p.split(",")) for p in a.policies.split(";")]
    rows = []
    print("| map | policy | w[target] | field, kernel ms | launches / tile visits / words raised | other build, kernel ms | its launches / visits / words | (a) one pair today, wall ms | (a) steps | field / (a) | "
          "(b) pf_components, kernel ms | (b) pf_dist_field_merged, kernel ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name in a.maps.split(","):
        g = clear_map(name)
        R, C = g.shape
        RC = g.size
        e = pathfit.Engine(g)
        cl = pathfit.Clearance(g, engine=e)
        d2 = cl.d2.reshape(-1)
        src = int(cl.info[3])
        tgt = int(np.flatnonzero(d2 >= 1)[-1])
        sc, tc = (src // C, src % C), (tgt // C, tgt % C)
        off, ids = np.array([0, 1], np.int32), np.array([src], np.int32)
        wbuf, ibuf, lab, cinfo = e.buf(RC, np.int32), e.buf(4, np.int64), e.buf(RC, np.int32), e.buf(4, np.int64)
        dist, dinfo = e.buf(RC, np.float64), e.buf(4, np.int64)
        e2 = second_engine(a.other, g) if a.other else None
        if e2:
            d2o, wo, io = e2.put(cl.d2.reshape(-1), np.int32), e2.buf(RC, np.int32), e2.buf(4, np.int64)
        for ad, rs in policies:
            comp = pathfit.Components(g, ad, rs, engine=e)

            def field():
                e.clearance_widest(cl.d2_device, off, ids, wbuf, ad, rs, ibuf)
                return e.last_kernel_ms(), e.clearance_widest_work()

            def other():
                e2.clearance_widest(d2o, off, ids, wo, ad, rs, io)
                return e2.last_kernel_ms(), e2.clearance_widest_work()

            def todays():
                """-> (wall ms, steps, the answer); the engine holds the original map again afterwards."""
                t0 = time.perf_counter()
                lo, hi, steps = 0, int(min(d2[src], d2[tgt])), 0
                while lo < hi:
                    mid = (lo + hi + 1) // 2
                    e.update_grid(cl.inflated(margin_sq=mid))
                    comp.refresh()
                    ok = bool(comp.same([(sc, tc)])[0])
                    steps += 1
                    lo, hi = (mid, hi) if ok else (lo, mid - 1)
                ms = (time.perf_counter() - t0) * 1e3
                e.update_grid(g)
                return ms, steps, lo

            def others():
                e.components(lab, ad, rs, cinfo)
                c = e.last_kernel_ms()
                e.dist_field_merged(off, ids, dist, ad, rs, dinfo)
                return c, e.last_kernel_ms()

            field(), todays(), others()                               # untimed: code objects, scratch
            if e2:
                other()
            F, W, A, S, CC, DD, OF, OW = [], [], [], [], [], [], [], []
            ans = None
            for _ in range(a.reps):
                ms, work = field()
                F.append(ms)
                W.append(work)
                if e2:
                    ms, work = other()
                    OF.append(ms)
                    OW.append(work)
                ms, steps, ans = todays()
                A.append(ms)
                S.append(steps)
                c, d = others()
                CC.append(c)
                DD.append(d)
            wt = int(wbuf.read(tgt, 1)[0])
            ok = wt == ans
            same = not e2 or (np.array_equal(wbuf.download(), wo.download()) and np.array_equal(ibuf.download(), io.download()))
            wk = " / ".join(f"{int(np.median([w[i] for w in W]))}" for i in range(3))
            owk = " / ".join(f"{int(np.median([w[i] for w in OW]))}" for i in range(3)) if OW else "-"
            rows.append(dict(map=name, shape=[R, C], policy=[ad, rs], w_target=wt, field_ms=F, work=[list(w) for w in W], pair_ms=A, pair_steps=S,
                             components_ms=CC, merged_ms=DD, agree=bool(ok), other_ms=OF, other_work=[list(w) for w in OW], other_agrees=bool(same)))
            print(f"| {name} {R}x{C} | {ad},{rs} | {wt} | {med(F)} | {wk} | {med(OF) if OF else '-'} | {owk} | {med(A)} | {int(np.median(S))} | {np.median(F) / np.median(A):.4f} | {med(CC)} | {med(DD)} |"
                  + ("" if ok else f" DISAGREE (bisection {ans})") + ("" if same else " THE BUILDS DISAGREE"), flush=True)
            comp.close()
        if e2:
            e2.close()
        cl.close()
        e.close()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
