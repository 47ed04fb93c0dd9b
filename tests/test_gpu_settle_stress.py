"""The rare paths of the parallel closed-set engine (pf_settle.h) against the oracle: tests/settle_cases.py run on the shipped library
and on the five stress variants of build.py's SETTLE_VARIANTS (lib/stress/, built by __graft_entry__.build()), whose band geometry
makes those paths common and whose branch counters (-DPF_OPEN_PATHS, pf_selftest_settle_paths) say which of them a run reached.  The
program itself compares every search with the oracle and balances the books of every launch (settled + sequential = the searches that
reach the engine, derived on the CPU; the branch counters against both); this module adds what each build promises.

Every parameter starts ONE fresh child process and waits for it; nothing is retried.  If a child ends by a signal, by an abort,
without its result line or at its time limit, the parameters after it skip themselves: nothing more is started on a GPU that may have faulted.

The time limit is a hang guard, not a pass criterion: the `default` child took MEASURED_DEFAULT_S = 3.4 s on an MI355X (process start,
HIP initialisation and the CPU oracle dominate); every child gets 20 times that, and no less than 120 s.

Counters no build can reach (EXEMPT, asserted to stay zero).
`cone_goal`: the goal's label is the offer of an expanded neighbour p, fl(g(p) + c); h(p) is exactly c (1, or the correctly rounded
sqrt(2) the move costs), so f(p) = fl(g(p) + c) = g(goal) = F, and under h = 0 f(p) = g(p) < F: p is expanded, an argmin parent and not
later than the goal, so the regularity pass never marks the goal.
`cone_queue`: the walk's queue is the touched list itself; a cell is queued once (its SEEN bit is claimed atomically), only when it
carries a label of this search, i.e. a successful relaxation logged it, and the main loop has handed the search back if that log ever
outgrew the same capacity.
`back_winners` with one node per lane: 64 nodes x 8 moves fill the list of 512 at most.  With two nodes per lane (st_wide2) 1024 > 768 is
possible in principle and needs more than 6 winning relaxations per node over a whole trip; nothing is promised for it.
`back_range` in every build with Q <= 64: tests/test_settle_cases.py::test_band_range_argument (a push asks for band bcur + 245 at
most, of 256)."""
import json
import os
import subprocess
import sys
import time

import pytest

import settle_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "maaco-path-planing_amd", "lib")
CASES = os.path.join(ROOT, "tests", "settle_cases.py")
MEASURED_DEFAULT_S = 3.4            # the `default` child on an MI355X, wall seconds; a variant took at most 3.6
LIMIT_S = max(120.0, 20.0 * MEASURED_DEFAULT_S)
EXEMPT = ("cone_goal", "cone_queue")
# what each variant's row of build.py's table promises, as counters that must be non-zero in that variant.  Every build runs the
# one-search launches that exhaust slot 0's label epoch.
PROMISED = {
    "st_cap4": ("wipe", "trips", "back_bucket", "back"),
    # bands of exact labels between 64 K and 1024 (test_settle_cases.py::test_band_histograms): the Dijkstra searches take parts of
    # bands, never fill a bucket, and so reach every exit of the engine: bound, exhaustion (the sealed pairs), the short row
    "st_q1": ("wipe", "trips", "take_part", "take_many", "superseded", "stop_bound", "stop_empty", "unreached", "all_regular", "row_short"),
    "st_q96": ("wipe", "trips", "back_range", "back"),
    # ... and both outcomes of the cone walk among the searches that fit its touched list (test_settle_cases.py::test_pairs_hold_all_three_outcomes_of_the_certificate)
    "st_touch": ("wipe", "trips", "back_touched", "back", "take_one", "take_many", "stop_bound", "all_regular", "irregular", "cone_ok", "cone_ancestor"),
    "st_wide2": ("wipe", "trips", "take_part", "stop_bound", "stop_empty", "unreached", "all_regular"),
}
_results = {}
_stopped = []                        # why no further child is started


def lib_of(name):
    return os.path.join(LIBDIR, "libpathfit.so") if name == "default" else os.path.join(LIBDIR, "stress", "libpathfit_%s.so" % name)


def exempt_in(name):
    geo = sc.geometry(name)
    return EXEMPT + (("back_range",) if geo["Q"] <= 64.0 else ()) + (("back_winners",) if geo["WIDE"] == 1 else ())


@pytest.mark.parametrize("name", ["default"] + sc.VARIANT_NAMES)
def test_settle_cases_vs_oracle(name):
    if _stopped:
        pytest.skip("not started: " + _stopped[0])
    assert os.path.exists(lib_of(name)), "build the stress variants first (__graft_entry__.build())"
    env = dict(os.environ, PF_LIB=lib_of(name))
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, CASES, name], env=env, timeout=LIMIT_S, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        _stopped.append("the %s child did not end within %.0f s" % (name, LIMIT_S))
        pytest.fail(_stopped[0])
    if r.returncode < 0 or r.returncode in (134, 139):
        _stopped.append("the %s child ended with status %d" % (name, r.returncode))
        pytest.fail(_stopped[0] + "\n" + r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if not lines:                                               # it died on the way (a HIP error surfaces as a Python exception, status 1)
        _stopped.append("the %s child ended with status %d and no result line" % (name, r.returncode))
        pytest.fail(_stopped[0] + "\n" + r.stdout[-2000:] + r.stderr[-2000:])
    out = json.loads(lines[-1])
    print(lines[-1])
    print("child wall seconds: %.1f (limit %.0f)" % (time.time() - t0, LIMIT_S))
    assert out["variant"] == name and out["lib"] == os.path.basename(lib_of(name))
    assert out["mismatches"] == 0 and r.returncode == 0, out["notes"]
    fams = out["families"]
    assert set(fams) == {"astar", "decode", "exact_fit"} and all(f["searches"] > 0 and f["reached"] > 0 for f in fams.values())
    assert all(f["settled"] + f["sequential"] == f["reached"] for f in fams.values())
    _results[name] = out
    a = fams["astar"]
    assert a["epoch_falls"] == 1 and a["short_back_touched"] == 0
    assert all(z["searches"] == len(sc.olc.SEALED) * sum(1 for m in sc.olc.MAP_NAMES for v, _, _ in sc.astar_runs(m) if str(v) == k) for k, z in a["sealed"].items())
    geo = sc.geometry(name)
    if geo == sc.SHIPPED:
        # the shipped geometry: nothing is handed back for want of room, and with h = 0 nothing else hands a search back
        for f in fams.values():
            assert f["totals"].get("2", [0, 0, 0])[2] == 0, f["totals"]
        z = a["sealed"]["2"]
        assert z["settled"] == z["searches"] and z["sequential"] == 0
        # A*: both outcomes of the certificate occur (the measured share is in DESIGN.md 4.3, not asserted)
        reached, settled, sequential = a["totals"]["0"]
        assert 0 < sequential < reached and settled > 0, a["totals"]
    if name == "default":
        assert out["counters"] is None                          # the shipped build carries no counters
        return
    c = out["counters"]
    assert list(c) == sc.COUNTERS
    for k in exempt_in(name):
        assert c[k] == 0, (name, k, c[k])
    for k in PROMISED[name]:
        assert c[k] > 0, (name, k, c)
    assert a["by_variant"]["2"]["irregular"] == 0 and fams["exact_fit"]["counters"]["row_short"] <= 2 * sc.FIT_CASES
    for k, z in a["sealed"].items():                            # every sealed search left by the engine's own exit or was handed back
        assert z["unreached"] + z["back"] == z["searches"] and z["sequential"] == z["back"], (k, z)


def test_every_branch_counter_is_reached_somewhere():
    if _stopped:
        pytest.skip("not all children ran: " + _stopped[0])
    assert set(_results) == {"default"} | set(sc.VARIANT_NAMES), "run the whole module: the coverage is taken over all variants"
    for k in sc.COUNTERS:
        hits = [v for v in sc.VARIANT_NAMES if _results[v]["counters"][k] > 0]
        if k in EXEMPT:
            assert not hits, (k, hits)
        elif k == "back_winners":                               # reachable in principle with two nodes per lane only; nothing is promised
            assert set(hits) <= {"st_wide2"}, (k, hits)
            print("back_winners:", {v: _results[v]["counters"][k] for v in sc.VARIANT_NAMES})
        elif k == "back_range":
            assert hits == ["st_q96"], (k, hits)
        else:
            assert hits, k
