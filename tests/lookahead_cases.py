"""Cases for the MPA look-ahead (pf_mpa_iter_ahead / pf_mpa_ahead_take) and a model of what a run must do.

No GPU here: the maps, the run table, the oracle's runs (acceptance counts, curve, best, longest candidate per iteration) and
`schedule`, which turns an acceptance list into the run's steps (single sweep / leading sweep of depth D / served from a
level / stale level, then a sweep) and the four totals of Engine.mpa_ahead_stats().  tests/test_lookahead_cases.py pins the
model's output; tests/test_gpu_mpa_lookahead_paths.py holds the device to it exactly.

The model restates the take rule on its own: a waiting level is served iff the level applied before it accepted nothing, no
level up to it overflowed and nothing else has been set up or swept on the handle since; a refused take of a level that is
there counts one stale level and drops the rest; the history gets STALE either way.  Only the depth of a sweep comes from
pathfit.mpa.lookahead_depth (tests/test_mpa_lookahead_policy.py is its test).
"""
import collections
import os
import sys

import numpy as np

import golden_io as gio

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

# bench.py's MPA parameters, for pathfit.MPA and for pf_loops.MpaOracle
KW = dict(FADs_rate=0.2, P_const=0.5, levy_beta=2.0, turn_penalty_factor=0.1, safety_penalty_factor=0.8, min_safe_distance=1.8,
          diagonal_obstacle_penalty=100.0)
OKW = dict(FADs_rate=0.2, P_const=0.5, levy_beta=2.0, w_turn=0.1, w_safe=0.8, min_safe=1.8, diag_pen=100.0)
# move policy -> (allow_diagonal_moves, restrict_diagonal_near_obstacle)
POLICIES = {"8": (1, 1), "4": (0, 1), "cut": (1, 0)}
AHEAD_MAX = 16                                              # PF_AHEAD_MAX


# ------------------------------------------------------------------------------------------------------------------ maps
def door_map():
    """16 x 24, free except column 12: a wall with one free cell at row 8.  Start 0, target 383."""
    g = np.zeros((16, 24), np.uint8)
    g[:, 12] = 1
    g[8, 12] = 0
    g[0, 0], g[15, 23] = 2, 3
    return g, 0, 383


def open12_map():
    """12 x 12 without obstacles.  Start 0, target 143."""
    g = np.zeros((12, 12), np.uint8)
    g[0, 0], g[11, 11] = 2, 3
    return g, 0, 143


def grid(name):
    """-> (grid with the cell values 0 / 1 / 2 / 3, start cell, target cell)"""
    if name == "door":
        return door_map()
    if name == "open12":
        return open12_map()
    return gio.grid(name)


# ------------------------------------------------------------------------------------------------------------- run table
Run = collections.namedtuple("Run", "map N K seed cap always policy")
RUNS = {
    # a: levels of another phase than their leader's are served and accept (iterations 17 and 33)
    "door16": Run("door", 20, 48, 0, 16, 0, "8"),
    # c: nothing ever accepts -- every level is served, full depth, truncation at the run's end; D N no multiple of 64, N = 1
    "open65": Run("open12", 65, 48, 0, 16, 0, "8"),
    "open5": Run("open12", 5, 48, 0, 16, 0, "8"),
    "open1": Run("open12", 1, 40, 3, 16, 0, "8"),
    "open5_cap2": Run("open12", 5, 48, 0, 2, 0, "8"),
    "open5_cap1": Run("open12", 5, 48, 0, 1, 0, "8"),
    # d: looking ahead after every iteration -- most levels are thrown away
    "fig7_s0_16": Run("fig7", 70, 48, 0, 16, 1, "8"),
    "fig7_s0_5": Run("fig7", 70, 48, 0, 5, 1, "8"),
    "fig7_s1_16": Run("fig7", 70, 48, 1, 16, 1, "8"),
    "fig7_s1_5": Run("fig7", 70, 48, 1, 5, 1, "8"),
}
# b: door under the other two move policies; the seed is first_quiet_seed(...) (pinned in the host test)
POLICY_SEEDS = {"4": 0, "cut": 0}


def policy_run(policy):
    return Run("door", 20, 48, POLICY_SEEDS[policy], 16, 0, policy)


# ---------------------------------------------------------------------------------------------------------- oracle runs
class _Lengths:
    """An Oracle that also notes, per iteration, the longest row a device sweep would have to hold: every search result, the
    two stitched searches of a FADs detour (before duplicates are dropped) and every rebuilt phase candidate."""

    def __init__(self, orc):
        self._o, self.it, self.longest, self._p1 = orc, 0, collections.defaultdict(int), 0

    def __getattr__(self, name):
        return getattr(self._o, name)

    def _note(self, n):
        self.longest[self.it] = max(self.longest[self.it], int(n))

    def astar(self, start, target, avoid=None, variant=0):
        p, st = self._o.astar(start, target, avoid, variant)
        if avoid is None:
            self._p1 = len(p)
            self._note(len(p))
        elif len(p):
            self._note(self._p1 - 1 + len(p))               # second leg of a detour, stitched behind the first
        return p, st

    def mpa_rebuild(self, *a):
        out, isnew, tc, st = self._o.mpa_rebuild(*a)
        if isnew:
            self._note(len(out))
        return out, isnew, tc, st


OracleRun = collections.namedtuple("OracleRun", "acc curve best longest")
_REF = {}


def oracle_run(map_name, N, K, seed, policy="8"):
    """The oracle's run -> (predators changed per iteration 1..K, curve, best (cells, stats), longest row per iteration)."""
    key = (map_name, N, K, seed, policy)
    if key not in _REF:
        import pf_loops
        import pf_oracle as po
        from probe_mpa_acceptance import acceptance_rows
        g, s, t = grid(map_name)
        ad, rs = POLICIES[policy]
        orc = _Lengths(po.Oracle(g, ad, rs))
        ref = pf_loops.MpaOracle(orc, s, t, N, K, seed=seed, restrict=rs, **OKW)
        orc.it = 1                                           # (the constructor's search, the initial path, is row 0)
        rows = acceptance_rows(ref, progress=lambda r: setattr(orc, "it", r[0] + 1))
        _REF[key] = OracleRun([r[2] for r in rows], list(ref.curve), ref.best, [orc.longest[it] for it in range(K + 1)])
    return _REF[key]


def run_oracle(run):
    return oracle_run(run.map, run.N, run.K, run.seed, run.policy)


def quiet_pair_before_end(acc):
    return any(acc[i] == 0 and acc[i + 1] == 0 for i in range(len(acc) - 2))


def first_quiet_seed(map_name, N, K, policy, seeds=range(16)):
    """The first seed whose run has two quiet iterations in a row before K (so that a level is served), or None."""
    for seed in seeds:
        if quiet_pair_before_end(oracle_run(map_name, N, K, seed, policy).acc):
            return seed
    return None


# ---------------------------------------------------------------------------------------------------------------- model
class Handle:
    """What one Engine remembers of the look-ahead: the levels that wait, whose they are, the four totals."""

    def __init__(self, cap, always=False):
        self.cap, self.always = min(int(cap), AHEAD_MAX) if cap >= 0 else 8, bool(always)
        self.waiting = None                                  # [owner, iterations still waiting, acceptances of the level applied last]
        self.owner = None                                    # the instance set up last
        self.merged_sweeps = self.levels_ahead = self.served = self.stale = 0

    def totals(self):
        return dict(merged_sweeps=self.merged_sweeps, levels_ahead=self.levels_ahead, served=self.served, stale=self.stale)


class Instance:
    """One solo MPA on a Handle: its acceptance list (the oracle's), its history and the steps it took."""

    def __init__(self, handle, acc, K, overflow_at=None):
        from pathfit.mpa import STALE, lookahead_depth
        self.STALE, self.depth_of = STALE, lookahead_depth
        self.h, self.acc, self.K, self.overflow_at = handle, list(acc), K, overflow_at
        self.hist, self.left, self.steps, self.launches, self.leaders = [], 0, [], [], []

    def step(self, it):
        """Iteration `it` -> its label; None once the iteration that overflows has raised."""
        h = self.h
        if h.owner is not self:                              # another instance was set up in between: its set-up dropped the levels
            h.owner, h.waiting = self, None
        label, took = "", False
        if h.cap > 0 and self.left > 0:
            w = h.waiting
            if w is not None and w[1]:
                current = w[0] is self and w[2] == 0 and w[1][0] == it and \
                    not (self.overflow_at is not None and self.overflow_at <= it)
                if current:
                    took = True
                    w[1].pop(0)
                    w[2] = self.acc[it - 1]
                    self.left -= 1
                    h.served += 1
                else:
                    h.stale += 1
                    h.waiting = None
            if not took:
                self.left = 0
                self.hist.append(self.STALE)
                label = "stale+"
        if took:
            label = "served"
        else:
            d = self.depth_of(self.hist, h.cap, self.K - it + 1, h.always)
            h.waiting = None                                 # any sweep forgets the levels of the one before
            if self.overflow_at == it:
                self.steps.append(label + "overflow")
                self.launches.append(1)
                return None
            if d > 1:
                h.merged_sweeps += 1
                h.levels_ahead += d - 1
                h.waiting = [self, list(range(it + 1, it + d)), self.acc[it - 1]]
                self.leaders.append(it)
                label += "lead(%d)" % d
            else:
                label += "single"
            self.left = max(d - 1, 0)
        self.hist.append(self.acc[it - 1])
        self.steps.append(label)
        self.launches.append(0 if took else 1)
        return label


Schedule = collections.namedtuple("Schedule", "steps totals launches history leaders")


def schedule(acc, cap, K, always=False, overflow_at=None):
    """What a run of K iterations with the acceptance list `acc` must do under "mpa_lookahead" = cap: per step one of
    "single", "lead(D)", "served", "stale+single", "stale+lead(D)" (and "...overflow" for the step that raises, the last);
    the totals merged_sweeps / levels_ahead / served / stale; the mpa_sweep launches per step; the acceptance history with
    its STALE marks; the iterations that led a merged sweep."""
    h = Handle(cap, always)
    m = Instance(h, acc, K, overflow_at)
    for it in range(1, K + 1):
        if m.step(it) is None:
            break
    return Schedule(m.steps, h.totals(), m.launches, m.hist, m.leaders)


def run_schedule(run, overflow_at=None):
    return schedule(run_oracle(run).acc, run.cap, run.K, bool(run.always), overflow_at)


def served_iterations(sched):
    return [it for it, s in enumerate(sched.steps, 1) if s == "served"]


def leader_of(sched, it):
    """The iteration that led the merged sweep iteration `it` was served from."""
    assert sched.steps[it - 1] == "served"
    return max(l for l in sched.leaders if l < it)


def phase_of(it, K):
    return 1 if it <= K / 3 else (2 if it <= 2 * K / 3 else 3)


# ---------------------------------------------------------------------------------------------- overflow in a level ahead
Overflow = collections.namedtuple("Overflow", "map N K seed cap path_cap at leader")


def find_overflow_case(maps=(("door", 20), ("fig7", 70)), seeds=range(32), K=48, cap=16):
    """The first (map, seed, path_cap P) for which the first row longer than P, in the oracle's run, belongs to an iteration
    that the model places at a level >= 1 of a merged sweep (whose level 0 then does not overflow: it comes before).  P is
    at least the initial path's length, so that the population itself fits.  None if there is none."""
    for name, N in maps:
        for seed in seeds:
            o = oracle_run(name, N, K, seed)
            base = schedule(o.acc, cap, K)
            for P in sorted(set(o.longest[1:])):
                P = P - 1                                    # one cell short of some iteration's longest row
                if P < o.longest[0] or P < 2:
                    continue
                at = next(it for it in range(1, K + 1) if o.longest[it] > P)
                if base.steps[at - 1] == "served":
                    return Overflow(name, N, K, seed, cap, P, at, leader_of(base, at))
    return None


# ------------------------------------------------------------------------------------------- two instances on one handle
def interleave(K, burst=3):
    """The order two instances are stepped in: `burst` iterations of A, `burst` of B, and so on -> [(who, it)]."""
    out = []
    for lo in range(1, K + 1, burst):
        for who in "AB":
            out += [(who, it) for it in range(lo, min(lo + burst, K + 1))]
    return out


def schedule_two(acc_a, acc_b, cap, K, burst=3):
    """Two solo MPAs on one Engine, stepped as interleave(K, burst) -> (instance A, instance B, totals)."""
    h = Handle(cap)
    inst = {"A": Instance(h, acc_a, K), "B": Instance(h, acc_b, K)}
    for who, it in interleave(K, burst):
        inst[who].step(it)
    return inst["A"], inst["B"], h.totals()
