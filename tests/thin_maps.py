"""Thin maps for the thin-grid tests: a side of 1, 2 or 3 cells, built with numpy alone (no fixture file is needed to make one).

`thin_map(R, C, obstacles)` -> (grid with the reference's cell values 0/1/2/3, start cell, target cell).  The start is (0, 0).
An empty map has its target in the opposite corner.  With obstacles, 13 % of the cells (rounded up) are obstacles; on a map at least 9 long
they all lie in the far 45 % of the long axis and the target is the last cell before that zone -- a corridor one to three cells
wide is cut by almost any obstacle, so this keeps one long feasible run (start -> target, more than half the long side) next to
a zone of dead ends, pockets and cut corridors.  The same recipe is captured with the reference's answers in
tests/golden/thin_cases.npz (oracle/capture_golden.py, `thin`), which also stores the grids: tests/test_oracle_thin_grids.py
checks that the stored grid is the one built here."""
import math

import numpy as np

SHAPES = [(1, 2), (2, 1), (1, 9), (9, 1), (2, 2), (3, 3), (2, 17), (17, 2), (3, 200), (200, 3), (3, 700), (700, 3), (1, 300),
          (1, 4096), (4096, 1)]
FRAC = 0.13


def name_of(R, C, obstacles):
    return f"{R}x{C}{'o' if obstacles else 'e'}"


def has_obstacle_version(R, C):
    return R * C >= 4


def all_maps():
    """Every (R, C, obstacles) of the golden file, in its order."""
    return [(R, C, ob) for R, C in SHAPES for ob in (False, True) if not ob or has_obstacle_version(R, C)]


def thin_map(R, C, obstacles=False, seed=0):
    g = np.zeros((R, C), np.uint8)
    s, t = (0, 0), (R - 1, C - 1)
    if obstacles:
        assert has_obstacle_version(R, C)
        L, along_cols = max(R, C), C >= R
        lo = int(math.ceil(0.55 * L)) if L >= 9 else 0
        if lo:
            t = (R - 1, lo - 1) if along_cols else (lo - 1, C - 1)
        rr, cc = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
        zone = ((cc if along_cols else rr) >= lo).reshape(-1)
        zone[s[0] * C + s[1]] = False
        zone[t[0] * C + t[1]] = False
        cand = np.flatnonzero(zone)
        k = min(int(math.ceil(FRAC * R * C)), len(cand))
        pick = np.random.default_rng(1000 * R + C + seed).choice(cand, k, replace=False)
        g.reshape(-1)[pick] = 1
    g[s] = 2
    g[t] = 3
    return g, s[0] * C + s[1], t[0] * C + t[1]


def few_obstacles_map(R, C, n=6, seed=0):
    """A map with n obstacle cells scattered over it, none in a corner (2 x 4096 / 4096 x 2: the end-to-end run stays feasible when
    no obstacle pair closes the corridor -- test_connectors asserts with the oracle that it does)."""
    g = np.zeros((R, C), np.uint8)
    rnd = np.random.default_rng(77 + seed)
    along_cols = C >= R
    L = max(R, C)
    pos = np.sort(rnd.choice(np.arange(8, L - 8, 16), n, replace=False))       # at least 16 apart: never a closed wall
    for p in pos:
        side = int(rnd.integers(0, min(R, C)))
        g[(side, p) if along_cols else (p, side)] = 1
    g[0, 0] = 2
    g[R - 1, C - 1] = 3
    return g, 0, R * C - 1
