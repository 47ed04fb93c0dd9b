"""CPU checkers for the nearest-source fields (pf_dist_field_merged / pf_dist_field_owners): field_checkers' reference-shaped
Dijkstra seeded with a whole source SET, and an owner tracer.  tests/test_nearest_owner_rule.py pins them against the
single-source checkers on any host; the GPU tests compare the device against them.

A set is a list of flat cell ids; the owner of a cell is the index within the set of the source at the root of the cell's chain
through the parent codes, the lowest index where a cell is listed more than once, -1 where the code is 255."""
import heapq

import numpy as np

import field_checkers as fc


def multi_dijkstra(grid, mm, sources):
    """field_checkers.reference_dijkstra with every free source pushed at g = 0 -> (labels float64 [R, C], parent codes uint8 [R, C]);
    a source on an obstacle is skipped."""
    R, C = mm.shape
    occ = np.asarray(grid).reshape(-1)
    dist = [fc.INF] * (R * C)
    code = [fc.NONE] * (R * C)
    m = mm.reshape(-1).tolist()
    step = [fc.DR[k] * C + fc.DC[k] for k in range(8)]
    heap = []
    for s in sources:
        s = int(s)
        if occ[s] != 1 and dist[s] != 0.0:
            dist[s], code[s] = 0.0, fc.SOURCE
            heap.append((0.0, s))
    heapq.heapify(heap)
    closed = set()
    while heap:
        g, u = heapq.heappop(heap)
        if u in closed:
            continue
        closed.add(u)
        for k in range(8):
            if (m[u] >> k) & 1:
                v = u + step[k]
                if v in closed:
                    continue
                t = g + fc.W[k]
                if t < dist[v]:                                       # strict, as dijkstra.py:84
                    dist[v], code[v] = t, k
                    heapq.heappush(heap, (t, v))
    return np.array(dist).reshape(R, C), np.array(code, np.uint8).reshape(R, C)


def owners_of(code, sources):
    """The owner map int32 [R, C] of parent codes with several roots, by walking every chain (memoised), and the territory sizes
    int64 [len(sources)]."""
    R, C = code.shape
    flat = code.reshape(-1)
    rank = {}
    for j, s in enumerate(sources):
        rank.setdefault(int(s), j)
    own = np.full(R * C, -2, np.int32)
    for v in range(R * C):
        chain, u = [], v
        while own[u] == -2:
            chain.append(u)
            k = int(flat[u])
            if k == fc.NONE:
                own[u] = -1
            elif k == fc.SOURCE:
                own[u] = rank[u]
            else:
                assert k < 8 and len(chain) <= R * C, (u, k)
                u -= fc.DR[k] * C + fc.DC[k]
        own[chain] = own[u]
    count = np.bincount(own[own >= 0], minlength=len(sources)).astype(np.int64)
    return own.reshape(R, C), count


def seeded_sets(g, sizes, seed):
    """One set of distinct seeded free cells per entry of `sizes` (capped at the number of free cells)."""
    free = np.flatnonzero(np.asarray(g).reshape(-1) != 1)
    rnd = np.random.default_rng(seed)
    return [[int(v) for v in rnd.choice(free, min(int(n), len(free)), replace=False)] for n in sizes]


def csr(sets):
    """-> (set_off int32 [B + 1], ids int32)"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    return off, np.array([v for s in sets for v in s], np.int32)
