"""CPU checkers for the coverage search (pf_cover_improve / pathfit.Coverage): the rule in its literal loop form
over Python sets, a numpy form on the packed words (the two planes `any` and `once`, one popcount per candidate), the validators,
the perturbations and the rounds around it, brute force over all sets of at most p sites, and seven deliberately WRONG solvers that
tests/test_cover_checkers.py must tell from the rule.  m sites, n elements, p slots; site i covers the set S[i] of elements (as
words: element j is bit j & 63 of word j >> 6); a row holds sites or -1 (an empty slot), the slots below `fixed` never change.  The
key is (n - covered, open sites); the candidates of a sweep are sel[o] = i for every o in [fixed, p) and every site i not in the
row, and sel[o] = -1 (written i = m) for every non-empty o; the smallest (key, o, i) is applied while its key is strictly below
the row's."""
import itertools

import numpy as np

from place_checkers import first_bad_row, perturbations, perturbed, valid_row  # noqa: F401  (Placement's rows and stream, unchanged)

SITES_MAX, ELEMS_MAX, OPEN_MAX = 1024, 1 << 20, 64
MAX_MOVES = 1 << 20
LDS_WORDS = 4096                                                     # PF_COVER_LDS_WORDS: the planes live in LDS up to this many words
DENSITIES = (0.02, 0.2, 0.6)
WRONG = ("largest_on_tie", "first_improvement", "swap_forgets_loss", "loss_is_whole_mask", "no_drops", "largest_empty_slot", "counts_tail_bits")


def words_of(n):
    return (int(n) + 63) // 64


if hasattr(np, "bitwise_count"):
    def popcount(w):
        return np.bitwise_count(np.asarray(w, np.uint64)).astype(np.int64)
else:
    _BYTE = np.array([bin(v).count("1") for v in range(256)], np.int64)

    def popcount(w):
        w = np.ascontiguousarray(w, "<u8")
        return _BYTE[w.view(np.uint8).reshape(w.shape + (8,))].sum(-1)


def pack(bits):
    """bool [..., n] -> uint64 [..., W], the tail bits 0."""
    b = np.asarray(bits, bool)
    n = b.shape[-1]
    pad = np.zeros(b.shape[:-1] + (words_of(n) * 64,), bool)
    pad[..., :n] = b
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).reshape(-1).view("<u8").reshape(b.shape[:-1] + (words_of(n),))


def unpack(words, n):
    w = np.ascontiguousarray(words, "<u8")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (8 * w.shape[-1],)), axis=-1, bitorder="little")[..., :n].astype(bool)


def bits(density, m, n, seed):
    """bool [m, n]: seeded masks of the given density."""
    return np.random.default_rng([seed, m, n, int(density * 1000)]).random((m, n)) < density


def sets_of(b):
    return [set(int(j) for j in np.flatnonzero(r)) for r in np.asarray(b, bool)]


def words_of_set(s, n):
    """A set of elements -> the W words as Python ints, built bit by bit."""
    out = [0] * words_of(n)
    for j in s:
        out[j >> 6] |= 1 << (j & 63)
    return out


# ---- the validators
def first_bad_tail(masks, n):
    """(b, i) of the first mask, in flat order, that holds a bit at an element >= n; None."""
    a = np.asarray(masks, np.uint64)
    a = a.reshape((-1,) + a.shape[-2:])
    if n % 64 == 0:
        return None
    bad = np.argwhere(a[:, :, -1] >> np.uint64(n % 64) != 0)
    return None if not len(bad) else (int(bad[0][0]), int(bad[0][1]))


# ---- the rule, literally
def key(S, n, row, wrong=None):
    """(n - cov, open): cnt by counting, slot by slot."""
    cnt = {}
    for s in row:
        if s >= 0:
            for j in S[s]:
                cnt[j] = cnt.get(j, 0) + 1
    cov = sum(1 for j in cnt if cnt[j] > 0 and (j < n or wrong == "counts_tail_bits"))
    return n - cov, sum(1 for s in row if s >= 0)


def once_count(S, n, row):
    cnt = {}
    for s in row:
        if s >= 0:
            for j in S[s]:
                cnt[j] = cnt.get(j, 0) + 1
    return sum(1 for j in cnt if cnt[j] == 1 and j < n)


def union(S, row):
    out = set()
    for s in row:
        if s >= 0:
            out |= S[s]
    return out


def candidate_key(S, n, row, o, i, wrong=None):
    """The key of the row with sel[o] = i (i = m: -1), or what a WRONG solver takes for it."""
    m = len(S)
    new = row[:o] + [i if i < m else -1] + row[o + 1:]
    if row[o] >= 0 and wrong in ("swap_forgets_loss", "loss_is_whole_mask"):
        mine = set() if i == m else S[i]
        if wrong == "swap_forgets_loss":
            cov = len(union(S, row) | mine) if i < m else len(union(S, new))
        else:
            cov = len((union(S, row) - S[row[o]]) | mine)
        return n - cov, sum(1 for s in new if s >= 0)
    return key(S, n, new, wrong)


def improve(S, n, sel, fixed, max_moves, wrong=None, trace=None):
    """The rule's loop over the sets S -> (row, covered (the W words), (cov after, open after, cov before, open before), status,
    (moves, sweeps, elements covered exactly once, drops)).  wrong: one of WRONG.  trace: a list that takes (row before, o, i, key of
    the candidate) per applied move."""
    m, p = len(S), len(sel)
    row = [int(v) for v in sel]
    first = key(S, n, row, wrong)
    moves = sweeps = drops = 0
    while True:
        sweeps += 1
        mine = key(S, n, row, wrong)
        best = None
        slots = list(range(fixed, p))
        if wrong == "largest_empty_slot":
            empty = [o for o in slots if row[o] < 0]
            slots = [o for o in slots if row[o] >= 0 or o == empty[-1]]
        for o in slots:
            for i in range(m + 1):
                if i in row or (i == m and (row[o] < 0 or wrong == "no_drops")):
                    continue
                k = candidate_key(S, n, row, o, i, wrong)
                if wrong == "first_improvement":
                    if best is None and k < mine:
                        best = (k, o, i)
                elif best is None or (k, o, i) < best or (wrong == "largest_on_tie" and k == best[0]):
                    best = (k, o, i)
        if best is None or not best[0] < mine:
            status = 0
            break
        if moves == max_moves:
            status = 2
            break
        if trace is not None:
            trace.append((list(row), best[1], best[2], best[0]))
        row[best[1]] = best[2] if best[2] < m else -1
        drops += best[2] == m
        moves += 1
    last = key(S, n, row, wrong)
    covered = np.array(words_of_set({j for j in union(S, row) if j < n}, n), np.uint64)
    return row, covered, (n - last[0], last[1], n - first[0], first[1]), status, (moves, sweeps, once_count(S, n, row), drops)


# ---- the rule in numpy, on the packed words
def planes(M, row):
    """(any, once): the union of the row's masks and the elements exactly one slot covers."""
    any_, twice = np.zeros(M.shape[1], np.uint64), np.zeros(M.shape[1], np.uint64)
    for s in row:
        if s >= 0:
            twice |= any_ & M[s]
            any_ = any_ | M[s]
    return any_, any_ & ~twice


def sweep_numpy(M, n, row, fixed, additions_only=False):
    """The smallest candidate of a sweep as the word (n - cov) << 24 | open << 17 | o << 11 | i; None with no candidate.  Only the
    smallest empty slot is evaluated: every empty slot has the same candidates with the same keys."""
    m = len(M)
    any_, once = planes(M, row)
    opn = sum(1 for s in row if s >= 0)
    free = np.ones(m, bool)
    free[[s for s in row if s >= 0]] = False
    best, empty = None, False
    for o in range(fixed, len(row)):
        full = row[o] >= 0
        if (not full and empty) or (full and additions_only):
            continue
        empty = empty or not full
        base = any_ & ~(once & M[row[o]]) if full else any_
        if free.any():
            cov = popcount(base[None, :] | M).sum(1)
            cov[~free] = -1
            i = int(np.argmax(cov))                                  # (the first largest: the smallest i)
            w = ((n - int(cov[i])) << 24) | ((opn + (0 if full else 1)) << 17) | (o << 11) | i
            best = w if best is None or w < best else best
        if full:
            w = ((n - int(popcount(base).sum())) << 24) | ((opn - 1) << 17) | (o << 11) | m
            best = w if best is None or w < best else best
    return best


def improve_numpy(M, n, sel, fixed, max_moves, additions_only=False):
    """improve() on the words M uint64 [m, W]; the applied candidate's key is the next row's.  additions_only: no swaps, no drops
    (the greedy construction alone: what the rule is compared with, not one of the WRONG solvers)."""
    M = np.ascontiguousarray(M, np.uint64)
    m = len(M)
    row = [int(v) for v in sel]
    cov = cov0 = int(popcount(planes(M, row)[0]).sum())
    opn = opn0 = sum(1 for s in row if s >= 0)
    moves = sweeps = drops = 0
    while True:
        sweeps += 1
        best = sweep_numpy(M, n, row, fixed, additions_only)
        if best is None or not (best >> 17) < (((n - cov) << 7) | opn):
            status = 0
            break
        if moves == max_moves:
            status = 2
            break
        o, i = (best >> 11) & 63, best & 2047
        row[o] = i if i < m else -1
        cov, opn = n - (best >> 24), (best >> 17) & 127
        drops += i == m
        moves += 1
    any_, once = planes(M, row)
    return row, any_, (cov, opn, cov0, opn0), status, (moves, sweeps, int(popcount(once).sum()), drops)


def same(a, b):
    """Two results, word for word."""
    return list(a[0]) == list(b[0]) and np.array_equal(np.asarray(a[1], np.uint64), np.asarray(b[1], np.uint64)) and \
        tuple(int(v) for v in a[2]) == tuple(int(v) for v in b[2]) and int(a[3]) == int(b[3]) and tuple(int(v) for v in a[4]) == tuple(int(v) for v in b[4])


def better_candidates(S, n, row, fixed):
    """Every (o, i) whose row has a key strictly below the row's own, found by rebuilding the rows (an independent look)."""
    m = len(S)
    mine = key(S, n, list(row))
    out = []
    for o in range(fixed, len(row)):
        for i in range(m + 1):
            if i in row or (i == m and row[o] < 0):
                continue
            new = list(row)
            new[o] = i if i < m else -1
            if key(S, n, new) < mine:
                out.append((o, i))
    return out


def brute_force(S, n, p, keep=()):
    """The smallest key over all sets of at most p sites that hold `keep`."""
    rest = [i for i in range(len(S)) if i not in keep]
    best = None
    for q in range(0, p - len(keep) + 1):
        for extra in itertools.combinations(rest, q):
            k = key(S, n, list(keep) + list(extra))
            best = k if best is None or k < best else best
    return best


# ---- the rounds
def key_of_result(got, n):
    return n - int(got[2][0]), int(got[2][1])


def search(M, n, p, keep=(), starts=8, rounds=3, seed=0, max_moves=None, solver=None):
    """Round 0 improves [keep..., -1, ...]; each later round improves `starts` perturbations of the incumbent (Placement's stream)
    and keeps the strictly smallest key at the smallest start index -> dict(row, covered (words), count, open, unique, history,
    moves, drops)."""
    solver = improve_numpy if solver is None else solver
    f = len(keep)
    limit = 16 * p if max_moves is None else max_moves
    got = solver(M, n, [int(v) for v in keep] + [-1] * (p - f), f, limit)
    best, moves, drops = got, int(got[4][0]), int(got[4][3])
    history = [key_of_result(got, n)]
    rng = np.random.default_rng(seed)
    for _ in range(rounds if p > f else 0):
        for row in perturbations(rng, best[0], f, len(M), starts):
            got = solver(M, n, row, f, limit)
            moves += int(got[4][0])
            drops += int(got[4][3])
            if key_of_result(got, n) < key_of_result(best, n):         # (in start order: the first smallest of the round wins)
                best = got
        history.append(key_of_result(best, n))
    return dict(row=list(best[0]), covered=np.asarray(best[1], np.uint64), count=int(best[2][0]), open=int(best[2][1]), unique=int(best[4][2]), history=history,
                moves=moves, drops=drops)


# ---- the map case the GPU file leans on: every free cell of the golden 20 x 20 map is a site and a target, strict rule, no range
MAP_NAME = "fig7"
MAP_SEARCH = dict(starts=4, rounds=2, seed=3)
MAP_FREE = 290
MAP_THREE = dict(additions=199, rule=206, moves=4)                   # three slots: covered by the additions alone, by the rule, its moves
MAP_ALL = dict(slots=24, additions=13, rule=12)                      # 24 slots: the sites that see all 290, by additions alone and by the rule


def map_cells(g):
    return [(int(r), int(c)) for r, c in np.argwhere(np.asarray(g) != 1)]


def sight_bits(g, sites, targets, strict=True, max_range_sq=-1):
    """bool [m, n]: what each site cell sees of the target cells (tests/visibility_checkers.seen_map)."""
    import visibility_checkers as vc
    occ = vc.occ_of(g)
    ids = [r * occ.shape[1] + c for r, c in targets]
    return np.array([vc.seen_map(occ, s, strict, max_range_sq).reshape(-1)[ids] for s in sites], bool).reshape(len(sites), len(ids))


# ---- the seeded cases that tell each WRONG solver from the rule: (density, m, n, p, seed, start) with start "empty" or "full"
WRONG_CASES = {"largest_on_tie": (0.2, 6, 20, 2, 0, "empty"), "first_improvement": (0.2, 6, 20, 2, 0, "empty"), "swap_forgets_loss": (0.2, 6, 20, 2, 0, "empty"),
               "loss_is_whole_mask": (0.2, 6, 20, 2, 1, "empty"), "no_drops": (0.6, 7, 30, 3, 7, "full"), "largest_empty_slot": (0.2, 6, 20, 2, 0, "empty"),
               "counts_tail_bits": (0.2, 6, 20, 2, 0, "empty")}


def full_row(m, p, seed):
    return [int(v) for v in np.random.default_rng([seed, m, p]).permutation(m)[:p]]


def half_row(m, p, seed):
    return [v if s % 2 == 0 else -1 for s, v in enumerate(full_row(m, p, seed))]


def wrong_case(name):
    """-> (S, n, the start row) of a WRONG solver's case; counts_tail_bits's sets hold elements in [n, 64 W) too."""
    density, m, n, p, seed, start = WRONG_CASES[name]
    S = sets_of(bits(density, m, words_of(n) * 64 if name == "counts_tail_bits" else n, seed))
    return S, n, [-1] * p if start == "empty" else full_row(m, p, seed)
