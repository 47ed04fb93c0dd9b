"""The host protocol the planners' entry points share (pathfit_fields.hip: arm_bad, first_bad, timed_end), pinned per entry point on
the smallest inputs at which a validation kernel's index arithmetic can go wrong (B = 2, a 3 x 4 or 5 x 5 matrix, p = 2 slots, 65
elements = two mask words with a tail, k = 2 robots with 3 tasks): (a) a valid call makes the small device-to-host copies it always
made -- one per validation kernel, and the read-back of the capacities --, (b) a call whose first validation fails names the first
offending index and leaves every buffer as it was, (c) so does a call whose second (third) validation fails: the word at d_bad is
still ~0 behind a kernel that found nothing."""
import numpy as np
import pytest

import golden_io as gio

pytestmark = pytest.mark.gpu

SENTINEL = 77
F8, I4, I8, U8 = np.float64, np.int32, np.int64, np.uint64
B = 2


@pytest.fixture(scope="module")
def eng():
    from pathfit import Engine
    e = Engine(gio.grid("fig7")[0])
    yield e
    e.close()


def attempt(e, ins, outs, call):
    """One engine call over the uploaded `ins` and the sentinel-filled `outs` ((size, dtype) each) -> (the small copies it made, its
    error message or None, whether every buffer holds what it held)."""
    from pathfit import PathfitError
    d = {k: e.put(np.ascontiguousarray(v).reshape(-1)) for k, v in ins.items()}
    d.update({k: e.put(np.full(size, SENTINEL, dt)) for k, (size, dt) in outs.items()})
    try:
        before, msg = e.d2h_counts()[0], None
        try:
            call(e, d)
        except PathfitError as err:
            msg = str(err)
        small = e.d2h_counts()[0] - before
        same = all(d[k].download().tobytes() == np.ascontiguousarray(v).tobytes() for k, v in ins.items())        # (words: a NaN stays a NaN)
        return small, msg, same and all(np.all(d[k].download() == SENTINEL) for k in outs)
    finally:
        for b in d.values():
            b.free()


def numbers(*shape):
    return np.random.default_rng(5).integers(1, 9, shape).astype(F8)


def with_entry(a, at, x):
    a = a.copy()
    a[at] = x
    return a


def tour_solve():
    n, mat = 4, numbers(B, 4, 4)
    outs = dict(total=(B, F8), order=(B * n, I4), status=(B, I4), info=(4 * B, I8))
    return dict(mat=mat), outs, lambda e, d: e.tour_solve(0, n, B, d["mat"], d["total"], d["order"], d["status"], None, d["info"]), 1, [
        (dict(mat=with_entry(mat, (1, 2, 3), np.nan)), "the entry (b, i, j) = (1, 2, 3) is neither >= 0 nor +inf")]


def assign_solve():
    n, m, mat = 3, 4, numbers(B, 3, 4)
    outs = dict(col=(B * n, I4), value=(2 * B, F8), status=(B, I4), dual=(B * (n + m), F8), info=(4 * B, I8))
    return dict(mat=mat), outs, lambda e, d: e.assign_solve(0, n, m, B, d["mat"], d["col"], d["value"], d["status"], d["dual"], d["info"]), 1, [
        (dict(mat=with_entry(mat, (1, 2, 3), np.nan)), "the entry (b, i, j) = (1, 2, 3) is neither +inf nor finite within 2^1000")]


def tour_improve(shared):
    n, mat, b = 4, numbers(1 if shared else B, 4, 4), 0 if shared else 1
    order = np.array([[0, 1, 2, 3], [0, 2, 1, 3]], I4)
    outs = dict(value=(2 * B, F8), status=(B, I4), info=(4 * B, I8))
    return dict(mat=mat, order=order), outs, lambda e, d: e.tour_improve(0, n, B, shared, d["mat"], 9, d["order"], d["value"], d["status"], d["info"]), 2, [
        (dict(mat=with_entry(mat, (b, 1, 3), np.nan)), f"the entry (b, i, j) = ({b}, 1, 3) is neither +inf nor a number in [0, 2^1000]"),
        (dict(order=with_entry(order, (1, 2), 2)), "the start (b, position) = (1, 2) is no permutation of the nodes with node 0 first")]


def fleet(name, shared, capped):
    k, n, N, b = 2, 3, 5, 0 if shared else 1
    nv, ni = (4, 5) if name == "fleet_balance" else (3, 4)
    mat = numbers(1 if shared else B, N, N)
    route = np.array([[0, 2, 3, 1, 4], [0, 2, 1, 3, 4]], I4)
    ins = dict(mat=mat, route=route, **(dict(cap=np.array([2, 2], I4)) if capped else {}))
    outs = dict(len=(B * k, F8), value=(nv * B, F8), status=(B, I4), info=(ni * B, I8))

    def call(e, d):
        getattr(e, name)(0, k, n, B, shared, d["mat"], d.get("cap"), 9, d["route"], d["len"], d["value"], d["status"], d["info"])
    bad = [(dict(mat=with_entry(mat, (b, 2, 4), np.nan)), f"the entry (b, i, j) = ({b}, 2, 4) is neither +inf nor a number in [0, 2^1000]"),
           (dict(route=with_entry(route, (1, 2), 2)), "the start (b, position) = (1, 2) is no permutation of the nodes with node 0 first")]
    if capped:                                                        # the read-back of cap and the capacity kernel: two more copies
        bad.append((dict(cap=np.array([2, 1], I4)), "the start (b, robot) = (1, 1) holds more tasks than its capacity"))
    return ins, outs, call, 4 if capped else 2, bad


def place_improve(shared):
    m, n, p, mat, b = 3, 4, 2, numbers(1 if shared else B, 3, 4), 0 if shared else 1
    sel = np.array([[0, -1], [2, 1]], I4)
    outs = dict(owner=(B * n, I4), value=(4 * B, F8), status=(B, I4), info=(4 * B, I8))
    return dict(mat=mat, sel=sel), outs, lambda e, d: e.place_improve(0, m, n, p, 1, B, shared, d["mat"], 9, d["sel"], d["owner"], d["value"], d["status"], d["info"]), 2, [
        (dict(mat=with_entry(mat, (b, 2, 3), np.nan)), f"the entry (b, i, j) = ({b}, 2, 3) is neither +inf nor a number in [+0.0, 2^1000]"),
        (dict(sel=with_entry(sel, (1, 1), 2)), "the row (b, slot) = (1, 1) lies outside [-1, m), repeats the site of a smaller slot")]


def cover_pack():
    K, n, ld = 2, 65, 16
    src, targets = numbers(K, ld), (np.arange(n) % ld).astype(I4)
    outs = dict(mask=(3 * 2, U8))
    return dict(src=src, targets=targets), outs, lambda e, d: e.cover_pack(1, K, n, d["src"], ld, d["targets"], 4.0, 1, d["mask"]), 1, [
        (dict(targets=with_entry(targets, 40, ld)), "target 40 lies outside [0, ld)")]


def cover_improve(shared):
    from pathfit.cover import pack_bits
    m, n, p, b = 3, 65, 2, 0 if shared else 1
    mask = pack_bits(np.random.default_rng(5).random((1 if shared else B, m, n)) < 0.4)
    sel = np.array([[0, -1], [2, 1]], I4)
    outs = dict(covered=(B * 2, U8), value=(4 * B, I8), status=(B, I4), info=(4 * B, I8))
    return dict(mask=mask, sel=sel), outs, lambda e, d: e.cover_improve(m, n, p, 1, B, shared, d["mask"], 9, d["sel"], d["covered"], d["value"], d["status"], d["info"]), 2, [
        (dict(mask=with_entry(mask, (b, 2, 1), mask[b, 2, 1] | U8(2))), f"the mask (b, i) = ({b}, 2) holds a bit at an element >= n"),
        (dict(sel=with_entry(sel, (1, 1), 2)), "the row (b, slot) = (1, 1) lies outside [-1, m), repeats the site of a smaller slot")]


CASES = {"tour_solve": tour_solve, "assign_solve": assign_solve, "cover_pack": cover_pack}
for s in (0, 1):
    CASES.update({f"tour_improve-shared{s}": lambda s=s: tour_improve(s), f"place_improve-shared{s}": lambda s=s: place_improve(s),
                  f"cover_improve-shared{s}": lambda s=s: cover_improve(s)})
    for name in ("fleet_improve", "fleet_balance"):
        CASES.update({f"{name}-shared{s}-cap{c}": lambda name=name, s=s, c=c: fleet(name, s, c) for c in (0, 1)})


@pytest.mark.parametrize("case", sorted(CASES))
def test_copies_first_index_and_untouched_buffers(eng, case):
    ins, outs, call, copies, bad = CASES[case]()
    small, msg, _ = attempt(eng, ins, outs, call)
    print(case, "small copies:", small)
    assert msg is None and small == copies                            # (a)
    for x, (change, want) in enumerate(bad):                          # (b) the first validation, (c) the later ones
        small, msg, same = attempt(eng, dict(ins, **change), outs, call)
        print(case, "validation", x, "->", msg)
        assert msg is not None and want in msg and same, (case, x, msg, same)
    assert attempt(eng, ins, outs, call)[:2] == (copies, None)        # the handle still works, the word is armed again
