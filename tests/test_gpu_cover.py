"""The coverage search on the device (pf_cover_pack, pf_cover_improve, pathfit.Coverage) against the numpy model of
tests/cover_checkers.py (pinned by tests/test_cover_checkers.py).  Every comparison is exact equality of integers; every output
buffer lies between canary words.  A workgroup of 1024 threads searches a start, a wavefront a site, a lane every 64th word, eight
slots a pass; the planes of a start live in LDS up to 4096 words and in the handle's scratch above: the sizes lie about the word,
the wavefront's stride, the workgroup, the pass and that switch, and reach each axis's limit."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import cover_checkers as cc
import golden_io as gio

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
PAD = 64                                                             # canary words in front of and behind every output


def between_canaries(e, n, dtype, inside=None):
    a = np.full(n + 2 * PAD, CANARY, dtype)
    if inside is not None:
        a[PAD:PAD + n] = inside
    return e.put(a)


def inner(buf, tag):
    a = buf.download()
    assert np.all(a[:PAD] == CANARY) and np.all(a[len(a) - PAD:] == CANARY), tag
    return a[PAD:len(a) - PAD]


@pytest.fixture(scope="module")
def eng():
    from pathfit import Engine
    e = Engine(gio.grid("fig7")[0])
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _model(key, m, n, start, fixed, limit):
    return cc.improve_numpy(np.frombuffer(key, np.uint64).reshape(m, -1), n, list(start), fixed, limit)


def model(M, n, start, fixed, limit):
    M = np.ascontiguousarray(M, np.uint64)
    return _model(M.tobytes(), M.shape[0], n, tuple(int(v) for v in start), fixed, limit)


def rand_words(m, n, seed, thin=1):
    """uint64 [m, W]: seeded words, each the AND of `thin` random words (density 2^-thin), the tail bits 0."""
    rng = np.random.default_rng([seed, m, n, thin])
    W = cc.words_of(n)
    M = rng.integers(0, 2 ** 64, (m, W), dtype=np.uint64)
    for _ in range(thin - 1):
        M &= rng.integers(0, 2 ** 64, (m, W), dtype=np.uint64)
    if n % 64:
        M[:, -1] &= np.uint64((1 << (n % 64)) - 1)
    return M


def run(e, masks, n, rows, fixed, shared, limit, want_covered=True, want_info=True):
    """One raw Engine call, every output between canaries -> (row [B, p], covered [B, W], value [B, 4], status [B], info [B, 4])."""
    from pathfit.engine import _View
    masks = np.ascontiguousarray(masks, np.uint64)
    rows = np.ascontiguousarray(rows, np.int32)
    B, p = rows.shape
    m, W = masks.shape[-2:]
    assert W == cc.words_of(n) and masks.shape == ((m, W) if shared else (B, m, W))
    dm = e.put(masks.reshape(-1))
    rb = between_canaries(e, B * p, np.int32, rows.reshape(-1))
    cb, vb = between_canaries(e, B * W, np.uint64), between_canaries(e, 4 * B, np.int64)
    sb, ib = between_canaries(e, B, np.int32), between_canaries(e, 4 * B, np.int64)
    try:
        e.cover_improve(m, n, p, fixed, B, shared, dm, limit, _View(e, rb.at(PAD), B * p, np.int32), _View(e, cb.at(PAD), B * W, np.uint64) if want_covered else None,
                        _View(e, vb.at(PAD), 4 * B, np.int64), _View(e, sb.at(PAD), B, np.int32), _View(e, ib.at(PAD), 4 * B, np.int64) if want_info else None)
        assert e.last_kernel_ms() > 0
        covered, info = inner(cb, "covered").reshape(B, W), inner(ib, "info").reshape(B, 4)
        assert (want_covered or np.all(covered == CANARY)) and (want_info or np.all(info == CANARY))
        return inner(rb, "row").reshape(B, p), covered, inner(vb, "value").reshape(B, 4), inner(sb, "status"), info
    finally:
        for b in (dm, rb, cb, vb, sb, ib):
            b.free()


def check(e, masks, n, rows, fixed=0, shared=False, limit=None, tag=None):
    masks = np.ascontiguousarray(masks, np.uint64)
    rows = np.ascontiguousarray(rows, np.int32)
    B, p = rows.shape
    m = masks.shape[-2]
    limit = 16 * p if limit is None else limit
    got = run(e, masks, n, rows, fixed, shared, limit)
    for b in range(B):
        want = model(masks if shared else masks[b], n, rows[b], fixed, limit)
        assert cc.same(tuple(x[b] for x in got), want), (tag, m, n, p, fixed, B, b, [x[b] for x in got][2:], want[2:])
        assert cc.valid_row(list(got[0][b]), m, p, fixed) and list(got[0][b, :fixed]) == list(rows[b, :fixed])
    return got


def three_rows(m, p, seed):
    return [[-1] * p, cc.full_row(m, p, seed), cc.half_row(m, p, seed)]


# ---- 1. sizes
@pytest.mark.parametrize("m,n,p", [(1, 1, 1), (2, 1, 1), (3, 2, 3), (5, 7, 2)])
def test_the_smallest_shapes(eng, m, n, p):
    for density in cc.DENSITIES + (1.0,):
        masks = [cc.pack(cc.bits(density, m, n, s)) for s in range(3)]
        for rows in ([[-1] * p] * 3, [cc.full_row(m, p, s) for s in range(3)], [cc.half_row(m, p, s) for s in range(3)]):
            row, covered, value, status, info = check(eng, masks, n, rows, tag=density)
            assert np.all(status == 0) and np.all(info[:, 1] == info[:, 0] + 1)


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 4095, 4096, 4097])
def test_elements_about_the_word_and_the_wavefronts_stride(eng, n):
    m, p = 20, 3
    masks = [rand_words(m, n, 1, 3), rand_words(m, n, 2, 1), cc.pack(cc.bits(0.02, m, n, 3))]
    row, covered, value, status, info = check(eng, masks, n, three_rows(m, p, 1), tag="n")
    assert np.all(status == 0) and info[0, 0] >= p and value[0, 2] == 0


@pytest.mark.parametrize("W", [cc.LDS_WORDS - 1, cc.LDS_WORDS, cc.LDS_WORDS + 1])
def test_the_planes_on_both_sides_of_the_lds_switch(eng, W):
    m, p = 12, 3
    for n in (64 * W, 64 * W - 37):
        masks = [rand_words(m, n, 4, 3), rand_words(m, n, 5, 2), rand_words(m, n, 6, 4)]
        row, covered, value, status, info = check(eng, masks, n, three_rows(m, p, 2), tag="switch")
        assert np.all(status == 0) and info[0, 0] >= p


@pytest.mark.parametrize("m", [63, 64, 65, 1023, 1024])
def test_sites_about_the_wavefront_and_the_limit(eng, m):
    n, p = 200, 4
    limit = 16 * p if m < 1000 else 5
    masks = [rand_words(m, n, 7, 4), cc.pack(cc.bits(0.02, m, n, 8))]
    row, covered, value, status, info = check(eng, masks, n, [[-1] * p, [m - 1, 0, -1, m - 2]], limit=limit, tag="m")   # (the last sites stand in a row)
    assert info[0, 0] >= 4 and (m > 1000 or np.all(status == 0))


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64])
def test_slots_about_the_pass_and_the_limit(eng, p):
    m, n = 80, 1000
    M = rand_words(m, n, 9, 5)
    row, covered, value, status, info = check(eng, M, n, three_rows(m, p, 3), shared=True, limit=min(16 * p, 90), tag="p")
    assert info[0, 0] >= min(p, 20)


@pytest.mark.parametrize("m,n,p,limit", [(1024, 65536, 64, 1), (16, 1 << 20, 3, 2)])
def test_the_limits_under_a_cap(eng, m, n, p, limit):
    M = rand_words(m, n, 10, 4)
    row, covered, value, status, info = check(eng, M, n, [cc.half_row(m, p, 5)], shared=True, limit=limit, tag="limit")
    assert status[0] == 2 and info[0, :2].tolist() == [limit, limit + 1]


# ---- 2. rows and batches
def test_a_full_redundant_row_is_dropped(eng):
    n = 300
    b = cc.bits(0.2, 3, n, 1)
    b = np.concatenate([b, b, b[:1] | b[1:2]])                        # sites 3 .. 5 repeat 0 .. 2; site 6 holds 0 and 1
    M = cc.pack(b)
    row, covered, value, status, info = check(eng, M, n, [[0, 3, 1, 4], [6, 0, 1, 2], [0, 1, 2, 5]], shared=True, tag="redundant")
    assert np.all(status == 0) and np.all(info[:, 3] >= 1) and np.all(value[:, 1] < 4) and list(value[:, 0]) == [int((b[0] | b[1] | b[2]).sum())] * 3


def test_fixed_slots_and_m_equal_p(eng):
    m, n, p = 12, 100, 4
    M = cc.pack(cc.bits(0.2, m, n, 8))
    for fixed in (0, 1, p):
        rows = [cc.full_row(m, p, s) for s in range(3)] + [cc.full_row(m, p, 3)[:max(fixed, 1)] + [-1] * (p - max(fixed, 1))]
        row, covered, value, status, info = check(eng, M, n, rows, fixed=fixed, shared=True, tag="fixed")
        assert np.all(status == 0)
        if fixed == p:
            assert np.array_equal(row[:3], np.array(rows[:3])) and info[:3, :2].tolist() == [[0, 1]] * 3 and np.array_equal(value[:3, :2], value[:3, 2:])
    M = cc.pack(np.eye(5, 40, dtype=bool))
    row, covered, value, status, info = check(eng, M, 40, [[-1] * 5, [4, 3, 2, 1, 0], [2, -1, -1, 0, -1]], shared=True, tag="m == p")
    assert info[1].tolist()[:2] == [0, 1] and list(row[1]) == [4, 3, 2, 1, 0] and list(value[:, 0]) == [5, 5, 5]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_batch_sizes_at_12_100_3(eng, B, shared):
    m, n, p = 12, 100, 3
    rows = [three_rows(m, p, b)[b % 3] for b in range(B)]
    if shared:
        check(eng, cc.pack(cc.bits(0.2, m, n, 9)), n, rows, shared=True, tag="batch")
    else:
        check(eng, [cc.pack(cc.bits(cc.DENSITIES[b % 3], m, n, b)) for b in range(B)], n, rows, tag="batch")


def test_the_cap_on_the_moves(eng):
    m, n, p = 30, 500, 5
    M = cc.pack(cc.bits(0.2, m, n, 10))
    full = model(M, n, [-1] * p, 0, 16 * p)
    moves = full[4][0]
    assert full[3] == 0 and moves >= p
    for limit in (0, 1, moves - 1, moves):
        row, covered, value, status, info = check(eng, M, n, [[-1] * p, full[0]], shared=True, limit=limit, tag="cap")
        assert list(status) == [0 if limit == moves else 2, 0] and info[0, :2].tolist() == [limit, limit + 1] and info[1, :2].tolist() == [0, 1]
        assert limit or list(row[0]) == [-1] * p


def test_covered_null_info_null_and_five_identical_runs(eng):
    m, n, p = 40, 3000, 6
    masks = [rand_words(m, n, 11, t) for t in (1, 2, 4, 6)]
    rows = three_rows(m, p, 1) + [cc.full_row(m, p, 3)]
    ref = check(eng, masks, n, rows, tag="identical")
    for _ in range(5):
        again = run(eng, masks, n, rows, 0, False, 16 * p)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, ref))
    bare = run(eng, masks, n, rows, 0, False, 16 * p, want_covered=False, want_info=False)
    assert all(bare[x].tobytes() == ref[x].tobytes() for x in (0, 2, 3))


# ---- 3. what the masks hold
@pytest.mark.parametrize("m,n,p", [(6, 70, 3), (70, 1300, 5)])
def test_mask_content(eng, m, n, p):
    zero, one = np.zeros((m, n), bool), np.ones((m, n), bool)
    b = cc.bits(0.2, m, n, 12)
    twice = np.concatenate([b[:m // 2], b[:m - m // 2]])              # duplicate masks
    masks = [cc.pack(x) for x in (zero, one, twice, b)]
    for rows in ([[-1] * p] * 4, [cc.half_row(m, p, b) for b in range(4)], [cc.full_row(m, p, b) for b in range(4)]):
        row, covered, value, status, info = check(eng, masks, n, rows, tag="content")
        assert np.all(status == 0)
        assert value[0].tolist()[:2] == [0, 0] and list(row[0]) == [-1] * p           # nothing covers anything: the slots end empty
        assert value[1].tolist()[:2] == [n, 1] and info[1, 2] == n                   # one all-one mask covers everything
        sites = [int(s) for s in row[2] if s >= 0]
        assert len({s % (m // 2) for s in sites}) == len(sites)                      # (m is even: site i repeats i + m / 2) no two copies of a mask stay


def test_both_deals_and_the_hbm_planes_through_the_stress_build(eng):
    """lib/stress/libpathfit_cv_lanes.so (build.py: COVER_VARIANTS) deals a lane per (site group, slot) and keeps the planes in HBM
    from three words on: every output is the model's in both libraries."""
    from test_gpu_assign import engine_on
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(root, "maaco-path-planing_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = mod.variant_path("cv_lanes")
    assert list(mod.COVER_VARIANTS) == ["cv_lanes"] and os.path.exists(so), "build the stress variants first (__graft_entry__.build())"
    other = engine_on(so, gio.grid("fig7")[0])
    try:
        for m, n, p in [(1, 1, 1), (3, 2, 3), (5, 7, 2), (20, 128, 3), (20, 129, 4), (65, 200, 5), (80, 1000, 9), (80, 1000, 33), (70, 4097, 64)]:
            masks = [rand_words(m, n, 13, 3), cc.pack(cc.bits(0.2, m, n, 1)), cc.pack(cc.bits(0.02, m, n, 2))]
            for fixed in (0, 1):
                rows = three_rows(m, p, 4)[fixed:] + [[-1] * p] * fixed      # (the empty row has no kept slot: it goes with fixed = 0 only)
                if fixed:
                    rows[2] = cc.full_row(m, p, 5)
                mine = check(eng, masks, n, rows, fixed=fixed, limit=min(16 * p, 40), tag="shipped")
                theirs = check(other, masks, n, rows, fixed=fixed, limit=min(16 * p, 40), tag="cv_lanes")
                assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, theirs))
        rows = [three_rows(12, 3, b)[b % 3] for b in range(300)]
        M = cc.pack(cc.bits(0.2, 12, 200, 9))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(check(eng, M, 200, rows, shared=True), check(other, M, 200, rows, shared=True)))
    finally:
        other.close()


# ---- 4. pf_cover_pack
def pack_on_device(e, kind, src, ld, targets, radius, row0, total_rows):
    """-> the whole mask block [total_rows, W] (CANARY where nothing was written), canaries about it checked."""
    from pathfit.engine import _View
    n, W = len(targets), cc.words_of(len(targets))
    K = len(src) // ld
    ds, dt = e.put(src), e.put(np.asarray(targets, np.int32))
    mb = between_canaries(e, total_rows * W, np.uint64)
    try:
        e.cover_pack(kind, K, n, ds, ld, dt, radius, row0, _View(e, mb.at(PAD), total_rows * W, np.uint64))
        assert e.last_kernel_ms() > 0
        return inner(mb, "mask").reshape(total_rows, W)
    finally:
        for b in (ds, dt, mb):
            b.free()


def padded(rows, ld, fill):
    out = np.full((len(rows), ld), fill, rows.dtype)
    out[:, :rows.shape[1]] = rows
    return out.reshape(-1)


def strip_map():
    g = np.zeros((1, 4096), np.uint8)
    g[0, [700, 701, 2900]] = 1
    return g


@pytest.mark.parametrize("which", ["fig7", "strip"])
def test_pack_against_the_downloaded_rows(which):
    from pathfit import Engine
    g = gio.grid("fig7")[0] if which == "fig7" else strip_map()
    RC = g.size
    free = np.flatnonzero(np.asarray(g).reshape(-1) != 1)
    views = free[::9][:40] if which == "fig7" else np.array([0, 5, 699, 702, 2048, 2899, 2901, 4095])
    rng = np.random.default_rng(3)
    e = Engine(g)
    try:
        K = len(views)
        dseen, dfield = e.buf(K * RC, np.uint8), e.buf(K * RC, np.float64)
        try:
            e.visibility_field(views, dseen, True, -1)
            e.dist_field_batch(views, dfield, True, True)
            seen, field = dseen.download().reshape(K, RC), dfield.download().reshape(K, RC)
        finally:
            dseen.free()
            dfield.free()
        assert np.isinf(field).any() and (seen != 0).any()
        for n in (RC, RC - 1, 65, RC - 70):
            targets = rng.permutation(RC)[:n] if n < RC else np.arange(RC)
            for row0, total, ld in ((0, K, RC), (3, K + 5, RC + 7)):
                got = pack_on_device(e, 0, padded(seen, ld, 1), ld, targets, 0.0, row0, total)
                want = cc.pack(seen[:, targets] != 0)
                assert np.array_equal(got[row0:row0 + K], want) and np.all(got[:row0] == CANARY) and np.all(got[row0 + K:] == CANARY)
                assert cc.first_bad_tail(got[row0:row0 + K], n) is None
                finite = field[:, targets][np.isfinite(field[:, targets])]
                at = float(np.sort(finite)[len(finite) // 3])         # a radius exactly at a field value, and one ulp below it
                for radius in (at, float(np.nextafter(at, 0.0)), 0.0, 1e300):
                    got = pack_on_device(e, 1, padded(field, ld, 0.0), ld, targets, radius, row0, total)
                    want = cc.pack(field[:, targets] <= radius)
                    assert np.array_equal(got[row0:row0 + K], want) and np.all(got[:row0] == CANARY) and np.all(got[row0 + K:] == CANARY)
                assert (field[:, targets] == at).any() and not np.array_equal(cc.pack(field[:, targets] <= at), cc.pack(field[:, targets] < at))
        nan = field.copy()
        nan[0, :5] = np.nan
        got = pack_on_device(e, 1, nan.reshape(-1), RC, np.arange(RC), 1e300, 0, K)
        assert np.array_equal(got, cc.pack(np.isfinite(nan)))         # +inf and NaN give 0
    finally:
        e.close()


# ---- 5. argument errors of the raw ABI
def test_argument_and_validation_errors_leave_every_output_untouched(eng):
    e, L = eng, eng.L
    m, n, p, B = 5, 70, 3, 3
    W = cc.words_of(n)
    good = np.array([cc.pack(cc.bits(0.2, m, n, b)) for b in range(B)])
    rows = np.array([[0, -1, 3], [4, 2, -1], [1, 0, 2]], np.int32)
    held = np.full(B * p + 2 * PAD, CANARY, np.int32)
    held[PAD:PAD + B * p] = rows.reshape(-1)
    rb, cb, vb = e.put(held), between_canaries(e, B * W, np.uint64), between_canaries(e, 4 * B, np.int64)
    sb, ib = between_canaries(e, B, np.int32), between_canaries(e, 4 * B, np.int64)
    dm = e.put(good.reshape(-1))
    sel, covered, value, status, info = rb.at(PAD), cb.at(PAD), vb.at(PAD), sb.at(PAD), ib.at(PAD)
    try:
        improve = L.pf_cover_improve
        out = (sel, covered, value, status, info)
        assert improve(None, m, n, p, 1, B, 0, dm.ptr, 9, *out) == -2
        for args, msg in [((0, n, p, 1, B, 0, dm.ptr, 9) + out, "m = 0"), ((1025, n, p, 1, B, 0, dm.ptr, 9) + out, "m = 1025"),
                          ((m, 0, p, 1, B, 0, dm.ptr, 9) + out, "n = 0"), ((m, (1 << 20) + 1, p, 1, B, 0, dm.ptr, 9) + out, "n = 1048577"),
                          ((m, n, 0, 0, B, 0, dm.ptr, 9) + out, "p = 0"), ((m, n, 6, 1, B, 0, dm.ptr, 9) + out, "p = 6"),
                          ((100, n, 65, 1, B, 0, dm.ptr, 9) + out, "p = 65"), ((m, n, p, -1, B, 0, dm.ptr, 9) + out, "fixed = -1"),
                          ((m, n, p, 4, B, 0, dm.ptr, 9) + out, "fixed = 4"), ((m, n, p, 1, 0, 0, dm.ptr, 9) + out, "B = 0"),
                          ((m, n, p, 1, B, 2, dm.ptr, 9) + out, "shared = 2"), ((m, n, p, 1, B, -1, dm.ptr, 9) + out, "shared = -1"),
                          ((m, n, p, 1, B, 0, dm.ptr, -1) + out, "max_moves = -1"), ((m, n, p, 1, B, 0, dm.ptr, (1 << 20) + 1) + out, "max_moves = 1048577"),
                          ((m, n, p, 1, B, 0, None, 9) + out, "must not be null"), ((m, n, p, 1, B, 0, dm.ptr, 9, None, covered, value, status, info), "must not be null"),
                          ((m, n, p, 1, B, 0, dm.ptr, 9, sel, covered, None, status, info), "must not be null"),
                          ((m, n, p, 1, B, 0, dm.ptr, 9, sel, covered, value, None, info), "must not be null")]:
            assert improve(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode(), (msg, L.pf_last_error(e.h))
        # a set tail bit: the smallest (b, i) is named
        bad = good.copy()
        bad[2, 1, W - 1] |= np.uint64(1) << np.uint64(n % 64)
        bad[1, 3, W - 1] |= np.uint64(1) << np.uint64(63)
        assert cc.first_bad_tail(bad, n) == (1, 3)
        dm.upload(bad.reshape(-1))
        assert improve(e.h, m, n, p, 1, B, 0, dm.ptr, 9, *out) == -1 and "(b, i) = (1, 3)" in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
        bad[1, 3] = good[1, 3]
        dm.upload(bad.reshape(-1))
        assert improve(e.h, m, n, p, 1, B, 0, dm.ptr, 9, *out) == -1 and "(b, i) = (2, 1)" in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
        dm.upload(good.reshape(-1))
        # a bad row: the smallest (b, slot) is named
        for change, fixed, at in [({(2, 2): 0}, 1, (2, 2)), ({(1, 1): 4, (2, 2): 0}, 1, (1, 1)), ({(1, 2): 5}, 1, (1, 2)), ({(0, 1): -2}, 1, (0, 1)),
                                  ({(1, 0): -1}, 1, (1, 0)), ({}, 2, (0, 1)), ({(0, 1): 3, (0, 2): 3}, 0, (0, 2))]:
            broken = rows.copy()
            for (b, s), v in change.items():
                broken[b, s] = v
            assert cc.first_bad_row(broken, m, p, fixed) == at
            held[PAD:PAD + B * p] = broken.reshape(-1)
            rb.upload(held)
            assert improve(e.h, m, n, p, fixed, B, 0, dm.ptr, 9, *out) == -1
            assert f"(b, slot) = ({at[0]}, {at[1]})" in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
            assert np.array_equal(rb.download(), held)
        for b in (cb, vb, sb, ib):
            assert np.all(b.download() == CANARY)
        # the handle still works
        held[PAD:PAD + B * p] = rows.reshape(-1)
        rb.upload(held)
        assert improve(e.h, m, n, p, 1, B, 0, dm.ptr, 9, *out) == 0
        want = model(good[0], n, rows[0], 1, 9)
        assert vb.download()[PAD:PAD + 4].tolist() == list(want[2]) and list(rb.download()[PAD:PAD + p]) == want[0]
    finally:
        for b in (rb, cb, vb, sb, ib, dm):
            b.free()


def test_pack_argument_errors_leave_the_masks_untouched(eng):
    e, L = eng, eng.L
    K, n, ld = 3, 70, 400
    W = cc.words_of(n)
    src8, src64 = e.put(np.ones(K * ld, np.uint8)), e.put(np.ones(K * ld, np.float64))
    tg = e.put(np.arange(n, dtype=np.int32))
    mb = between_canaries(e, K * W, np.uint64)
    mask = mb.at(PAD)
    try:
        pack = L.pf_cover_pack
        assert pack(None, 0, K, n, src8.ptr, ld, tg.ptr, 0.0, 0, mask) == -2
        for args, msg in [((2, K, n, src8.ptr, ld, tg.ptr, 0.0, 0, mask), "kind = 2"), ((-1, K, n, src8.ptr, ld, tg.ptr, 0.0, 0, mask), "kind = -1"),
                          ((0, 0, n, src8.ptr, ld, tg.ptr, 0.0, 0, mask), "K = 0"), ((0, 1025, n, src8.ptr, ld, tg.ptr, 0.0, 0, mask), "K = 1025"),
                          ((0, K, 0, src8.ptr, ld, tg.ptr, 0.0, 0, mask), "n = 0"), ((0, K, (1 << 20) + 1, src8.ptr, ld, tg.ptr, 0.0, 0, mask), "n = 1048577"),
                          ((0, K, n, src8.ptr, 0, tg.ptr, 0.0, 0, mask), "ld = 0"), ((0, K, n, src8.ptr, ld, tg.ptr, 0.0, -1, mask), "row0 = -1"),
                          ((0, K, n, src8.ptr, ld, tg.ptr, 0.0, 1022, mask), "row0 = 1022"), ((1, K, n, src64.ptr, ld, tg.ptr, -1.0, 0, mask), "radius"),
                          ((1, K, n, src64.ptr, ld, tg.ptr, float("nan"), 0, mask), "radius"), ((1, K, n, src64.ptr, ld, tg.ptr, float("inf"), 0, mask), "radius"),
                          ((0, K, n, None, ld, tg.ptr, 0.0, 0, mask), "must not be null"), ((0, K, n, src8.ptr, ld, None, 0.0, 0, mask), "must not be null"),
                          ((0, K, n, src8.ptr, ld, tg.ptr, 0.0, 0, None), "must not be null")]:
            assert pack(e.h, *args) == -1 and msg in L.pf_last_error(e.h).decode(), (msg, L.pf_last_error(e.h))
        for j, v in ((69, ld), (7, -1)):                              # a target outside [0, ld): the first is named, nothing is read or written
            t = np.arange(n, dtype=np.int32)
            t[j] = v
            t[69] = ld
            tg.upload(t)
            assert pack(e.h, 0, K, n, src8.ptr, ld, tg.ptr, 0.0, 0, mask) == -1 and f"target {j} " in L.pf_last_error(e.h).decode(), L.pf_last_error(e.h)
        assert np.all(mb.download() == CANARY)
        tg.upload(np.arange(n, dtype=np.int32))
        assert pack(e.h, 0, K, n, src8.ptr, ld, tg.ptr, 0.0, 0, mask) == 0
        assert np.array_equal(inner(mb, "mask").reshape(K, W), cc.pack(np.ones((K, n), bool)))
    finally:
        for b in (src8, src64, tg, mb):
            b.free()


# ---- 6. Coverage end to end
def ids_of(g, cells):
    return [r * g.shape[1] + c for r, c in cells]


def against_the_model(t, bits, search):
    """The packed masks against bool [m, n]; the row, sites, covered, mask, seen_by, unique, history, moves and drops against the
    model."""
    M = cc.pack(bits)
    assert np.array_equal(t.masks, M)
    want = cc.search(M, t.n, t.count, keep=t.keep, max_moves=t.max_moves, **search)
    assert list(t.row) == want["row"] and t.sites == [v for v in want["row"] if v >= 0] and t.cells == [t.candidates[v] for v in t.sites]
    assert [t.covered, t.moves, t.drops, t.history] == [want["count"], want["moves"], want["drops"], want["history"]]
    assert np.array_equal(t.mask, cc.unpack(want["covered"], t.n)) and t.covered == int(t.mask.sum()) and t.complete == (t.covered == t.n)
    assert t.coverage == t.covered / t.n and t.coverage_of(t.sites) == t.covered and t.coverage_of([]) == 0
    assert np.array_equal(t.seen_by, bits[t.sites].sum(0)) and np.array_equal(t.mask, t.seen_by > 0)
    assert t.unique == [[int(j) for j in np.flatnonzero(bits[s] & (t.seen_by == 1))] for s in t.sites] and sum(len(u) for u in t.unique) == want["unique"]
    assert np.array_equal(t.map().reshape(-1)[t.target_ids], t.mask) and int(t.map().sum()) == len(set(t.target_ids[t.mask].tolist()))
    return want


def sight_bits(e, g, t):
    from pathfit import Visibility
    v = Visibility(g, t.restrict_diagonal_near_obstacle, engine=e)
    try:
        return v.seen(t.candidates, t.max_range).reshape(t.m, -1)[:, t.target_ids]
    finally:
        v.close()


def reach_bits(e, g, t):
    from pathfit import DistanceField
    df = DistanceField(g, sources=t.candidates, engine=e)
    try:
        return df.fields.reshape(t.m, -1)[:, t.target_ids] <= t.radius
    finally:
        df.close()


def test_coverage_on_the_map_every_free_cell_a_site_and_a_target():
    """The pinned fact: three cameras see 206 of the 290 free cells (three additions alone 199); 12 guards see everything."""
    from pathfit import Coverage, Engine
    g = gio.grid(cc.MAP_NAME)[0]
    cells = cc.map_cells(g)
    e = Engine(g)
    t = u = r = None
    try:
        t = Coverage(g, cells, 3, engine=e, **cc.MAP_SEARCH)
        assert t.targets == cells and t.n == cc.MAP_FREE
        bits = sight_bits(e, g, t)
        assert np.array_equal(bits, cc.sight_bits(g, cells, cells))
        against_the_model(t, bits, cc.MAP_SEARCH)
        assert t.history[0] == (cc.MAP_FREE - cc.MAP_THREE["rule"], 3) and t.covered >= cc.MAP_THREE["rule"] > cc.MAP_THREE["additions"] and t.kernel_ms > 0
        assert np.array_equal((t.exposure() > 0).reshape(-1)[t.target_ids], t.mask)
        u = Coverage(g, cells, cc.MAP_ALL["slots"], engine=e, starts=2, rounds=1)
        against_the_model(u, bits, dict(starts=2, rounds=1))
        assert u.complete and u.history[0] == (0, cc.MAP_ALL["rule"]) and len(u.sites) <= cc.MAP_ALL["rule"] < cc.MAP_ALL["additions"]
        r = Coverage(g, cells[::3], 4, targets=cells, by="reach", radius=5.5, keep=[2], engine=e, **cc.MAP_SEARCH)
        against_the_model(r, reach_bits(e, g, r), cc.MAP_SEARCH)
        nf = r.field()
        try:
            assert np.array_equal(nf.fields.reshape(-1)[r.target_ids] <= 5.5, r.mask) and r.sites[0] == 2
        finally:
            nf.close()
    finally:
        for o in (t, u, r):
            if o is not None:
                o.close()
        e.close()


def seeded_cells(g, count, seed):
    free = np.flatnonzero(np.asarray(g).reshape(-1) != 1)
    pick = np.random.default_rng(seed).choice(free, count, replace=False)
    return [(int(v) // g.shape[1], int(v) % g.shape[1]) for v in pick]


@pytest.mark.parametrize("by", ["sight", "reach"])
def test_coverage_on_g256_with_200_sites_and_2000_targets(by):
    from pathfit import Coverage, Engine
    g = gio.grid("g256")[0]
    sites, targets = seeded_cells(g, 200, 1), seeded_cells(g, 2000, 2)
    search = dict(starts=5, rounds=2, seed=9)
    kw = dict(max_range=60.5) if by == "sight" else dict(radius=40.0)
    e = Engine(g)
    t = None
    try:
        t = Coverage(g, sites, 8, targets=targets, by=by, keep=[7, 3], engine=e, **search, **kw)
        bits = sight_bits(e, g, t) if by == "sight" else reach_bits(e, g, t)
        against_the_model(t, bits, search)
        assert t.sites[:2] == [7, 3] and len(t.history) == 3 and t.kernel_ms > 0 and 0 < t.covered
        if by == "sight":
            assert np.array_equal((t.exposure() > 0).reshape(-1)[t.target_ids], t.mask)
    finally:
        if t is not None:
            t.close()
        e.close()


def two_rooms_map():
    """Two rooms joined by two doors; candidate sites and targets in both."""
    g = np.zeros((9, 21), np.uint8)
    g[:, 10] = 1
    g[1, 10] = g[7, 10] = 0
    return g, [(4, 2), (0, 18), (8, 12), (4, 9), (1, 11), (7, 5)], [(8, 18), (8, 3), (2, 5), (6, 14), (0, 0), (4, 20), (1, 9), (7, 11)]


@pytest.mark.parametrize("by", ["sight", "reach"])
def test_sources_in_three_chunks(monkeypatch, by):
    from pathfit import Coverage
    g, sites, targets = two_rooms_map()
    search = dict(starts=4, rounds=2, seed=0)
    kw = {} if by == "sight" else dict(radius=9.0)
    whole = Coverage(g, sites, 2, targets=targets, by=by, **search, **kw)
    monkeypatch.setattr(Coverage, "CHUNK_BYTES", 2 * 189 * (1 if by == "sight" else 8))      # two rows of the 9 x 21 map at a time: chunks of 2, 2 and 2
    t = Coverage(g, sites, 2, targets=targets, by=by, engine=whole.engine, **search, **kw)
    try:
        assert t.chunk == 2 and whole.chunk == 6
        assert np.array_equal(t.masks, whole.masks) and list(t.row) == list(whole.row) and t.history == whole.history
        against_the_model(t, sight_bits(t.engine, g, t) if by == "sight" else reach_bits(t.engine, g, t), search)
    finally:
        for o in (t, whole):
            o.close()


def test_a_target_in_a_sealed_room_stays_uncovered():
    from pathfit import Coverage
    g, sites, targets = two_rooms_map()
    g[:, 15] = 1                                                      # a third room on the right: it holds targets, no site
    sites = [s for s in sites if s[1] < 15]
    targets = [d for d in targets if d[1] != 15]
    shut = [j for j, d in enumerate(targets) if d[1] > 15]
    search = dict(starts=3, rounds=1, seed=0)
    for by, kw in (("sight", {}), ("reach", dict(radius=30.0))):
        t = Coverage(g, sites, None, targets=targets, by=by, **search, **kw)
        try:
            assert t.count == len(sites)
            against_the_model(t, sight_bits(t.engine, g, t) if by == "sight" else reach_bits(t.engine, g, t), search)
            assert shut and not t.complete and not t.mask[shut].any() and t.covered == t.n - len(shut) and len(t.sites) < t.count
        finally:
            t.close()


def test_no_site_covers_anything_and_every_slot_ends_empty():
    """A wall between the sites and the targets: all masks are zero end to end, so every slot ends empty."""
    from pathfit import Coverage
    g = np.zeros((5, 9), np.uint8)
    g[:, 4] = 1
    sites, targets = [(0, 0), (1, 1)], [(0, 8), (4, 8)]
    for by, kw in (("reach", dict(radius=1.0)), ("sight", {})):
        t = Coverage(g, sites, targets=targets, by=by, starts=2, rounds=1, **kw)
        try:
            for again in (False, True):
                if again:
                    t.refresh()
                assert not t.masks.any() and list(t.row) == [-1, -1] and t.sites == [] and t.cells == [] and t.unique == []
                assert t.covered == 0 and t.coverage == 0.0 and not t.complete and not t.mask.any() and t.seen_by.tolist() == [0, 0]
                assert t.history == [(2, 0), (2, 0)] and t.moves == t.drops == 2 and not t.map().any() and t.coverage_of([0, 1]) == 0
            against_the_model(t, np.zeros((2, 2), bool), dict(starts=2, rounds=1))
            if by == "sight":
                assert t.exposure().shape == (5, 9) and not t.exposure().any()
        finally:
            t.close()


def test_refresh_after_a_door_closes():
    from pathfit import Coverage
    g, sites, targets = two_rooms_map()
    search = dict(starts=4, rounds=2, seed=1)
    t = Coverage(g, sites, 1, targets=targets, by="reach", radius=40.0, **search)
    try:
        assert t.complete
        g2 = g.copy()
        g2[1, 10] = g2[7, 10] = 1                                    # both doors shut: one site reaches one room only
        t.engine.update_grid(g2)
        t.refresh()
        against_the_model(t, reach_bits(t.engine, g2, t), search)
        assert not t.complete and 0 < t.covered < t.n
    finally:
        t.close()


def test_a_coverage_a_placement_and_a_visibility_take_turns(eng):
    from pathfit import Coverage, Placement, Visibility
    g = gio.grid("fig7")[0]
    cells = cc.map_cells(g)
    c = Coverage(g, cells[::7], 3, targets=cells[::2], engine=eng, starts=3, rounds=1)
    p = Placement(g, cells[::7], cells[::3], 3, engine=eng, starts=3, rounds=1)
    v = Visibility(g, engine=eng)
    try:
        row, covered, total = list(c.row), c.covered, p.total
        seen = v.seen(cells[:5])
        p.refresh()
        c.refresh()
        assert np.array_equal(v.seen(cells[:5]), seen)
        assert list(c.row) == row and c.covered == covered and p.total == total
        assert np.array_equal((c.exposure() > 0).reshape(-1)[c.target_ids], c.mask)
    finally:
        for o in (c, p, v):
            o.close()


def test_solve_masks(eng):
    from pathfit import Coverage
    masks = np.array([cc.pack(cc.bits(d, 10, 250, 2)) for d in cc.DENSITIES])
    rows = [[3, -1, -1], [3, 9, 0], [3, -1, 5]]
    out = Coverage.solve_masks(eng, masks, rows, 250, fixed=1)
    for b in range(3):
        assert cc.same((out.row[b], out.covered[b], out.value[b], out.status[b], out.info[b]), model(masks[b], 250, rows[b], 1, 48))
    starts = [[-1] * 4] * 2 + [[1, 2, 3, 4]]
    out = Coverage.solve_masks(eng, masks[1], starts, 250, shared=True, max_moves=2)
    for b, row in enumerate(starts):
        assert cc.same((out.row[b], out.covered[b], out.value[b], out.status[b], out.info[b]), model(masks[1], 250, row, 0, 2))
