"""The settling engine's stress cases themselves (tests/settle_cases.py), checked on the CPU: the cases are well formed, the oracle
answers them, build.py's table matches the program's list and the header's knobs, and the CPU facts the GPU assertions of
tests/test_gpu_settle_stress.py rest on hold: how full the bands of exact labels get at the shipped and at the stress band widths, how
many cells the far and the short searches touch, and -- through the CPU model of scripts/settle/settle_study.c -- that the pairs hold
A* searches with irregular nodes whose path survives and searches whose fixpoint path differs from the sequential one.  No GPU."""
import ctypes as C
import importlib.util
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import field_checkers as fc
import open_list_cases as olc
import settle_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "maaco-path-planing_amd", "csrc")


@pytest.fixture(scope="module")
def ref():
    return olc.Reference.get()


def build_module():
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(ROOT, "maaco-path-planing_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cases_are_well_formed(ref):
    assert len(sc.COUNTERS) == len(set(sc.COUNTERS)) == 21
    assert set(sc.GEOMETRY) == {"default"} | set(sc.VARIANT_NAMES)
    for name in olc.MAP_NAMES:
        runs = sc.astar_runs(name)
        assert {v for v, _, _ in runs} == set(sc.CLOSED) and len(runs) == (6 if name == "blocks128" else 2)
    assert {(ad, rs) for _, ad, rs in sc.astar_runs("blocks128")} == set(olc.POLICIES)
    for variant in sc.CLOSED:
        cases = sc.fit_cases(ref, variant)
        assert len(cases) == sc.FIT_CASES and all(len(p) > 2 and p[0] == s and p[-1] == t for s, t, _, p in cases)
        assert sum(av is not None for _, _, av, _ in cases) >= 3 and max(len(p) for _, _, _, p in cases) > 64     # more than one lane round of the write-out
    ss, tt = olc.short_pairs(ref.maps["rooms64"])
    o = ref.oracle("rooms64")
    flat = ref.maps["rooms64"].reshape(-1)
    # the one-search launches that reach the engine: the label epoch of slot 0 runs out once, not twice
    n = sum(sc.reaches_engine(o, flat, int(ss[k % 48]), int(tt[k % 48]), None, o.astar(int(ss[k % 48]), int(tt[k % 48]), None, 0)[0], 0) for k in range(sc.WIPE_LAUNCHES))
    assert 127 <= n < 2 * 126


@pytest.mark.parametrize("name", olc.MAP_NAMES)
def test_oracle_answers_and_the_searches_that_reach_the_engine(ref, name):
    g = ref.maps[name]
    flat = g.reshape(-1)
    s, t, av = ref.pairs(name)
    for variant, ad, rs in sc.astar_runs(name):
        o = ref.oracle(name, ad, rs)
        res = ref.astar(name, variant, ad, rs)
        reach = [sc.reaches_engine(o, flat, int(s[i]), int(t[i]), av[i], res[i][0], variant) for i in range(len(s))]
        assert all(reach[i] and not len(res[i][0]) for i in olc.SEALED), (name, variant, ad, rs)       # nothing answers the sealed pairs beforehand
        assert not reach[2] and not reach[3] and not reach[6] and not reach[7] if (flat == 1).any() else not reach[2]   # start == target, an endpoint on an obstacle
        assert sum(reach) >= 24 and sum(1 for i in range(len(s)) if reach[i] and len(res[i][0])) >= 16, (name, variant, sum(reach))
    if name == "rooms64":                                       # the room's pairs: another component, answered before the engine
        o = ref.oracle(name)
        res = ref.astar(name, 0)
        assert sum(1 for i in range(8, 24) if not sc.reaches_engine(o, flat, int(s[i]), int(t[i]), av[i], res[i][0], 0)) >= 12
    if name == "blocks128":
        d = ref.decodes()
        o = ref.oracle(name)
        one = [sc.decode_reached(o, flat, 0, g.size - 1, w) for w in d["wp"]]
        multi = [sc.decode_reached(o, flat, int(a), int(b), w) for a, b, w in zip(d["ms"], d["mt"], d["wpm"])]
        assert all(0 <= k <= 6 for k in one + multi) and sum(one) >= 64 and sum(multi) >= 64
        assert all((k == 6) >= (len(p) > 0) for k, p in zip(one, d["one"]))          # a whole chain ran every link (unless a link is one cell long)


def defines(text, names):
    out = {}
    for n in names:
        m = re.search(r"^#define\s+%s\s+([0-9.]+)\s" % n, text, re.M)
        out[n] = float(m.group(1)) if "." in m.group(1) else int(m.group(1))
    return out


def test_variant_table_matches_the_program_and_the_header():
    mod = build_module()
    assert list(mod.SETTLE_VARIANTS) == sc.VARIANT_NAMES and list(mod.VARIANTS) == olc.VARIANT_NAMES
    assert not set(mod.SETTLE_VARIANTS) & set(mod.VARIANTS)
    src = open(os.path.join(CSRC, "pf_settle.h")).read()
    d = defines(src, ["PF_SETTLE_CAP", "PF_ST_Q", "PF_ST_NBK", "PF_ST_WIDE", "PF_ST_TOUCH_NUM", "PF_ST_TOUCH_DEN"])
    assert dict(Q=d["PF_ST_Q"], WIDE=d["PF_ST_WIDE"], CAP=d["PF_SETTLE_CAP"], NBK=d["PF_ST_NBK"], TOUCH=(d["PF_ST_TOUCH_NUM"], d["PF_ST_TOUCH_DEN"])) == sc.SHIPPED
    assert "PF_ST_TOUCHED_CAP(RC)" in open(os.path.join(CSRC, "pathfit.hip")).read()
    key = {"PF_SETTLE_CAP": "CAP", "PF_ST_Q": "Q", "PF_ST_WIDE": "WIDE"}
    for name in sc.VARIANT_NAMES:
        flags = mod.variant_flags(name)
        assert flags[0] == "-DPF_OPEN_PATHS" and all(f.startswith("-D") for f in flags)
        got = {}
        for f in flags[1:]:
            k, _, val = f[2:].partition("=")
            assert k in key or k in ("PF_ST_TOUCH_NUM", "PF_ST_TOUCH_DEN"), f
            got[k] = float(val) if k == "PF_ST_Q" else int(val)
        want = dict(sc.GEOMETRY[name])
        touch = want.pop("TOUCH", None)
        assert {key[k]: v for k, v in got.items() if k in key} == want, name
        assert touch == ((got["PF_ST_TOUCH_NUM"], got["PF_ST_TOUCH_DEN"]) if "PF_ST_TOUCH_NUM" in got else None)
        geo = sc.geometry(name)
        assert 1 <= geo["CAP"] <= 1024 and 1 <= geo["TOUCH"][0] <= 2 * geo["TOUCH"][1] and geo["WIDE"] in (1, 2)   # the header's static_asserts
        assert os.path.basename(mod.variant_path(name)) == "libpathfit_%s.so" % name
    # the header's counters, in its order
    names = [l.split(",")[0].strip() for l in src.split("enum {", 1)[1].split("PF_ST_OP_N", 1)[0].splitlines() if l.strip().startswith("ST_")]
    assert [n[3:].lower() for n in names] == sc.COUNTERS
    # the binding
    from pathfit import _lib
    assert "pf_selftest_settle_paths" in _lib.SYMBOLS


def reach_of_a_push(q):
    """The farthest band, counted from the current one, a push can ask for: a trip takes bands up to bcur + 63, an entry of band b
    has f < (b + 1) / Q, and a child lies at most 2 sqrt(2) above its parent in f (one move costs at most sqrt(2) and raises h by at
    most the same; the roundings are many orders below the 1 / Q that is left)."""
    return 63 + math.ceil(2.0 * math.sqrt(2.0) * q)


def test_band_range_argument():
    """`back_range` is exempt in every build with Q <= 64 and promised at Q = 96."""
    for name in ["default"] + sc.VARIANT_NAMES:
        geo = sc.geometry(name)
        assert (reach_of_a_push(geo["Q"]) < geo["NBK"]) == (geo["Q"] <= 64.0), name
    assert reach_of_a_push(64.0) == 245 and reach_of_a_push(96.0) == 335
    # the winner list: 64 K nodes x 8 moves against its capacity (pf_settle.h: 512, or 768 when K = 2)
    assert 64 * 1 * 8 <= 512 and 64 * 2 * 8 > 768


@pytest.fixture(scope="module")
def labels(ref):
    """Exact labels (a heap Dijkstra) from two case sources per map: the corner of pair 0 and the start of the far pair 8."""
    out = {}
    for name, g in ref.maps.items():
        mm = fc.move_masks(g, 1, 1)
        s, _, _ = ref.pairs(name)
        out[name] = [fc.reference_dijkstra(g, mm, int(s[i]))[0].reshape(-1) for i in (0, 8)]
    return out


def fullest_band(lab, q):
    b = np.floor(lab[np.isfinite(lab)] * q).astype(np.int64)
    return int(np.bincount(b).max())


# the maps the GPU assertions on the band takes rely on: bands of exact labels above 64 K at the stress Q
RELY_Q1 = ["empty96", "blocks128", "sparse128", "g256"]


def test_band_histograms(labels):
    for name, labs in labels.items():
        # shipped Q: no band of exact labels fills a trip (the partial take is out of a Dijkstra's reach), yet bands of twice
        # st_cap4's 4 entries exist on every map
        full = [fullest_band(lab, 64.0) for lab in labs]
        assert 2 * sc.geometry("st_cap4")["CAP"] <= max(full) < 64, (name, full)
        assert max(fullest_band(lab, 96.0) for lab in labs) < 64
    for build in ("st_q1", "st_wide2"):
        geo = sc.geometry(build)
        for name in RELY_Q1:
            for lab in labels[name]:
                assert 64 * geo["WIDE"] < fullest_band(lab, geo["Q"]) < geo["CAP"], (build, name, fullest_band(lab, geo["Q"]))


def test_touched_list_populations(ref):
    """st_touch: the engine relaxes every cell the sequential loop ever pushed at least once (it expands every node below the goal's
    key), so a search that pushes more than the cap overflows the touched list; the short searches stay below half of it."""
    num, den = sc.geometry("st_touch")["TOUCH"]
    for name, g in ref.maps.items():
        cap = g.size * num // den
        for variant in sc.CLOSED:
            res = ref.astar(name, variant)
            assert sum(int(st[1]) - 1 > cap for _, st in res) >= 4, (name, variant)
            assert sum(0 < int(st[1]) + int(st[3]) < cap // 2 and len(p) > 1 for p, st in res) >= 2 or name != "blocks128"
        o = ref.oracle(name)
        ss, tt = olc.short_pairs(g)
        for variant in sc.CLOSED:
            for a, b in zip(ss, tt):
                st = o.astar(int(a), int(b), None, variant)[1]
                assert 2 * (int(st[1]) + int(st[3])) <= cap, (name, variant, a, b, st)


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    """scripts/settle/settle_study.c built into a temporary directory, the way scripts/settle/run_study.py builds it."""
    if not shutil.which("gcc"):
        pytest.skip("no C compiler for the CPU model")
    so = str(tmp_path_factory.mktemp("settle_study") / "libsettle_study.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so,
                           os.path.join(ROOT, "scripts", "settle", "settle_study.c"), "-lm", "-Wno-unused-function", "-Wno-misleading-indentation"])
    L = C.CDLL(so)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.orc_ws_create.restype = vp; L.orc_ws_create.argtypes = [i32, i32]
    L.settle_v0.restype = i64; L.settle_v0.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, i32, vp, i64, vp, vp]
    L.ref_v0_labels.restype = i64; L.ref_v0_labels.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, vp, i64, vp, vp]
    return L


def goal_cone(mm, lab, s, t, mask):
    """(irregular nodes of the region, irregular nodes in the goal's cone of argmin parents) from the fixpoint's labels `lab` (inf: not
    labelled), restating pf_settle.h's regularity pass and cone_walk: p is an argmin parent of x when its offer is x's label and it is
    expanded (f(p) <= F); x is irregular when none of them has f(p) <= f(x)."""
    Cc = mm.shape[1]
    tr, tc = divmod(t, Cc)
    m = mm.reshape(-1)
    F = lab[t]

    def f(x):
        return lab[x] + math.sqrt(float((x // Cc - tr) ** 2 + (x % Cc - tc) ** 2))

    def parents(x):
        ps = [x + fc.DR[k] * Cc + fc.DC[k] for k in range(8) if (m[x] >> k) & 1 and lab[x + fc.DR[k] * Cc + fc.DC[k]] + fc.W[k] == lab[x]]
        return [p for p in ps if p != t and not (mask is not None and mask[p] and p != s) and f(p) <= F]

    def irregular(x):
        return x != s and not any(f(p) <= f(x) for p in parents(x))
    region = [int(x) for x in np.flatnonzero(np.isfinite(lab)) if x != s and (x == t or f(x) <= F)]
    seen, todo, dirty = {t}, [t], 0
    while todo:
        x = todo.pop()
        dirty += irregular(x)
        for p in parents(x) if x != s else []:
            if p not in seen and p != s:
                seen.add(p); todo.append(p)
    return sum(irregular(x) for x in region), dirty


def test_pairs_hold_all_three_outcomes_of_the_certificate(ref, study):
    """Over the 5 x 48 pairs, A* under the default policy: searches with irregular nodes whose fixpoint path is the sequential one
    (the cone walk may certify them), searches whose fixpoint path differs (they MUST be handed back), and regular ones; Dijkstra has
    no irregular node anywhere (with h = 0 an argmin parent always has the smaller key).  Both outcomes of the cone walk occur among
    searches that the st_touch build does not hand back beforehand: their sequential pushes and decrease-keys stay below two thirds
    of its touched list."""
    irregular = differs = regular = clean_small = dirty_small = 0
    num, den = sc.geometry("st_touch")["TOUCH"]
    for name, g in ref.maps.items():
        occ = np.ascontiguousarray((g == 1).astype(np.uint8))
        R, Cc = occ.shape
        ws = study.orc_ws_create(R, Cc)
        s, t, av = ref.pairs(name)
        o = ref.oracle(name)
        out_a, out_b, ga, gb = np.zeros(R * Cc, np.int32), np.zeros(R * Cc, np.int32), np.zeros(R * Cc), np.zeros(R * Cc)
        for i in range(len(s)):
            mask = o.avoid_mask(av[i]) if av[i] is not None else None
            for hzero in (0, 1):
                sa, sb = np.zeros(10, np.int64), np.zeros(6, np.int64)
                na = study.settle_v0(occ.ctypes.data, R, Cc, 1, 1, int(s[i]), int(t[i]), mask.ctypes.data if mask is not None else None, hzero,
                                     out_a.ctypes.data, R * Cc, sa.ctypes.data, ga.ctypes.data)
                nb = study.ref_v0_labels(ws, occ.ctypes.data, R, Cc, 1, 1, int(s[i]), int(t[i]), mask.ctypes.data if mask is not None else None, hzero,
                                         out_b.ctypes.data, R * Cc, sb.ctypes.data, gb.ctypes.data)
                want = ref.astar(name, 2 if hzero else 0)[i][0]
                assert np.array_equal(out_b[:max(nb, 0)], want)                   # the model's sequential side is the oracle
                same = na == nb and np.array_equal(out_a[:max(na, 0)], out_b[:max(nb, 0)])
                if hzero:
                    assert sa[1] == 0 and same, (name, i)
                elif nb > 1:
                    if sa[1] > 0:
                        n_irr, in_cone = goal_cone(fc.move_masks(g, 1, 1), ga, int(s[i]), int(t[i]), mask)
                        assert n_irr == sa[1] and (in_cone > 0 or same), (name, i, n_irr, in_cone)     # the model's count; a clean cone keeps the path
                        small = 3 * (int(sb[1]) + int(sb[3])) <= 2 * (g.size * num // den)
                        clean_small += small and in_cone == 0
                        dirty_small += small and in_cone > 0
                    irregular += sa[1] > 0
                    differs += not same
                    regular += sa[1] == 0
                    assert same or sa[1] > 0, (name, i)                           # a path can differ only where a node is irregular
    assert differs >= 1 and irregular > differs and regular >= 100, (irregular, differs, regular)
    assert clean_small >= 2 and dirty_small >= 2, (clean_small, dirty_small)
