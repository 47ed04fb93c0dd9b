"""The open-list stress cases themselves (tests/open_list_cases.py), checked on the CPU: the generator is reproducible, the
oracle's answers are well-formed, the searches are large enough to leave the 64-lane window, and the stress variants' bucket
geometry satisfies the inequalities pf_astar_sw.h asserts.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import open_list_cases as olc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    return olc.Reference.get()


def build_module():
    spec = importlib.util.spec_from_file_location("pathfit_build", os.path.join(ROOT, "maaco-path-planing_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_is_reproducible(ref):
    again = olc.maps()
    assert list(again) == list(ref.maps) == ["empty96", "blocks128", "sparse128", "rooms64", "g256"]
    for name, g in ref.maps.items():
        assert np.array_equal(g, again[name]) and g.dtype == np.uint8
        s, t, av = ref.pairs(name)
        s2, t2, av2 = olc.pairs(name, again[name], ref.oracle(name))
        assert np.array_equal(s, s2) and np.array_equal(t, t2) and len(s) == olc.N_PAIRS
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(av, av2))
    a, b = olc.decode_cases(ref.maps["blocks128"]), olc.decode_cases(again["blocks128"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_pairs_hold_the_edge_cases(ref):
    for name, g in ref.maps.items():
        flat = g.reshape(-1)
        C = g.shape[1]
        s, t, av = ref.pairs(name)
        free = np.flatnonzero(flat != 1)
        assert (s[0], t[0]) == (free[0], free[-1]) and (s[1], t[1]) == (free[-1], free[0])          # corner to corner
        assert s[2] == t[2] and s[3] == t[3]                                                           # start == target
        assert all(olc._cheb(int(s[i]), int(t[i]), C) == 1 for i in (4, 5))                            # adjacent cells
        if (flat == 1).any():
            assert flat[t[6]] == 1 and flat[s[7]] == 1                                                 # an endpoint on an obstacle
        kinds = [sum(a is None for a in av), sum(a is not None and len(a) == 8 for a in av), sum(a is not None and len(a) != 8 for a in av)]
        assert min(kinds) >= 8, kinds                                                                  # none / small / random and path-shaped
    s, t, _ = ref.pairs("rooms64")
    assert (olc.in_room(s) != olc.in_room(t)).sum() >= 12       # the reference exhausts its side of the wall; the engine's component test answers


@pytest.mark.parametrize("name", ["empty96", "blocks128", "sparse128", "rooms64", "g256"])
def test_oracle_answers_are_well_formed_and_leave_the_window(ref, name):
    g = ref.maps[name]
    flat, C = g.reshape(-1), g.shape[1]
    s, t, av = ref.pairs(name)
    for variant, ad, rs, _, _ in olc.astar_runs(name):
        res = ref.astar(name, variant, ad, rs)
        for i, (p, st) in enumerate(res):
            assert (len(p) == 0) == (st[5] != 0), (name, variant, i)
            if len(p):
                assert p[0] == s[i] and p[-1] == t[i] and (flat[p] != 1).all()
                step = np.maximum(np.abs(np.diff(p // C)), np.abs(np.diff(p % C)))
                assert (step == 1).all() if len(p) > 1 else s[i] == t[i]
                if not ad:
                    assert (np.abs(np.diff(p // C)) + np.abs(np.diff(p % C)) == 1).all()
                if av[i] is not None and len(p) > 2:
                    assert not np.isin(p[1:-1], av[i]).any()
        # an open list of more than 64 + 8 entries cannot live in the window alone: at least half of the searches push that many
        big = sum(int(st[1]) > olc.WINDOW + olc.HEADS for _, st in res)
        assert 2 * big >= len(res), (name, variant, ad, rs, big)
        # the pairs an avoid wall separates: one component (a path exists without the wall), endpoints outside the wall, no path with
        # it, and more than FLOOD_CELLS cells popped on the way there -- the pop loop has to drain the start's whole side
        o = ref.oracle(name, ad, rs)
        for i in olc.SEALED:
            p, st = res[i]
            assert len(p) == 0 and st[0] > olc.FLOOD_CELLS and st[1] > olc.WINDOW + olc.HEADS, (name, variant, ad, rs, i, st)
            assert len(o.astar(int(s[i]), int(t[i]), None, variant)[0]) > 1 and not np.isin([s[i], t[i]], av[i]).any()
            assert o.astar(int(t[i]), int(s[i]), av[i], 0)[1][0] > olc.FLOOD_CELLS          # the goal's side is no small pocket either
    if name == "rooms64":
        fails = sum(len(p) == 0 for p, _ in ref.astar(name, 0))      # (by the oracle; the engine's component test answers the room's)
        assert fails >= 12
    if name == "g256":
        for variant in (0, 1):
            gs, gt, gav, gp, gpops, gpushes = olc.golden_g256(variant)
            assert len(gs) >= 4
            o = ref.oracle(name)
            for i in range(len(gs)):                             # the oracle and the reference's own record agree
                p, st = o.astar(int(gs[i]), int(gt[i]), gav[i], variant)
                assert np.array_equal(p, gp[i]) and (len(p) <= 1 or (st[0] == gpops[i] and st[1] == gpushes[i]))


def test_decode_and_mpa_references_are_well_formed(ref):
    d = ref.decodes()
    assert len(d["one"]) == 64 and len(d["multi"]) == 64 and d["wp"].shape == (64, 5)
    assert sum(len(p) > 0 for p in d["one"]) >= 8 and sum(len(p) > 0 for p in d["multi"]) >= 8
    for p, st in zip(d["one"] + d["multi"], d["one_stats"] + d["multi_stats"]):
        assert st.shape == (5,) and (len(p) > 0) == bool(np.isfinite(st[4]))
    m = ref.mpa()
    assert len(m["pop"]) == 32 and len(m["curve"]) == 7 and m["fit"] == sorted(m["fit"])
    assert m["curve"][-1] < m["curve"][0] and len({p.tobytes() for p in m["pop"]}) > 1   # rebuilt paths were accepted: the MPA connector ran


def test_variant_flags_satisfy_the_header_asserts():
    """The three static_asserts of pf_astar_sw.h, recomputed from the numbers in build.py's table and the header's defaults."""
    mod = build_module()
    assert list(mod.VARIANTS) == olc.VARIANT_NAMES
    import re
    csrc = os.path.join(ROOT, "maaco-path-planing_amd", "csrc")
    src, dev = open(os.path.join(csrc, "pf_astar_sw.h")).read(), open(os.path.join(csrc, "pf_device.h")).read()

    def define(text, name):
        """The value of `#define name <integer expression>` (digits, + * and parentheses only)."""
        expr = re.search(r"^#define\s+%s\s+([0-9()+*\s.]+?)\s*(?:/\*.*)?$" % name, text, re.M).group(1)
        return eval(expr, {"__builtins__": {}})
    POOL_STRIDE, SORT_LDS, DUMP = define(dev, "PF_POOL_STRIDE"), define(src, "PF_SORT_LDS"), define(src, "PF_SW_DUMP")
    defaults = {k: define(src, k) for k in ("PF_SW_Q", "PF_SW_NBK", "PF_SW_CAP", "PF_SW_SPILL", "PF_SELECT_MIN")}
    assert defaults == dict(PF_SW_Q=256.0, PF_SW_NBK=1024, PF_SW_CAP=256, PF_SW_SPILL=16384, PF_SELECT_MIN=256)   # the shipped geometry
    known = set(defaults) | {"PF_OPEN_PATHS"}
    for name in ["default"] + olc.VARIANT_NAMES:
        flags = [] if name == "default" else mod.variant_flags(name)
        v = dict(defaults)
        for f in flags:
            assert f.startswith("-D")
            k, _, val = f[2:].partition("=")
            assert k in known, f                                  # PF_RUN_SORT / PF_EARLY_REFILL / PF_ROTATE keep their shipped values
            if k in v:
                v[k] = float(val) if k == "PF_SW_Q" else int(val)
        assert name == "default" or "-DPF_OPEN_PATHS" in flags
        nbk, cap, spill, q = v["PF_SW_NBK"], v["PF_SW_CAP"], v["PF_SW_SPILL"], v["PF_SW_Q"]
        assert nbk & (nbk - 1) == 0
        assert float(nbk) >= 2.8285 * q + 1.0
        assert 4 * (nbk + 1) <= SORT_LDS
        assert ((nbk + 1) * cap + spill + DUMP) * 16 <= POOL_STRIDE
        assert os.path.basename(mod.variant_path(name)) == "libpathfit_%s.so" % name
    assert src.count("static_assert(") == 4                      # the three on the geometry (above) and the pop loop's NH == 7
    names = [l.split(",")[0].strip() for l in src.split("enum {", 1)[1].split("PF_OP_N", 1)[0].splitlines() if l.strip().startswith("OP_")]
    assert [n[3:].lower() for n in names] == olc.COUNTERS and len(names) == 21    # the header's counters, in its order


def test_facades_raise_on_a_scratch_overflow_of_their_own_search():
    """A search that comes back status 3 although its row holds R * C cells ran out of open-list scratch: MPA's initial search and
    the connector facades must raise, not answer "no path".  (No stress variant overflows MPA's own start -> target search, so
    the engine is a stand-in here; tests/test_gpu_open_list_stress.py reaches the connector facades on the GPU.)"""
    import pathfit

    class Overflowing:
        R = C = 8
        calls = 0

        def mpa_setup(self, mp, sp):
            pass

        def astar_host(self, variant, starts, targets, avoid=None, path_cap=None, **kw):
            self.calls += 1
            return [np.zeros(0, np.int32)], np.array([3], np.int32)

    g = np.zeros((8, 8), np.int64)
    g[0, 0], g[7, 7] = 2, 3
    e = Overflowing()
    with pytest.raises(RuntimeError, match="capacity overflow in the initial search"):
        pathfit.MPA(g, 4, 1, engine=e)
    assert e.calls == 1                                          # path_cap is R * C already: nothing to grow, no second try
    for cls in (pathfit.AStarSolver, pathfit.DijkstraSolver):
        with pytest.raises(RuntimeError, match="open-list scratch overflow"):
            cls(g, engine=e).solve()
