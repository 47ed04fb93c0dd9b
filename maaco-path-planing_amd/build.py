"""Build libpathfit.so (hand-written HIP for gfx950) in-tree with hipcc.

    python maaco-path-planing_amd/build.py [--force]

hipcc cross-compiles gfx950 without a GPU; the .so travels to the GPU box with
the repo snapshot.  PF_EXTRA_FLAGS adds compiler flags:
-DPF_TRACE / -DPF_STAMPS / -DPF_WALK_PROBE the diagnostic builds of scripts/.  -ffp-contract=off: the reference's arithmetic is unfused
IEEE double and bit-exact path parity depends on it.

    python maaco-path-planing_amd/build.py --variants [--force]

also builds the stress variants of the A* open list (VARIANTS below) into lib/stress/libpathfit_<name>.so: the shipped code under
a bucket geometry that makes its rare branches common, with the branch counters of -DPF_OPEN_PATHS compiled in
(tests/test_gpu_open_list_stress.py runs tests/open_list_cases.py against each), and the stress variants of the parallel closed-set
engine (SETTLE_VARIANTS: tests/test_gpu_settle_stress.py runs tests/settle_cases.py against each), the assignment solver's
workgroup form at every m (ASSIGN_VARIANTS: tests/test_gpu_assign.py holds it against the shipped library), and the coverage
search's other deal with the planes in HBM from three words on (COVER_VARIANTS: tests/test_gpu_cover.py does the same), and the
sight graph's field with its labels in HBM from 65 nodes on (SIGHT_VARIANTS: tests/test_gpu_sight.py does the same).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# the translation units of the one library: the solvers, and the field family in a device code object of its own
SRCS = [os.path.join(HERE, "csrc", f) for f in ("pathfit.hip", "pathfit_fields.hip")]
DEPS = SRCS + [os.path.join(HERE, "csrc", f) for f in sorted(os.listdir(os.path.join(HERE, "csrc"))) if f.endswith(".h")] + \
       [os.path.join(os.path.dirname(HERE), "include", "pathfit.h")]
OUT = os.path.join(HERE, "lib", "libpathfit.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17",
         "-Wall", "-Wno-unused-function"]
# Stress variants of the open list (pf_astar_sw.h): name -> the flags added to FLAGS, and what they make common.  Every variant
# carries -DPF_OPEN_PATHS; PF_RUN_SORT, PF_EARLY_REFILL and PF_ROTATE keep their shipped values.
VARIANTS = {
    "cap8": ["-DPF_SW_CAP=8"],                                                             # full buckets, spill list, respill
    "wide64": ["-DPF_SW_Q=16.0", "-DPF_SW_NBK=64", "-DPF_SW_CAP=64"],                      # buckets of (nearly) 64, concatenation, wrap
    "wide256": ["-DPF_SW_Q=16.0", "-DPF_SW_NBK=64", "-DPF_SW_CAP=256", "-DPF_SELECT_MIN=65"],   # buckets > 64, pivot selection, evictions
    "spill256": ["-DPF_SW_CAP=8", "-DPF_SW_SPILL=256"],                                    # the spill list filling up: status 3
}
# Stress variants of the parallel closed-set engine (pf_settle.h), the same way: its shipped code under a band geometry that makes its
# rare branches common.  The branch counters of -DPF_OPEN_PATHS cover both engines.
SETTLE_VARIANTS = {
    "st_cap4": ["-DPF_SETTLE_CAP=4"],                                                      # full buckets: hand-backs from the main loop
    "st_q1": ["-DPF_ST_Q=1.0"],                                                            # bands of hundreds of nodes: the partial take, many-band takes
    "st_q96": ["-DPF_ST_Q=96.0"],                                                          # pushes beyond the circular band range
    "st_touch": ["-DPF_ST_TOUCH_NUM=1", "-DPF_ST_TOUCH_DEN=4"],                           # the touched list filling up on the far pairs
    "st_wide2": ["-DPF_ST_WIDE=2", "-DPF_ST_Q=1.0"],                                       # two nodes per lane and trip
}
# The stress variant of the assignment solver (pf_assign.h): a workgroup per problem at every m, where the shipped library runs a
# wavefront per problem up to 64 columns -- the workgroup form with one to sixty-four live columns and idle wavefronts.
ASSIGN_VARIANTS = {
    "as_group": ["-DPF_ASSIGN_WAVE_M=0"],
}
# The stress variant of the coverage search (pf_cover.h): the deal that is not shipped (a lane per (site group, slot) walking the
# words), and the planes of a start in the handle's scratch instead of LDS from W = 3 on, so that small cases run the HBM form.
COVER_VARIANTS = {
    "cv_lanes": ["-DPF_COVER_DEAL=0", "-DPF_COVER_LDS_WORDS=2"],
}
# The stress variant of the sight graph's field (pf_sight.h): the labels of a set in the output row (HBM) instead of LDS from 65
# nodes on -- the form that is not shipped, reachable at small sizes, and both sides of its switch at 64 / 65 nodes.
SIGHT_VARIANTS = {
    "sg_hbm": ["-DPF_SIGHT_LDS_NODES=64"],
}
VARIANT_COMMON = ["-DPF_OPEN_PATHS"]
MAX_JOBS = 16


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in DEPS)


def _cmd(out, extra):
    return [HIPCC] + FLAGS + os.environ.get("PF_EXTRA_FLAGS", "").split() + list(extra) + ["-o", out] + SRCS


def build(force=False, verbose=False):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not force and not _stale(OUT):
        return OUT
    cmd = _cmd(OUT, [])
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return OUT


def variant_path(name):
    return os.path.join(HERE, "lib", "stress", "libpathfit_%s.so" % name)


def variant_flags(name):
    for group in (VARIANTS, SETTLE_VARIANTS, ASSIGN_VARIANTS, COVER_VARIANTS, SIGHT_VARIANTS):
        if name in group:
            return VARIANT_COMMON + group[name]
    raise KeyError(name)


def build_variant(name, force=False, verbose=False):
    """lib/stress/libpathfit_<name>.so: the main library's flags plus the variant's, the same staleness rule."""
    return build_variants([name], force, verbose)[0]


def build_variants(names=None, force=False, verbose=False):
    """Several variants at once: one hipcc child each, at most MAX_JOBS at a time."""
    names = list(VARIANTS) + list(SETTLE_VARIANTS) + list(ASSIGN_VARIANTS) + list(COVER_VARIANTS) + list(SIGHT_VARIANTS) if names is None else list(names)
    outs = [variant_path(n) for n in names]
    os.makedirs(os.path.dirname(variant_path("x")), exist_ok=True)
    todo = [(n, o) for n, o in zip(names, outs) if force or _stale(o)]
    failed = []
    for i in range(0, len(todo), MAX_JOBS):
        procs = []
        for n, o in todo[i:i + MAX_JOBS]:
            cmd = _cmd(o, variant_flags(n))
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((n, subprocess.Popen(cmd)))
        failed += [n for n, p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, "hipcc (stress variants: %s)" % ", ".join(failed))
    return outs


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    if "--variants" in sys.argv:
        print("\n".join(build_variants(force="--force" in sys.argv, verbose=True)))
