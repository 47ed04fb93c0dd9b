"""The build's view of csrc/: every translation unit is compiled into the one library, and every source and header counts for the
staleness rule -- so that a new unit or header cannot be forgotten (runs on a CPU-only host, compiles nothing)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "maaco-path-planing_amd")
sys.path[:0] = [PKG]

import build  # noqa: E402

CSRC = os.path.join(PKG, "csrc")


def csrc(ext):
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(ext))


def test_every_unit_is_compiled_and_watched():
    units = csrc(".hip")
    assert len(units) >= 2
    cmd = build._cmd("x", [])
    deps = {os.path.abspath(d) for d in build.DEPS}
    for u in units:
        assert [os.path.abspath(a) for a in cmd].count(u) == 1, u
        assert u in deps, u


def test_every_header_is_watched():
    deps = {os.path.abspath(d) for d in build.DEPS}
    headers = csrc(".h")
    assert headers
    for h in headers:
        assert h in deps, h
    assert os.path.join(ROOT, "include", "pathfit.h") in deps


def test_one_command_one_output():
    cmd = build._cmd("x", ["-DPF_CC_TILED=0"])
    assert cmd.count("-o") == 1 and cmd[cmd.index("-o") + 1] == "x"
    assert "-DPF_CC_TILED=0" in cmd and "-c" not in cmd
