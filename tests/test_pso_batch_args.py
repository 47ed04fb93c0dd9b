"""PSOBatch argument checks: ValueError with the `PSOBatch:` prefix before any Engine exists (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import pso_batch

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(pso_batch, "Engine", boom)


def make(g, iterations=3, n=10, w=5, **kw):
    from pathfit import PSOBatch
    return PSOBatch(g, iterations, n, w, 0.7, 1.5, 1.5, **kw)


def test_empty_seed_list(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^PSOBatch: seeds is empty"):
        make(g, seeds=[])
    with pytest.raises(ValueError, match="^PSOBatch: seeds is empty"):
        make(g)


def test_seed_range(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=r"^PSOBatch: seeds must be in \[0, 2\^64\)"):
        make(g, seeds=[1, -1])
    with pytest.raises(ValueError, match=r"^PSOBatch: seeds must be in \[0, 2\^64\)"):
        make(g, seeds=[1 << 64])


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_list_lengths_must_match(no_engine, which):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=f"^PSOBatch: 2 {which} for 3 seeds"):
        make(g, seeds=[1, 2, 3], **{which: [(0, 0), (0, 1)]})
    with pytest.raises(ValueError, match=f"^PSOBatch: 2 {which} for 1 seeds"):
        make(g, seeds=[1], **{which: [(0, 0), (0, 1)]})


@pytest.mark.parametrize("which", ["starts", "targets"])
@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3)])
def test_out_of_range(no_engine, which, cell):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^PSOBatch: .* is outside the 20x20 grid"):
        make(g, seeds=[1, 2], **{which: [(0, 0), cell]})


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_on_an_obstacle(no_engine, which):
    g, _, _ = gio.grid("fig7")
    r, c = (int(v) for v in np.argwhere(np.asarray(g) == 1)[0])
    with pytest.raises(ValueError, match=rf"^PSOBatch: {which}\[1\] = \({r}, {c}\) is on an obstacle"):
        make(g, seeds=[1, 2], **{which: [(0, 0), (r, c)]})


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_not_a_pair(no_engine, which):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=rf"^PSOBatch: {which}\[0\] must be an \(r, c\) pair"):
        make(g, seeds=[1], **{which: [7]})


def test_sizes(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^PSOBatch: num_particles must be >= 1"):
        make(g, n=0, seeds=[1])
    with pytest.raises(ValueError, match="^PSOBatch: num_waypoints_per_particle must be >= 1"):
        make(g, w=0, seeds=[1])
    with pytest.raises(ValueError, match="^PSOBatch: num_iterations must be >= 0"):
        make(g, iterations=-1, seeds=[1])
    with pytest.raises(ValueError, match="^PSOBatch: grid must be 2-D"):
        make(np.zeros(16, int), seeds=[1])


@pytest.mark.parametrize("marker, what", [(2, "Start"), (3, "Target")])
def test_missing_marker(no_engine, marker, what):
    """starts / targets default to the grid's markers: a grid without one fails in the solo class's words, prefixed."""
    g, _, _ = gio.grid("fig7")
    h = np.array(g)
    h[h == marker] = 0
    with pytest.raises(ValueError, match=f"^PSOBatch: PSO: {what} node not found"):
        make(h, seeds=[1])
    # ... and is fine when every swarm names its own cells: the check then reaches the device (patched out here)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(h, seeds=[1], starts=[(0, 0)], targets=[(19, 19)])


def test_valid_arguments_reach_the_device(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, seeds=[4, 5], starts=[(0, 0), (19, 19)], targets=[(19, 19), (0, 0)])
