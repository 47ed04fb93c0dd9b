"""GABatch argument checks: ValueError with the `GABatch:` prefix before any Engine exists (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import ga_batch

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(ga_batch, "Engine", boom)


def make(g, generations=3, n=10, w=5, **kw):
    from pathfit import GABatch
    return GABatch(g, generations, n, w, 0.1, 0.8, **kw)


def test_empty_seed_list(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^GABatch: seeds is empty"):
        make(g, seeds=[])
    with pytest.raises(ValueError, match="^GABatch: seeds is empty"):
        make(g)


def test_seed_range(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=r"^GABatch: seeds must be in \[0, 2\^64\)"):
        make(g, seeds=[1, -1])
    with pytest.raises(ValueError, match=r"^GABatch: seeds must be in \[0, 2\^64\)"):
        make(g, seeds=[1 << 64])


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_list_lengths_must_match(no_engine, which):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=f"^GABatch: 2 {which} for 3 seeds"):
        make(g, seeds=[1, 2, 3], **{which: [(0, 0), (0, 1)]})
    with pytest.raises(ValueError, match=f"^GABatch: 2 {which} for 1 seeds"):
        make(g, seeds=[1], **{which: [(0, 0), (0, 1)]})


@pytest.mark.parametrize("which", ["starts", "targets"])
@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3)])
def test_out_of_range(no_engine, which, cell):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^GABatch: .* is outside the 20x20 grid"):
        make(g, seeds=[1, 2], **{which: [(0, 0), cell]})


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_on_an_obstacle(no_engine, which):
    g, _, _ = gio.grid("fig7")
    r, c = (int(v) for v in np.argwhere(np.asarray(g) == 1)[0])
    with pytest.raises(ValueError, match=rf"^GABatch: {which}\[1\] = \({r}, {c}\) is on an obstacle"):
        make(g, seeds=[1, 2], **{which: [(0, 0), (r, c)]})


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_not_a_pair(no_engine, which):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=rf"^GABatch: {which}\[0\] must be an \(r, c\) pair"):
        make(g, seeds=[1], **{which: [7]})


def test_sizes(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="^GABatch: population_size must be >= 1"):
        make(g, n=0, seeds=[1])
    with pytest.raises(ValueError, match="^GABatch: num_waypoints_per_chromosome must be >= 1"):
        make(g, w=0, seeds=[1])
    with pytest.raises(ValueError, match="^GABatch: num_generations must be >= 0"):
        make(g, generations=-1, seeds=[1])
    with pytest.raises(ValueError, match="^GABatch: grid must be 2-D"):
        make(np.zeros(16, int), seeds=[1])


@pytest.mark.parametrize("marker, what", [(2, "Start"), (3, "Target")])
def test_missing_marker(no_engine, marker, what):
    """starts / targets default to the grid's markers: a grid without one fails in the solo class's words, prefixed."""
    g, _, _ = gio.grid("fig7")
    h = np.array(g)
    h[h == marker] = 0
    with pytest.raises(ValueError, match=f"^GABatch: GA: {what} node not found"):
        make(h, seeds=[1])
    # ... and is fine when every population names its own cells: the check then reaches the device (patched out here)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(h, seeds=[1], starts=[(0, 0)], targets=[(19, 19)])


def test_valid_arguments_reach_the_device(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, seeds=[4, 5], starts=[(0, 0), (19, 19)], targets=[(19, 19), (0, 0)])


def test_header_and_binding_table_name_the_new_entries():
    from pathfit import _lib
    for n in ("pf_decode_batch_multi", "pf_ga_select_batch", "pf_ga_breed_batch", "pf_ga_assemble_batch", "pf_sort_order_by_key_seg",
              "pf_best_rows_seg"):
        assert n in _lib.SYMBOLS and hasattr(_lib.lib(), n)
