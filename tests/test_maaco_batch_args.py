"""MAACOBatch argument checks: ValueError before any Engine exists (runs on a CPU-only host)."""
import numpy as np
import pytest

import golden_io as gio

KW = dict(alpha=1.0, beta=7.0, rho=0.1, Q=2.5, a_turn_coef=1.0, wh_max=0.9, wh_min=0.2, k_h_adaptive=0.9, q0_initial=0.5)


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import maaco_batch

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(maaco_batch, "Engine", boom)


def make(g, **kw):
    from pathfit import MAACOBatch
    return MAACOBatch(g, 10, 2, **dict(KW, **kw))


def test_empty_seed_list(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="seeds is empty"):
        make(g, seeds=[])


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_list_lengths_must_match(no_engine, which):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match=f"{which} for 3 seeds"):
        make(g, seeds=[1, 2, 3], **{which: [(0, 0), (0, 1)]})
    with pytest.raises(ValueError, match=f"{which} for 1 seeds"):
        make(g, seeds=[1], **{which: [(0, 0), (0, 1)]})


@pytest.mark.parametrize("which", ["starts", "targets"])
@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3)])
def test_out_of_range(no_engine, which, cell):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="outside the 20x20 grid"):
        make(g, seeds=[1, 2], **{which: [(0, 0), cell]})


@pytest.mark.parametrize("which", ["starts", "targets"])
def test_on_an_obstacle(no_engine, which):
    g, _, _ = gio.grid("fig7")
    r, c = (int(v) for v in np.argwhere(np.asarray(g) == 1)[0])
    with pytest.raises(ValueError, match="on an obstacle"):
        make(g, seeds=[1, 2], **{which: [(0, 0), (r, c)]})


def test_missing_marker_is_maacos_error(no_engine):
    g, _, _ = gio.grid("fig7")
    h = np.array(g)
    h[h == 2] = 0
    with pytest.raises(ValueError, match="MAACO: Start node not found"):
        make(h, seeds=[1])
    make_ok = dict(starts=[(0, 1)])            # an explicit start needs no marker: the checks pass and the Engine is next
    with pytest.raises(AssertionError, match="device was touched"):
        make(h, seeds=[1], **make_ok)


def test_bad_seed_and_ants(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(ValueError, match="seeds must be"):
        make(g, seeds=[-1])
    from pathfit import MAACOBatch
    with pytest.raises(ValueError, match="num_ants"):
        MAACOBatch(g, 0, 2, seeds=[1], **KW)
