"""Components argument checks: ValueError before any device is touched (runs on a CPU-only host)."""
import numpy as np
import pytest

import component_checkers as cc
import golden_io as gio


@pytest.fixture
def no_engine(monkeypatch):
    from pathfit import components

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(components, "Engine", boom)


class HostBuf:
    def __init__(self, n, dtype):
        self.a = np.zeros(n, dtype)

    def download(self):
        return self.a.copy()

    def free(self):
        pass


class ModelEngine:
    """An engine of the grid's shape whose `components` is the model; every later device call fails the test when `sealed`."""
    h = 1

    def __init__(self, g):
        self.g, (self.R, self.C) = g, g.shape
        self.sealed, self.calls = False, 0

    def buf(self, n, dtype):
        assert not self.sealed, "the device was touched before the arguments were checked (buf)"
        return HostBuf(n, dtype)

    def components(self, d_labels, ad, rs, d_info):
        assert not self.sealed, "the device was touched before the arguments were checked (components)"
        lab, sizes, _ = cc.flood_fill(self.g, ad, rs)
        d_labels.a[:] = lab.reshape(-1)
        d_info.a[:] = cc.info_of(sizes)
        self.calls += 1

    def last_kernel_ms(self):
        return 0.0

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched before the arguments were checked ({name})")


def make(g, **kw):
    from pathfit import Components
    return Components(g, **kw)


def test_grid_must_be_2d(no_engine):
    with pytest.raises(ValueError, match="^Components: grid must be 2-D"):
        make(np.zeros(16, int))
    with pytest.raises(ValueError, match="^Components: grid must be 2-D"):
        make(np.zeros((2, 2, 2), int))


def test_engine_of_another_shape(no_engine):
    g, _, _ = gio.grid("fig7")

    class Other:
        R, C = 20, 21
    with pytest.raises(ValueError, match="^Components: the engine's grid has another shape"):
        make(g, engine=Other())


def test_valid_arguments_reach_the_device(no_engine):
    g, _, _ = gio.grid("fig7")
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g)
    with pytest.raises(AssertionError, match="the device was touched"):
        make(g, allow_diagonal_moves=False, restrict_diagonal_near_obstacle=False)


@pytest.fixture
def img1(no_engine):
    g, _, _ = gio.grid("img1")
    e = ModelEngine(g)
    comp = make(g, engine=e)
    assert comp.count == 2 and comp.largest == (0, 281) and comp.free_cells == 298 and e.calls == 1
    e.sealed = True
    return comp


@pytest.mark.parametrize("cell", [(-1, 0), (0, 20), (20, 3)])
def test_label_of_outside_the_grid(img1, cell):
    with pytest.raises(ValueError, match=r"^Components: cells\[1\] = .* is outside the 20x20 grid"):
        img1.label_of([(0, 0), cell])


@pytest.mark.parametrize("bad", [[7], [(1, 2, 3)], ["ab", (0, 0)], [None]])
def test_label_of_not_a_pair(img1, bad):
    with pytest.raises(ValueError, match=r"^Components: cells\[0\] must be an \(r, c\) pair"):
        img1.label_of(bad)


def test_label_of_needs_a_list(img1):
    with pytest.raises(ValueError, match="^Components: cells must be a list"):
        img1.label_of(5)


@pytest.mark.parametrize("label", [-1, 2, 1.5, "a", None, True])
def test_mask_label_outside_the_count(img1, label):
    with pytest.raises(ValueError, match=r"^Components: label = .* is outside \[0, 2\)"):
        img1.mask(label)


@pytest.mark.parametrize("bad", [[((0, 0),)], [5], [((0, 0), (1, 1), (2, 2))]])
def test_same_needs_pairs_of_cells(img1, bad):
    with pytest.raises(ValueError, match=r"^Components: pairs\[0\] must be a pair of \(r, c\) cells"):
        img1.same(bad)
    with pytest.raises(ValueError, match=r"^Components: pairs\[.\]\[0\]\[0\] must be an \(r, c\) pair"):
        img1.same([(7, (0, 0))])


def test_checked_calls_reach_the_device(img1):
    with pytest.raises(AssertionError, match="the device was touched"):
        img1.same([((0, 0), (3, 4))])
    with pytest.raises(AssertionError, match="the device was touched"):
        img1.same([((0, 0), (3, 40))])                              # a cell beside the grid is an answer (False), no error
    assert len(img1.same([])) == 0
    with pytest.raises(AssertionError, match="the device was touched"):
        img1.sizes
    lab = cc.flood_fill(img1.grid, 1, 1)[0]
    assert np.array_equal(img1.labels, lab) and np.array_equal(img1.mask(1), lab == 1)    # the model engine's host buffer
    assert np.array_equal(img1.label_of([(0, 0), (19, 19)]), lab[[0, 19], [0, 19]])
