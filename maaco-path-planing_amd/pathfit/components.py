"""Components: the connected components of a grid's free cells under a move policy (pf_components) -- which cells can reach each
other at all, how large each region is, and whether a and b are connected, for thousands of pairs on the device
(pf_components_same).  The labels stay in HBM (`labels_device`); `labels` downloads them once.  `refresh` labels again after
`engine.update_grid`."""
import numpy as np

from ._field import Field
from ._lib import PathfitError
from .engine import Engine


class Components(Field):
    """labels[r, c] = -1 on an obstacle, else the rank of the cell's component when the components are ordered by their smallest cell
    id r * C + c (so label 0 holds the first free cell).  Two free cells are adjacent iff the move policy allows the move between
    them; the START and TARGET markers are free cells."""
    _bufs = ("labels_device", "ibuf")

    def __init__(self, grid, allow_diagonal_moves=True, restrict_diagonal_near_obstacle=True, engine=None):
        self._set_grid(grid)
        self.allow_diagonal_moves = bool(allow_diagonal_moves)
        self.restrict_diagonal_near_obstacle = bool(restrict_diagonal_near_obstacle)
        self._set_engine(engine, Engine)                             # every argument is checked: the device
        self.labels_device = self.ibuf = None
        self.labels_device = self.engine.buf(self.rows * self.cols, np.int32)
        self.ibuf = self.engine.buf(4, np.int64)
        self.refresh()

    def refresh(self):
        """Label the map the engine holds now (after engine.update_grid); everything downloaded before is dropped."""
        self._check_open()
        self._labels = self._sizes = self._first = None
        self.engine.components(self.labels_device, self.allow_diagonal_moves, self.restrict_diagonal_near_obstacle, self.ibuf)
        self.kernel_ms = self.engine.last_kernel_ms()
        self.info = self.ibuf.download()
        self.count, self.free_cells = int(self.info[0]), int(self.info[1])
        self.largest = (int(self.info[3]), int(self.info[2]))         # (label, size); (-1, 0) on a map without a free cell
        return self

    def _check_open(self):
        if self.labels_device is None or not getattr(self.engine, "h", None):
            raise PathfitError(f"{type(self).__name__}: the labels are closed")

    @property
    def labels(self):
        """int32 [R, C], downloaded on first use."""
        if self._labels is None:
            self._check_open()
            self._labels = self.labels_device.download().reshape(self.rows, self.cols)
        return self._labels

    def _sizes_and_first(self):
        if self._sizes is None:
            self._check_open()
            if self.count == 0:
                self._sizes, self._first = np.zeros(0, np.int64), np.zeros(0, np.int32)
                return
            e = self.engine
            ds, df = e.buf(self.count, np.int64), e.buf(self.count, np.int32)
            try:
                e.component_sizes(self.labels_device, self.count, ds, df)
                self.sizes_kernel_ms = e.last_kernel_ms()
                self._sizes, self._first = ds.download(), df.download()
            finally:
                ds.free()
                df.free()

    @property
    def sizes(self):
        """int64 [count]: the cells of each component."""
        self._sizes_and_first()
        return self._sizes

    @property
    def first_cells(self):
        """The smallest cell of each component as (r, c) pairs, in label order (strictly increasing cell ids)."""
        self._sizes_and_first()
        return [(int(v) // self.cols, int(v) % self.cols) for v in self._first]

    def label_of(self, cells):
        """int32 per (r, c) pair: the cell's label, -1 on an obstacle."""
        ids = self._cell_ids("cells", cells)
        return self.labels.reshape(-1)[ids].astype(np.int32)

    def mask(self, label):
        """bool [R, C]: the cells of component `label`."""
        return self.labels == self._index("label", label, self.count)

    def same(self, pairs):
        """bool per ((r, c), (r, c)) pair: both cells are free and lie in one component (a free cell is connected to itself; a cell
        beside the grid is connected to nothing).  Computed on the device from the labels in HBM; the map is not downloaded."""
        who = type(self).__name__
        try:
            pairs = list(pairs)
        except TypeError:
            raise ValueError(f"{who}: pairs must be a list of ((r, c), (r, c)) pairs, got {pairs!r}") from None
        for i, p in enumerate(pairs):
            try:
                ok = len(p) == 2
            except TypeError:
                ok = False
            if not ok:
                raise ValueError(f"{who}: pairs[{i}] must be a pair of (r, c) cells, got {p!r}")
        a = self._cell_ids("pairs[.][0]", [p[0] for p in pairs], False)
        b = self._cell_ids("pairs[.][1]", [p[1] for p in pairs], False)
        n = len(pairs)
        if n == 0:
            return np.zeros(0, bool)
        self._check_open()
        e = self.engine
        da, db, ds = e.put(a, np.int32), e.put(b, np.int32), e.buf(n, np.int32)
        try:
            e.components_same(self.labels_device, da, db, n, ds)
            self.same_kernel_ms = e.last_kernel_ms()
            return ds.download() != 0
        finally:
            for buf in (da, db, ds):
                buf.free()
