"""What the field classes share (DistanceField, NearestSourceField, CostField, TurnField, PathSmoother, Components, Clearance,
Visibility, SpaceTime, and through Planner the six planners Tour, Assignment, TourSearch, FleetTours, Placement, Coverage): the
constructor's grid and engine checks, the (r, c) -> cell id parser with its two messages, the index check and the close / __del__
pair.  Every message starts with the class name; all checks run before the device is touched.  What only the planners share -- the
device state around their fields, the chunk loop, the route tracer, refresh, the restart driver and the checks of their
solve_matrices -- is _planner.py's."""
import numpy as np


class Field:
    _bufs = ()                              # the attributes that hold device buffers: close() frees them

    def _set_grid(self, grid):
        self.grid = np.array(grid, dtype=int)
        if self.grid.ndim != 2:
            raise ValueError(f"{type(self).__name__}: grid must be 2-D")
        self.rows, self.cols = self.grid.shape

    def _set_engine(self, engine, new_engine):
        """The last check, then the device: `engine`, or new_engine(grid) for one of the object's own, which close() closes."""
        if engine is not None and (engine.R, engine.C) != self.grid.shape:
            raise ValueError(f"{type(self).__name__}: the engine's grid has another shape")
        self._own_engine = engine is None
        self.engine = engine if engine is not None else new_engine(self.grid)

    def _cell(self, what, p, inside=True):
        """(r, c) -> the cell id r * cols + c; a pair beside the grid is an error when `inside`, else the id -1."""
        who = type(self).__name__
        try:
            r, c = (int(v) for v in p)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {what} must be an (r, c) pair, got {p!r}") from None
        if not (0 <= r < self.rows and 0 <= c < self.cols):
            if not inside:
                return -1
            raise ValueError(f"{who}: {what} = {(r, c)} is outside the {self.rows}x{self.cols} grid")
        return r * self.cols + c

    def _cell_ids(self, what, cells, inside=True):
        """A list of (r, c) pairs -> int32 cell ids."""
        try:
            cells = list(cells)
        except TypeError:
            raise ValueError(f"{type(self).__name__}: {what} must be a list of (r, c) pairs, got {cells!r}") from None
        return np.array([self._cell(f"{what}[{i}]", p, inside) for i, p in enumerate(cells)], np.int32).reshape(len(cells))

    def _index(self, name, v, n):
        """v as an int in [0, n)."""
        try:
            ok = int(v) == v and not isinstance(v, bool) and 0 <= int(v) < n
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{type(self).__name__}: {name} = {v!r} is outside [0, {n})")
        return int(v)

    def close(self):
        for name in self._bufs:
            buf = getattr(self, name, None)
            setattr(self, name, None)
            if buf is not None:
                buf.free()
        if getattr(self, "_own_engine", False) and getattr(self, "engine", None) is not None:
            self.engine.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
