"""Engine: one (device, grid) handle of libpathfit.so with numpy-friendly batch calls.

Device buffers are explicit (``DevBuf``) so that populations stay resident in
HBM between calls; the ``*_host`` conveniences stage numpy arrays for the
facades and tests.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import Counters, MaacoParams, MpaParams, PathfitError, ScoreParams

INF = float("inf")
ST_OK, ST_INFEASIBLE, ST_STEP_CAP, ST_OVERFLOW, ST_KEPT = 0, 1, 2, 3, 4


class DevBuf:
    """A typed device allocation owned by an Engine."""

    def __init__(self, eng, shape, dtype):
        self.eng = eng
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        eng._ck(eng.L.pf_dev_alloc(eng.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        a = np.ascontiguousarray(arr, self.dtype)
        assert a.nbytes <= self.nbytes, (a.nbytes, self.nbytes)
        if a.nbytes:
            self.eng._ck(self.eng.L.pf_h2d(self.eng.h, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, count=None):
        out = np.empty(self.shape if count is None else (count,), self.dtype)
        if out.nbytes:
            self.eng._ck(self.eng.L.pf_d2h(self.eng.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def zero(self):
        self.eng._ck(self.eng.L.pf_memset(self.eng.h, self.ptr, 0, self.nbytes))
        return self

    def at(self, elem_offset):
        return self.ptr + int(elem_offset) * self.dtype.itemsize

    def read(self, elem_offset, count):
        """Host copy of `count` elements from `elem_offset` (row reads on demand)."""
        out = np.empty(int(count), self.dtype)
        if out.nbytes:
            self.eng._ck(self.eng.L.pf_d2h(self.eng.h, out.ctypes.data, self.at(elem_offset), out.nbytes))
        return out

    def write(self, elem_offset, arr):
        a = np.ascontiguousarray(arr, self.dtype)
        if a.nbytes:
            self.eng._ck(self.eng.L.pf_h2d(self.eng.h, self.at(elem_offset), a.ctypes.data, a.nbytes))
        return self

    def copy_from(self, elem_offset, src, src_offset, count):
        """Device-to-device copy of `count` elements."""
        self.eng.d2d(self.at(elem_offset), src.at(src_offset), int(count) * self.dtype.itemsize)
        return self

    def free(self):
        if self.ptr and getattr(self.eng, "h", None):   # the handle may already be closed
            self.eng.L.pf_dev_free(self.eng.h, self.ptr)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _View(DevBuf):
    """A DevBuf over memory the library owns (never freed here)."""

    def __init__(self, eng, ptr, count, dtype):
        self.eng, self.ptr = eng, ptr
        self.shape, self.dtype = (int(count),), np.dtype(dtype)
        self.nbytes = int(count) * self.dtype.itemsize

    def free(self):
        self.ptr = 0


def score_params(variant=0, restrict_policy=True, w_turn=0.1, w_safe=0.05, min_safe=1.5, diag_pen=1000.0):
    return ScoreParams(int(variant), int(bool(restrict_policy)), float(w_turn), float(w_safe), float(min_safe),
                       float(diag_pen))


def maaco_out13(out):
    """The 13 doubles one colony's iteration leaves (pf_maaco_iterate / pf_maaco_batch_iterate), by name."""
    return {"ib_len": float(out[0]), "ib_turns": float(out[1]), "ib_idx": int(out[2]), "took": out[3] != 0.0, "best_len": float(out[4]),
            "best_turns": float(out[5]), "skipped": out[8] != 0.0, "overflow_agents": int(out[12])}


class Engine:
    def __init__(self, grid, device=0):
        g = np.ascontiguousarray(np.asarray(grid), dtype=np.int64)
        if g.ndim != 2:
            raise ValueError("grid must be 2-D")
        self.R, self.C = (int(v) for v in g.shape)
        self.grid_u8 = np.ascontiguousarray(np.clip(g, 0, 255).astype(np.uint8))
        self.L = _lib.lib()
        h = C.c_void_p()
        rc = self.L.pf_create(self.grid_u8.ctypes.data, self.R, self.C, int(device), C.byref(h))
        if rc != 0:
            raise PathfitError(self.L.pf_last_error(None).decode())
        self.h = h
        self.device = int(device)
        self._out13 = (C.c_double * 13)()   # pf_maaco_iterate's answer block, reused
        self.klog = None          # a list: every hot-path launch appends (kernel family, its HIP-event ms, its counters)
        self._mpa_owner = None    # weak reference to the solo MPA whose pf_mpa_setup the handle holds (see mpa_setup)

    def update_grid(self, grid):
        """Dynamic maps: replace the occupancy (same shape); solvers built on the old map must be set up again."""
        g = np.ascontiguousarray(np.asarray(grid), dtype=np.int64)
        if g.shape != (self.R, self.C):
            raise ValueError("update_grid: the new grid must have the handle's shape")
        self.grid_u8 = np.ascontiguousarray(np.clip(g, 0, 255).astype(np.uint8))
        self._ck(self.L.pf_update_grid(self.h, self.grid_u8.ctypes.data))

    def close(self):
        if getattr(self, "h", None):
            self.L.pf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise PathfitError(self.L.pf_last_error(self.h).decode())

    def _logk(self, name):
        if self.klog is not None:
            self.klog.append((name, self.last_kernel_ms(), self.counters()))

    def buf(self, shape, dtype):
        return DevBuf(self, shape, dtype)

    def put(self, arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype)
        return DevBuf(self, a.shape if a.ndim else (1,), a.dtype).upload(a)

    def d2d(self, dst_ptr, src_ptr, nbytes):
        if nbytes:
            self._ck(self.L.pf_d2d(self.h, dst_ptr, src_ptr, int(nbytes)))

    def set_option(self, name, value):
        self._ck(self.L.pf_set_option(self.h, name.encode(), int(value)))

    def slot_state(self, slot=0):
        """(solve tag, avoid epoch, settle label epoch) of one search slot (pf_selftest_slot_state; tests of the epoch wraps)."""
        out = (C.c_int64 * 3)()
        self._ck(self.L.pf_selftest_slot_state(self.h, int(slot), out))
        return int(out[0]), int(out[1]), int(out[2])

    def counters(self):
        c = Counters()
        self._ck(self.L.pf_get_counters(self.h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def last_kernel_ms(self):
        return float(self.L.pf_last_kernel_ms(self.h))

    def default_path_cap(self, W=None):
        """Cells per path row when the caller names none: a search's path visits a cell once (at most R * C cells); a decode of W
        waypoints may end each of its W + 1 segments on a visited cell (astar.py:55-56), so it holds up to R * C + W + 1."""
        return min(self.R * self.C + (0 if W is None else int(W) + 1), 8 * (self.R + self.C) + 64)

    # ------------------------------------------------------------------ K2
    def astar_batch(self, variant, d_start, d_target, n, path_cap, d_cells, d_len, d_status, d_avoid_off=None,
                    d_avoid_cells=None, d_counters=None, allow_diag=True, restrict_corner=True):
        self._ck(self.L.pf_astar_batch(self.h, variant, int(allow_diag), int(restrict_corner), n, d_start.ptr,
                                       d_target.ptr, d_avoid_off.ptr if d_avoid_off else None,
                                       d_avoid_cells.ptr if d_avoid_cells else None, path_cap, d_cells.ptr,
                                       d_len.ptr, d_status.ptr, d_counters.ptr if d_counters else None))
        self._logk("astar")

    def astar_host(self, variant, starts, targets, avoid_lists=None, path_cap=None, allow_diag=True,
                   restrict_corner=True, want_counters=False):
        """-> (list of path arrays, status array[, counters n x 4])."""
        n = len(starts)
        cap = int(path_cap or self.default_path_cap())
        ds, dt = self.put(starts, np.int32), self.put(targets, np.int32)
        dc, dl, dst = self.buf((max(n, 1), cap), np.int32), self.buf(max(n, 1), np.int32), self.buf(max(n, 1), np.int32)
        doff = dav = None
        if avoid_lists is not None:
            off = np.zeros(n + 1, np.int64)
            for i, a in enumerate(avoid_lists):
                off[i + 1] = off[i] + (len(a) if a is not None else 0)
            flat = np.concatenate([np.asarray(a, np.int32) for a in avoid_lists if a is not None and len(a)]) \
                if off[-1] else np.zeros(1, np.int32)
            doff, dav = self.put(off, np.int64), self.put(flat, np.int32)
        dcnt = self.buf((max(n, 1), 4), np.int64) if want_counters else None
        self.astar_batch(variant, ds, dt, n, cap, dc, dl, dst, doff, dav, dcnt, allow_diag, restrict_corner)
        cells, lens, st = dc.download(), dl.download(), dst.download()
        paths = [cells[i, :lens[i]].copy() for i in range(n)]
        if want_counters:
            return paths, st[:n], dcnt.download()[:n]
        return paths, st[:n]

    # ------------------------------------------------------------------ distance fields
    def dist_field_batch(self, sources, d_out, allow_diag=True, restrict_corner=True, d_info=None):
        """Exact path lengths from the K cells `sources` (host int32 ids) to every cell -> d_out [K, R * C] doubles in HBM; d_info
        [K, 4] int64 = (levels, cells reached, relaxations offered, list appends) per source."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_dist_field_batch(self.h, int(allow_diag), int(restrict_corner), int(src.size), src.ctypes.data if src.size else None,
                                            d_out.ptr, d_info.ptr if d_info else None))
        self._logk("dist_field")

    def dist_fields_host(self, sources, allow_diag=True, restrict_corner=True, want_info=False):
        """-> float64 [K, R, C] (and int64 [K, 4] when want_info)."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        K = max(int(src.size), 1)
        out = self.buf((K, self.R, self.C), np.float64)
        info = self.buf((K, 4), np.int64) if want_info else None
        try:
            self.dist_field_batch(src, out, allow_diag, restrict_corner, info)
            res = out.download()[:src.size]
            return (res, info.download()[:src.size]) if want_info else res
        finally:
            out.free()
            if info is not None:
                info.free()

    def dist_field_parents(self, K, d_fields, d_parents, allow_diag=True, restrict_corner=True):
        """Parent maps of K fields (d_fields [K, R * C] doubles, the policy they were computed under) -> d_parents [K, R * C] uint8:
        0..7 the move of the tree's last step into the cell, 8 the source, 255 no route (pf_dist_field_parents)."""
        self._ck(self.L.pf_dist_field_parents(self.h, int(allow_diag), int(restrict_corner), int(K), d_fields.ptr if d_fields else None,
                                              d_parents.ptr if d_parents else None))
        self._logk("dist_field_parents")

    def dist_field_paths(self, K, d_parents, d_target, n, path_cap, d_cells, d_len, d_status, d_field_idx=None, d_fields=None,
                         reverse=False, d_chosen=None):
        """n queries (d_field_idx[q], d_target[q]) traced through the parent maps into rows laid out as astar_batch's; d_field_idx
        None: each query takes its nearest source by d_fields; d_chosen int32[n] takes the field used (pf_dist_field_paths)."""
        self._ck(self.L.pf_dist_field_paths(self.h, int(K), d_parents.ptr if d_parents else None, d_fields.ptr if d_fields else None, int(n),
                                            d_field_idx.ptr if d_field_idx else None, d_target.ptr if d_target else None, int(bool(reverse)),
                                            int(path_cap), d_cells.ptr if d_cells else None, d_len.ptr if d_len else None,
                                            d_status.ptr if d_status else None, d_chosen.ptr if d_chosen else None))
        self._logk("dist_field_paths")

    def dist_field_merged(self, set_off, sources, d_out, allow_diag=True, restrict_corner=True, d_info=None):
        """One field per source SET (host int32 CSR: set b = sources[set_off[b]:set_off[b + 1]]) -> d_out [B, R * C] doubles, the
        length from each cell's nearest source of the set; d_info [B, 4] int64 as dist_field_batch's (pf_dist_field_merged)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_dist_field_merged(self.h, int(allow_diag), int(restrict_corner), int(off.size) - 1, off.ctypes.data if off.size else None,
                                             src.ctypes.data if src.size else None, d_out.ptr if d_out else None, d_info.ptr if d_info else None))
        self._logk("dist_field_merged")

    def dist_field_owners(self, set_off, sources, d_parents, d_owner, d_info=None, d_count=None):
        """The parent maps of merged fields (d_parents [B, R * C] uint8) -> d_owner [B, R * C] int32, the index within its set of the
        source at the root of each cell's chain (-1: no route); d_count [len(sources)] int64 the cells each source owns; d_info: the
        field call's block, which bounds the rounds of the pointer doubling (pf_dist_field_owners)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_dist_field_owners(self.h, int(off.size) - 1, d_parents.ptr if d_parents else None, off.ctypes.data if off.size else None,
                                             src.ctypes.data if src.size else None, d_info.ptr if d_info else None, d_owner.ptr if d_owner else None,
                                             d_count.ptr if d_count else None))
        self._logk("dist_field_owners")

    # ------------------------------------------------------------------ any-angle smoothing
    def line_of_sight_batch(self, d_from, d_to, n, d_visible, d_first_block=None, restrict_corner=True):
        """n pairs of cell ids in HBM -> d_visible int32[n] (0 / 1: the segment between the centres meets no obstacle; with
        restrict_corner, touches none in a corner either) and d_first_block int32[n] (the blocking cell nearest d_from, -1 when
        visible), on the occupancy the handle holds now (pf_line_of_sight_batch)."""
        self._ck(self.L.pf_line_of_sight_batch(self.h, int(bool(restrict_corner)), int(n), d_from.ptr if d_from else None, d_to.ptr if d_to else None,
                                               d_visible.ptr if d_visible else None, d_first_block.ptr if d_first_block else None))
        self._logk("line_of_sight")

    def smooth_batch(self, n, path_cap, d_cells, d_len, way_cap, d_way_cells, d_way_len, d_status, d_way_idx=None, d_stats=None,
                     restrict_corner=True):
        """Rows of astar_batch's layout in HBM -> the waypoints forward string pulling keeps: d_way_cells [n, way_cap], d_way_idx (their
        positions in the input row), d_way_len, d_stats [n, 2] = (length, turns), d_status (0 ok, 1 bad row, 3 more waypoints than
        way_cap) (pf_smooth_batch)."""
        self._ck(self.L.pf_smooth_batch(self.h, int(bool(restrict_corner)), int(n), int(path_cap), d_cells.ptr if d_cells else None,
                                        d_len.ptr if d_len else None, int(way_cap), d_way_cells.ptr if d_way_cells else None,
                                        d_way_idx.ptr if d_way_idx else None, d_way_len.ptr if d_way_len else None,
                                        d_stats.ptr if d_stats else None, d_status.ptr if d_status else None))
        self._logk("smooth")

    # ------------------------------------------------------------------ connected components
    def components(self, d_labels, allow_diag=True, restrict_corner=True, d_info=None):
        """The components of the free cells under the move policy, on the map the handle holds now -> d_labels int32 [R * C] in HBM
        (-1 on an obstacle, else the rank of the cell's component by its smallest cell id); d_info int64 [4] = (count, free cells,
        the largest component's size, its label) (pf_components)."""
        self._ck(self.L.pf_components(self.h, int(bool(allow_diag)), int(bool(restrict_corner)), d_labels.ptr if d_labels else None,
                                      d_info.ptr if d_info else None))
        self._logk("components")

    def component_sizes(self, d_labels, count, d_sizes=None, d_first=None):
        """Labels in HBM -> d_sizes int64 [count] (the cells per label) and d_first int32 [count] (the smallest cell id per label);
        labels outside [0, count) are ignored (pf_component_sizes)."""
        self._ck(self.L.pf_component_sizes(self.h, d_labels.ptr if d_labels else None, int(count), d_sizes.ptr if d_sizes else None,
                                           d_first.ptr if d_first else None))
        self._logk("component_sizes")

    def components_same(self, d_labels, d_a, d_b, n, d_same):
        """n pairs of cell ids in HBM -> d_same int32 [n]: 1 where both ids lie inside the grid on free cells of one component, else 0
        (pf_components_same)."""
        self._ck(self.L.pf_components_same(self.h, d_labels.ptr if d_labels else None, int(n), d_a.ptr if d_a else None, d_b.ptr if d_b else None,
                                           d_same.ptr if d_same else None))
        self._logk("components_same")

    def components_phase_ms(self):
        """The spans of the last `components` call made under set_option("components_phases", 1): (init + link, flatten, rank,
        labels, sizes + info) ms."""
        out = (C.c_float * 5)()
        self._ck(self.L.pf_components_phase_ms(self.h, out))
        return tuple(float(v) for v in out)

    # ------------------------------------------------------------------ clearance fields
    def clearance_field(self, d_d2, border=False, d_near=None, d_info=None):
        """The exact squared distance from every cell to the nearest obstacle, on the map the handle holds now -> d_d2 int32 [R * C]
        in HBM (0 on an obstacle, PF_CLEAR_NONE without any; border: the cells just outside the grid count too); d_near int32
        [R * C] the nearest obstacle cell inside the grid (the smallest id on a tie, -1 without any; never the border); d_info int64
        [4] = (obstacle cells, free cells, the largest d2 over the free cells, the smallest cell that attains it)
        (pf_clearance_field)."""
        self._ck(self.L.pf_clearance_field(self.h, int(bool(border)), d_d2.ptr if d_d2 else None, d_near.ptr if d_near else None,
                                           d_info.ptr if d_info else None))
        self._logk("clearance_field")

    def clearance_paths(self, d_d2, n, path_cap, d_cells, d_len, margin_d2, d_out, d_status, d_profile=None):
        """Rows of astar_batch's layout in HBM against a field in HBM -> d_out int32 [n, 4] = (the smallest d2, the first position
        that attains it, the cells with d2 < margin_d2, the first such position or -1), d_profile int32 [n, path_cap] d2 per cell,
        d_status (0 ok, 1 bad row) (pf_clearance_paths)."""
        self._ck(self.L.pf_clearance_paths(self.h, d_d2.ptr if d_d2 else None, int(n), int(path_cap), d_cells.ptr if d_cells else None,
                                           d_len.ptr if d_len else None, int(margin_d2), d_out.ptr if d_out else None,
                                           d_profile.ptr if d_profile else None, d_status.ptr if d_status else None))
        self._logk("clearance_paths")

    def clearance_segments(self, d_d2, d_from, d_to, n, d_min, d_at=None, touched=False):
        """n pairs of cell ids in HBM -> d_min int32 [n], the smallest d2 over the cells the segment between the centres crosses
        (touched: and those it only touches in a corner), and d_at int32 [n], the smallest cell id that attains it; PF_CLEAR_NONE
        and -1 for an endpoint outside the grid (pf_clearance_segments)."""
        self._ck(self.L.pf_clearance_segments(self.h, d_d2.ptr if d_d2 else None, int(bool(touched)), int(n), d_from.ptr if d_from else None,
                                              d_to.ptr if d_to else None, d_min.ptr if d_min else None, d_at.ptr if d_at else None))
        self._logk("clearance_segments")

    def clearance_widest(self, d_d2, set_off, sources, d_out, allow_diag=True, restrict_corner=True, d_info=None):
        """A clearance field in HBM and source SETS (host int32 CSR, as dist_field_merged's) -> d_out int32 [B, R * C]: the largest,
        over the walks from a source of the set to the cell, of the smallest move capacity (min of the two cells' d2, and of the two
        side cells' for a diagonal under restrict_corner), 0 where nothing of capacity >= 1 arrives; d_info int64 [B, 4] = (sources
        that counted, cells with w >= 1, the smallest w >= 1, the smallest cell that attains it) (pf_clearance_widest)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_clearance_widest(self.h, int(bool(allow_diag)), int(bool(restrict_corner)), d_d2.ptr if d_d2 else None, int(off.size) - 1,
                                            off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, d_out.ptr if d_out else None,
                                            d_info.ptr if d_info else None))
        self._logk("clearance_widest")

    def clearance_widest_work(self):
        """(launches, tile visits, words raised, 0) of the last clearance_widest call: they depend on the schedule (the probe's figures)."""
        out = (C.c_int64 * 4)()
        self._ck(self.L.pf_clearance_widest_work(self.h, out))
        return tuple(int(v) for v in out)

    # ------------------------------------------------------------------ cost fields
    def cost_field(self, d_cost, set_off, sources, d_out, allow_diag=True, restrict_corner=True, d_info=None):
        """A cost map in HBM (float64 [R * C], in [1, 2^20] on every free cell) and source SETS (host int32 CSR, as
        dist_field_merged's) -> d_out float64 [B, R * C]: the cost of the cheapest walk into each cell from a source of the set, a
        move weighing the mean of its two cells' costs (times sqrt(2) for a diagonal), inf where none arrives; d_info int64 [B, 4] =
        (sources that counted, cells reached, the cell with the largest finite label, 0) (pf_cost_field)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_cost_field(self.h, int(bool(allow_diag)), int(bool(restrict_corner)), d_cost.ptr if d_cost else None, int(off.size) - 1,
                                      off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, d_out.ptr if d_out else None,
                                      d_info.ptr if d_info else None))
        self._logk("cost_field")

    def cost_field_repair(self, d_cost, changed, set_off, sources, d_rows, allow_diag=True, restrict_corner=True, d_info=None):
        """d_rows float64 [B, R * C]: what cost_field (or an earlier repair) left for the same sets and policy on a map and a cost map
        that differ from the engine's present grid and d_cost at most on the flat cell ids of `changed` (host; duplicates and cells
        that did not change are fine) -> the rows, and d_info, bit for bit as cost_field would write them now: the labels that lost
        their support are raised to inf, then lowered from there (pf_cost_field_repair).  cost_field_work then reports (launches of
        both phases, tile visits of both, words lowered, words raised)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        chg = np.ascontiguousarray(changed, np.int32).reshape(-1)
        self._ck(self.L.pf_cost_field_repair(self.h, int(bool(allow_diag)), int(bool(restrict_corner)), d_cost.ptr if d_cost else None, int(chg.size),
                                             chg.ctypes.data if chg.size else None, int(off.size) - 1, off.ctypes.data if off.size else None,
                                             src.ctypes.data if src.size else None, d_rows.ptr if d_rows else None, d_info.ptr if d_info else None))
        self._logk("cost_field_repair")

    def cost_field_work(self):
        """(launches, tile visits, words lowered, words raised) of the last cost_field or cost_field_repair call (0 words raised after
        cost_field); the first three depend on the schedule (the probe's figures)."""
        out = (C.c_int64 * 4)()
        self._ck(self.L.pf_cost_field_work(self.h, out))
        return tuple(int(v) for v in out)

    def cost_field_parents(self, d_cost, K, d_fields, d_parents, allow_diag=True, restrict_corner=True):
        """Parent maps of K cost fields (the cost map and policy they were computed under) -> d_parents [K, R * C] uint8, coded as
        dist_field_parents' (pf_cost_field_parents); dist_field_paths and dist_field_owners take them unchanged."""
        self._ck(self.L.pf_cost_field_parents(self.h, int(bool(allow_diag)), int(bool(restrict_corner)), d_cost.ptr if d_cost else None, int(K),
                                              d_fields.ptr if d_fields else None, d_parents.ptr if d_parents else None))
        self._logk("cost_field_parents")

    def cost_paths(self, d_cost, n, path_cap, d_cells, d_len, d_total, d_bad):
        """Rows of astar_batch's layout in HBM -> d_total float64 [n], the left-to-right sum of the moves' weights (NaN for a bad
        row), and d_bad int32 [n], the first step that is no king move inside the grid or -1 (pf_cost_paths)."""
        self._ck(self.L.pf_cost_paths(self.h, d_cost.ptr if d_cost else None, int(n), int(path_cap), d_cells.ptr if d_cells else None,
                                      d_len.ptr if d_len else None, d_total.ptr if d_total else None, d_bad.ptr if d_bad else None))
        self._logk("cost_paths")

    # ------------------------------------------------------------------ turn fields
    def turn_field(self, d_cost, turn_weight, set_off, sources, d_states, d_best, allow_diag=True, restrict_corner=True, d_info=None):
        """Source SETS (host int32 CSR, as dist_field_merged's), a cost map in HBM or None (cost 1 everywhere) and a turn weight in
        [0, 2^20] -> d_states float64 [B, 8, R * C]: the cheapest cost of a walk from a source of the set that enters the cell by
        move d, a move weighing as cost_field's plus turn_weight when it differs from the move before; d_best float64 [B, R * C]:
        the smallest of the eight; d_info int64 [B, 4] as cost_field's, counted on d_best (pf_turn_field)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_turn_field(self.h, int(bool(allow_diag)), int(bool(restrict_corner)), d_cost.ptr if d_cost else None, float(turn_weight),
                                      int(off.size) - 1, off.ctypes.data if off.size else None, src.ctypes.data if src.size else None,
                                      d_states.ptr if d_states else None, d_best.ptr if d_best else None, d_info.ptr if d_info else None))
        self._logk("turn_field")

    def turn_field_repair(self, d_cost, turn_weight, changed, set_off, sources, d_states, d_best, allow_diag=True, restrict_corner=True, d_info=None):
        """d_states float64 [B, 8, R * C] and d_best float64 [B, R * C]: what turn_field (or an earlier repair) left for the same sets,
        policy and turn weight on a map and a cost map that differ from the engine's present grid and d_cost (None: ones) at most on
        the flat cell ids of `changed` (host; duplicates and cells that did not change are fine) -> the states, best and d_info, bit
        for bit as turn_field would write them now: the states that lost their support are raised to inf, then lowered from there
        (pf_turn_field_repair).  turn_field_work then reports (launches of both phases, tile visits of both, state words lowered,
        state words raised)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        chg = np.ascontiguousarray(changed, np.int32).reshape(-1)
        self._ck(self.L.pf_turn_field_repair(self.h, int(bool(allow_diag)), int(bool(restrict_corner)), d_cost.ptr if d_cost else None, float(turn_weight),
                                             int(chg.size), chg.ctypes.data if chg.size else None, int(off.size) - 1, off.ctypes.data if off.size else None,
                                             src.ctypes.data if src.size else None, d_states.ptr if d_states else None, d_best.ptr if d_best else None,
                                             d_info.ptr if d_info else None))
        self._logk("turn_field_repair")

    def turn_field_work(self):
        """(launches, tile visits, state words lowered, state words raised) of the last turn_field or turn_field_repair call (0 words
        raised after turn_field); the first three depend on the schedule (the probe's figures)."""
        out = (C.c_int64 * 4)()
        self._ck(self.L.pf_turn_field_work(self.h, out))
        return tuple(int(v) for v in out)

    def turn_field_paths(self, d_cost, turn_weight, B, d_states, d_set_idx, d_target, n, path_cap, d_cells, d_len, d_status, reverse=False):
        """n queries (d_set_idx[q], d_target[q]) chased through the states of turn_field (the same cost map and turn weight) into
        rows laid out as astar_batch's: the route whose cost is d_best at the target (pf_turn_field_paths)."""
        self._ck(self.L.pf_turn_field_paths(self.h, d_cost.ptr if d_cost else None, float(turn_weight), int(B), d_states.ptr if d_states else None, int(n),
                                            d_set_idx.ptr if d_set_idx else None, d_target.ptr if d_target else None, int(bool(reverse)), int(path_cap),
                                            d_cells.ptr if d_cells else None, d_len.ptr if d_len else None, d_status.ptr if d_status else None))
        self._logk("turn_field_paths")

    def turn_paths(self, d_cost, turn_weight, n, path_cap, d_cells, d_len, d_total, d_turns, d_bad):
        """Rows of astar_batch's layout in HBM -> d_total float64 [n], the left-to-right sum of the moves' weights plus turn_weight
        per turn (NaN for a bad row), d_turns int32 [n], the turns, and d_bad int32 [n], the first step that is no king move
        inside the grid or -1 (pf_turn_paths)."""
        self._ck(self.L.pf_turn_paths(self.h, d_cost.ptr if d_cost else None, float(turn_weight), int(n), int(path_cap), d_cells.ptr if d_cells else None,
                                      d_len.ptr if d_len else None, d_total.ptr if d_total else None, d_turns.ptr if d_turns else None,
                                      d_bad.ptr if d_bad else None))
        self._logk("turn_paths")

    # ------------------------------------------------------------------ visibility fields
    def visibility_field(self, viewpoints, d_seen, restrict_corner=True, max_range_sq=-1, d_info=None):
        """What each of the K cells `viewpoints` (host int32 ids) sees, on the map the handle holds now -> d_seen uint8 [K, R * C] in
        HBM (1 where the segment between the centres meets no obstacle; with restrict_corner, touches none in a corner either; and
        dr^2 + dc^2 <= max_range_sq unless that is -1); d_info int64 [K, 4] = (cells seen, the largest dr^2 + dc^2 among them, the
        smallest cell id that attains it, 0), (0, -1, -1, 0) when nothing is seen (pf_visibility_field)."""
        view = np.ascontiguousarray(viewpoints, np.int32).reshape(-1)
        self._ck(self.L.pf_visibility_field(self.h, int(bool(restrict_corner)), int(max_range_sq), int(view.size), view.ctypes.data if view.size else None,
                                            d_seen.ptr if d_seen else None, d_info.ptr if d_info else None))
        self._logk("visibility_field")

    def visibility_count(self, viewpoints, d_count, restrict_corner=True, max_range_sq=-1, d_info=None):
        """-> d_count int32 [R * C] in HBM: how many of the viewpoints see each cell (one listed twice counts twice), without the K
        masks; d_info int64 [4] = (free cells with count > 0, free cells, the largest count over the free cells, the smallest free
        cell id that attains it) (pf_visibility_count)."""
        view = np.ascontiguousarray(viewpoints, np.int32).reshape(-1)
        self._ck(self.L.pf_visibility_count(self.h, int(bool(restrict_corner)), int(max_range_sq), int(view.size), view.ctypes.data if view.size else None,
                                            d_count.ptr if d_count else None, d_info.ptr if d_info else None))
        self._logk("visibility_count")

    def visibility_paths(self, d_count, n, path_cap, d_cells, d_len, d_out, d_status, d_profile=None):
        """Rows of astar_batch's layout in HBM against counts in HBM -> d_out int64 [n, 4] = (the sum of the counts over the row's
        cells, the largest count, the first position that attains it, the cells with count > 0), d_profile int32 [n, path_cap] the
        count per cell, d_status (0 ok, 1 bad row: d_out = (0, -1, -1, 0)) (pf_visibility_paths)."""
        self._ck(self.L.pf_visibility_paths(self.h, d_count.ptr if d_count else None, int(n), int(path_cap), d_cells.ptr if d_cells else None,
                                            d_len.ptr if d_len else None, d_out.ptr if d_out else None, d_profile.ptr if d_profile else None,
                                            d_status.ptr if d_status else None))
        self._logk("visibility_paths")

    # ------------------------------------------------------------------ the sight graph
    def sight_pack(self, nodes, d_adj, ld, restrict_corner=True, max_range_sq=-1, d_info=None):
        """The sight graph over the M cells `nodes` (host int32 ids, strictly increasing), on the map the handle holds now -> d_adj
        uint64 [M, ld] in HBM: bit j & 63 of word j >> 6 of row i is set iff nodes[i] sees nodes[j] (within max_range_sq unless that is
        -1); the diagonal bit says the node's cell is free.  d_info int64 [4] = (set off-diagonal bits, the largest off-diagonal
        degree, the smallest node index that attains it, nodes on obstacles) (pf_sight_pack)."""
        nd = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        self._ck(self.L.pf_sight_pack(self.h, int(bool(restrict_corner)), int(max_range_sq), int(nd.size), nd.ctypes.data if nd.size else None,
                                      d_adj.ptr if d_adj else None, int(ld), d_info.ptr if d_info else None))
        self._logk("sight_pack")

    def sight_field(self, nodes, d_adj, ld, set_off, sources, d_dist, d_parent=None, d_info=None):
        """Exact any-angle labels over a sight graph: one row per source SET of node indices (host int32 CSR as dist_field_merged's;
        a set may be empty) -> d_dist [B, M] doubles, the least left-to-right sum of sqrt(dr^2 + dc^2) over the walks from a usable
        source, +inf where none arrives; d_parent int32 [B, M] (the smallest node index that explains the label, -1 at sources and
        at +inf); d_info int64 [B, 4] = (finite labels, usable sources, the smallest node index with the largest finite label or -1,
        0) (pf_sight_field)."""
        nd = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_sight_field(self.h, int(nd.size), nd.ctypes.data if nd.size else None, d_adj.ptr if d_adj else None, int(ld), int(off.size) - 1,
                                       off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, d_dist.ptr if d_dist else None,
                                       d_parent.ptr if d_parent else None, d_info.ptr if d_info else None))
        self._logk("sight_field")

    def sight_field_work(self):
        """(the most rounds a set took, the rounds of all sets, candidate sums formed, labels lowered) of the last sight_field call."""
        out = (C.c_int64 * 4)()
        self._ck(self.L.pf_sight_field_work(self.h, out))
        return tuple(int(v) for v in out)

    def sight_paths(self, nodes, B, d_dist, d_parent, n, d_target, way_cap, d_way, d_way_len, d_status, d_set=None, d_stats=None, reverse=False):
        """n queries in HBM: the parents chased from node d_target[i] of set d_set[i] (None: set 0) -> d_way int32 [n, way_cap] the
        waypoints' cell ids source -> target (target -> source when reverse), d_way_len, d_stats [n, 2] = (length, turns), d_status
        (0 ok, 1 out of range, 2 infeasible, 3 more waypoints than way_cap, 4 parents that end nowhere) (pf_sight_paths)."""
        nd = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        self._ck(self.L.pf_sight_paths(self.h, int(nd.size), nd.ctypes.data if nd.size else None, int(B), d_dist.ptr if d_dist else None,
                                       d_parent.ptr if d_parent else None, int(n), d_set.ptr if d_set else None, d_target.ptr if d_target else None,
                                       int(bool(reverse)), int(way_cap), d_way.ptr if d_way else None, d_way_len.ptr if d_way_len else None,
                                       d_stats.ptr if d_stats else None, d_status.ptr if d_status else None))
        self._logk("sight_paths")

    # ------------------------------------------------------------------ space-time fields
    def spacetime_stamp(self, horizon, d_occ, n, path_cap, d_cells, d_len, d_status, d_t0=None, after_end=True, corners=False, clear=False):
        """ORs n path rows of astar_batch's layout into the dynamic planes d_occ uint64 [T + 1, R, ceil(C / 64)]: the cell at position
        j of row i at tick d_t0[i] + j (None: 0); after_end: the last cell stays to tick T; corners: a unit diagonal step also stamps
        its two corner cells at both ticks; clear: the planes are zeroed first; d_status 0 ok, 1 a bad row, of which nothing is
        stamped (pf_spacetime_stamp)."""
        self._ck(self.L.pf_spacetime_stamp(self.h, int(horizon), d_occ.ptr if d_occ else None, int(n), int(path_cap), d_cells.ptr if d_cells else None,
                                           d_len.ptr if d_len else None, d_t0.ptr if d_t0 else None, int(bool(after_end)), int(bool(corners)), int(bool(clear)),
                                           d_status.ptr if d_status else None))
        self._logk("spacetime_stamp")

    def spacetime_field(self, horizon, d_occ, set_off, sources, d_arrive, allow_diag=True, restrict_corner=True, d_reach=None, d_info=None):
        """One arrival field per source SET (host int32 CSR as dist_field_merged's) against the planes -> d_arrive int32 [B, R * C]
        (the least tick a robot can be on the cell, -1: never within the horizon), d_reach uint64 [B, T + 1, R * ceil(C / 64)] the
        reach planes, d_info int64 [B, 4] = (cells reached, the largest arrival tick, the smallest cell id that attains it, 0)
        (pf_spacetime_field)."""
        off = np.ascontiguousarray(set_off, np.int32).reshape(-1)
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        self._ck(self.L.pf_spacetime_field(self.h, int(allow_diag), int(restrict_corner), int(horizon), d_occ.ptr if d_occ else None, int(off.size) - 1,
                                           off.ctypes.data if off.size else None, src.ctypes.data if src.size else None, d_arrive.ptr if d_arrive else None,
                                           d_reach.ptr if d_reach else None, d_info.ptr if d_info else None))
        self._logk("spacetime_field")

    def spacetime_paths(self, horizon, d_occ, B, d_reach, n, d_set_idx, d_target, path_cap, d_cells, d_len, d_status, d_tick=None, d_tick_out=None,
                        allow_diag=True, restrict_corner=True):
        """n queries (d_set_idx[q], d_target[q], d_tick[q]: -1 the earliest arrival, -2 the hold tick, >= 0 that tick; None: all -1)
        walked back through the reach planes into rows of tick + 1 cells, cell j the position at tick j; d_tick_out takes the tick
        used (pf_spacetime_paths)."""
        self._ck(self.L.pf_spacetime_paths(self.h, int(allow_diag), int(restrict_corner), int(horizon), d_occ.ptr if d_occ else None, int(B),
                                           d_reach.ptr if d_reach else None, int(n), d_set_idx.ptr if d_set_idx else None, d_target.ptr if d_target else None,
                                           d_tick.ptr if d_tick else None, int(path_cap), d_cells.ptr if d_cells else None, d_len.ptr if d_len else None,
                                           d_status.ptr if d_status else None, d_tick_out.ptr if d_tick_out else None))
        self._logk("spacetime_paths")

    def spacetime_conflicts(self, horizon, d_occ, n, path_cap, d_cells, d_len, d_out, d_status, d_t0=None, hold=False, allow_diag=True,
                            restrict_corner=True):
        """n rows starting at d_t0 (None: 0) against the static map, the planes and the policy -> d_out int32 [n, 4] = (the first
        conflicting tick or -1, its kind 1 static / 2 vertex / 3 swap / 4 corner, the cell entered, the conflicting steps); d_status 0
        ok, 1 a bad row, 2 the row runs past the horizon (pf_spacetime_conflicts)."""
        self._ck(self.L.pf_spacetime_conflicts(self.h, int(allow_diag), int(restrict_corner), int(horizon), d_occ.ptr if d_occ else None, int(n), int(path_cap),
                                               d_cells.ptr if d_cells else None, d_len.ptr if d_len else None, d_t0.ptr if d_t0 else None, int(bool(hold)),
                                               d_out.ptr if d_out else None, d_status.ptr if d_status else None))
        self._logk("spacetime_conflicts")

    # ------------------------------------------------------------------ K1
    # ------------------------------------------------------------------ tours
    def tour_matrix(self, stops, d_fields, d_mat):
        """The stop-to-stop matrix out of n field rows in HBM (d_fields float64 [n, R * C], row i the field from stops[i]; `stops`
        host int32 cell ids) -> d_mat float64 [n, n], d_mat[i, j] = d_fields[i, stops[j]]: a plain gather (pf_tour_matrix)."""
        st = np.ascontiguousarray(stops, np.int32).reshape(-1)
        self._ck(self.L.pf_tour_matrix(self.h, int(st.size), st.ctypes.data if st.size else None, d_fields.ptr if d_fields else None,
                                       d_mat.ptr if d_mat else None))
        self._logk("tour_matrix")

    def tour_solve(self, mode, n, B, d_mat, d_total, d_order, d_status, need=None, d_info=None):
        """B problems d_mat float64 [B, n, n] (entries >= 0 or +inf) that share n, mode (0 open, 1 return, 2 last) and need (host
        uint32 [n]: the nodes that must come before each node, or None) -> d_total float64 [B], the exact optimum; d_order int32
        [B, n], the nodes in visiting order (all -1 where infeasible); d_status int32 [B], 0 or 1 = infeasible; d_info int64 [B, 4] =
        (finite table states, the last middle node or -1, 0, 0) (pf_tour_solve)."""
        nd = None if need is None else np.ascontiguousarray(need, np.uint32).reshape(-1)
        self._ck(self.L.pf_tour_solve(self.h, int(mode), int(n), nd.ctypes.data if nd is not None and nd.size else None, int(B),
                                      d_mat.ptr if d_mat else None, d_total.ptr if d_total else None, d_order.ptr if d_order else None,
                                      d_status.ptr if d_status else None, d_info.ptr if d_info else None))
        self._logk("tour_solve")

    def tour_improve(self, mode, n, B, shared, d_mat, max_moves, d_order, d_value, d_status, d_info=None):
        """B start orders d_order int32 [B, n] (in and out) over one matrix d_mat float64 [n, n] (`shared`) or over [B, n, n], of
        which the upper triangles are read, under mode 0 open, 1 return or 2 last: best-improvement 2-opt, at most max_moves moves
        a start -> d_value float64 [B, 2] = (total after, total before); d_status int32 [B], 0 a local optimum, 1 not searched (a
        +inf weight: the order row is all -1), 2 stopped by the cap; d_info int64 [B, 4] = (moves, sweeps, 0, 0)
        (pf_tour_improve)."""
        self._ck(self.L.pf_tour_improve(self.h, int(mode), int(n), int(B), int(bool(shared)), d_mat.ptr if d_mat else None, int(max_moves),
                                        d_order.ptr if d_order else None, d_value.ptr if d_value else None, d_status.ptr if d_status else None,
                                        d_info.ptr if d_info else None))
        self._logk("tour_improve")

    def fleet_improve(self, mode, k, n, B, shared, d_mat, d_cap, max_moves, d_route, d_len, d_value, d_status, d_info=None):
        """B start rows d_route int32 [B, k + n] (in and out: node 0 first, the robots 0 .. k - 1 in increasing order, the tasks
        behind a robot its route) over one matrix d_mat float64 [k + n, k + n] (`shared`) or over [B, k + n, k + n], of which the
        upper triangles are read, under mode 0 open or 1 return and the capacities d_cap int32 [k] (None: unlimited):
        best-improvement 2-opt and segment relocation, at most max_moves moves a start -> d_len float64 [B, k], each robot's
        length; d_value float64 [B, 3] = (total after, total before, makespan after); d_status int32 [B], 0 no improving move
        is left, 1 not searched (a +inf weight: the row is all -1), 2 stopped by the cap; d_info int64 [B, 4] = (moves, sweeps,
        2-opt moves, relocate moves) (pf_fleet_improve)."""
        self._ck(self.L.pf_fleet_improve(self.h, int(mode), int(k), int(n), int(B), int(bool(shared)), d_mat.ptr if d_mat else None,
                                         d_cap.ptr if d_cap else None, int(max_moves), d_route.ptr if d_route else None, d_len.ptr if d_len else None,
                                         d_value.ptr if d_value else None, d_status.ptr if d_status else None, d_info.ptr if d_info else None))
        self._logk("fleet_improve")

    def fleet_balance(self, mode, k, n, B, shared, d_mat, d_cap, max_moves, d_route, d_len, d_value, d_status, d_info=None):
        """fleet_improve's arguments under the min-max rule: a candidate is priced by the largest length it leaves, the move of a
        sweep is the smallest (span', delta, code, i, j), applied iff it lowers the span or keeps it with a delta < 0 -> d_len
        float64 [B, k]; d_value float64 [B, 4] = (makespan after, total after, makespan before, total before); d_status int32
        [B] as fleet_improve's; d_info int64 [B, 5] = (moves, sweeps, 2-opt moves, relocate moves, moves that lowered the span)
        (pf_fleet_balance)."""
        self._ck(self.L.pf_fleet_balance(self.h, int(mode), int(k), int(n), int(B), int(bool(shared)), d_mat.ptr if d_mat else None,
                                         d_cap.ptr if d_cap else None, int(max_moves), d_route.ptr if d_route else None, d_len.ptr if d_len else None,
                                         d_value.ptr if d_value else None, d_status.ptr if d_status else None, d_info.ptr if d_info else None))
        self._logk("fleet_balance")

    def place_improve(self, mode, m, n, p, fixed, B, shared, d_mat, max_moves, d_sel, d_owner, d_value, d_status, d_info=None):
        """B start rows d_sel int32 [B, p] (in and out: sites of [0, m), -1 an empty slot, no site twice, the slots below `fixed`
        not empty and kept) over one matrix d_mat float64 [m, n] (`shared`) or over [B, m, n] (entries +inf or in [+0.0, 2^1000]),
        under mode 0 sum or 1 max: best-improvement additions and swaps, at most max_moves moves a start -> d_owner int32 [B, n]
        (or None), the open site nearest to each demand or -1; d_value float64 [B, 4] = (sum after, max after, sum before, max
        before); d_status int32 [B], 0 no better candidate is left, 2 stopped by the cap; d_info int64 [B, 4] = (moves, sweeps,
        unserved after, unserved before) (pf_place_improve)."""
        self._ck(self.L.pf_place_improve(self.h, int(mode), int(m), int(n), int(p), int(fixed), int(B), int(bool(shared)), d_mat.ptr if d_mat else None,
                                         int(max_moves), d_sel.ptr if d_sel else None, d_owner.ptr if d_owner else None, d_value.ptr if d_value else None,
                                         d_status.ptr if d_status else None, d_info.ptr if d_info else None))
        self._logk("place_improve")

    def cover_pack(self, kind, K, n, d_src, ld, d_targets, radius, row0, d_mask):
        """K source rows in HBM (d_src uint8 for kind 0, the bit byte != 0: visibility_field's rows; float64 for kind 1, the bit
        x <= radius: the fields' rows), leading dimension ld, read at the n cells d_targets (int32 on the device) -> the rows
        row0 .. row0 + K - 1 of the bit masks d_mask uint64 [m, ceil(n / 64)], 64 targets a word, the tail bits 0 (pf_cover_pack)."""
        self._ck(self.L.pf_cover_pack(self.h, int(kind), int(K), int(n), d_src.ptr if d_src else None, int(ld), d_targets.ptr if d_targets else None,
                                      float(radius), int(row0), d_mask.ptr if d_mask else None))
        self._logk("cover_pack")

    def cover_improve(self, m, n, p, fixed, B, shared, d_mask, max_moves, d_sel, d_covered, d_value, d_status, d_info=None):
        """B start rows d_sel int32 [B, p] (in and out: place_improve's rows) over one mask set d_mask uint64 [m, W] (`shared`) or over
        [B, m, W], W = ceil(n / 64): best-improvement additions, swaps and drops under the key (n - covered, open), at most
        max_moves moves a start -> d_covered uint64 [B, W] (or None), the union; d_value int64 [B, 4] = (covered after, open after,
        covered before, open before); d_status int32 [B], 0 no better candidate is left, 2 stopped by the cap; d_info int64 [B, 4] =
        (moves, sweeps, elements covered exactly once, drops) (pf_cover_improve)."""
        self._ck(self.L.pf_cover_improve(self.h, int(m), int(n), int(p), int(fixed), int(B), int(bool(shared)), d_mask.ptr if d_mask else None, int(max_moves),
                                         d_sel.ptr if d_sel else None, d_covered.ptr if d_covered else None, d_value.ptr if d_value else None,
                                         d_status.ptr if d_status else None, d_info.ptr if d_info else None))
        self._logk("cover_improve")

    # ------------------------------------------------------------------ assignments
    def assign_matrix(self, n_rows, cols, d_fields, d_mat, row0=0, ld=None, transpose=False):
        """A chunk of n_rows field rows in HBM (d_fields float64 [n_rows, R * C]) gathered at the host int32 cell ids `cols` ->
        d_mat[(row0 + i) * ld + j] = d_fields[i, cols[j]], or d_mat[j * ld + row0 + i] with `transpose`; ld defaults to len(cols)
        (pf_assign_matrix)."""
        cl = np.ascontiguousarray(cols, np.int32).reshape(-1)
        self._ck(self.L.pf_assign_matrix(self.h, int(n_rows), int(cl.size), cl.ctypes.data if cl.size else None, d_fields.ptr if d_fields else None,
                                         int(row0), int(cl.size if ld is None else ld), int(bool(transpose)), d_mat.ptr if d_mat else None))
        self._logk("assign_matrix")

    def assign_solve(self, mode, n, m, B, d_mat, d_col, d_value, d_status, d_dual=None, d_info=None):
        """B problems d_mat float64 [B, n, m] (n <= m <= 1024; +inf = no way) under mode 0 sum, 1 max or 2 max_sum -> d_col int32
        [B, n], the column of each row (all -1 where infeasible); d_value float64 [B, 2] = (left-to-right sum, max); d_status int32
        [B], 0 or 1 = infeasible; d_dual float64 [B, n + m] = u then v; d_info int64 [B, 4] = (tree steps of the sum phase, of the
        max phase, the first row that could not be placed or -1, 0) (pf_assign_solve)."""
        self._ck(self.L.pf_assign_solve(self.h, int(mode), int(n), int(m), int(B), d_mat.ptr if d_mat else None, d_col.ptr if d_col else None,
                                        d_value.ptr if d_value else None, d_status.ptr if d_status else None, d_dual.ptr if d_dual else None,
                                        d_info.ptr if d_info else None))
        self._logk("assign_solve")

    def score_batch(self, n, path_cap, d_cells, d_len, d_stats, sp):
        """Rows of astar_batch's layout in HBM -> d_stats [n, 5] doubles (pf_score_batch)."""
        self._ck(self.L.pf_score_batch(self.h, C.byref(sp), int(n), int(path_cap), d_cells.ptr, d_len.ptr, d_stats.ptr))

    def score_host(self, paths, sp):
        n = len(paths)
        cap = max([len(p) for p in paths] + [1])
        cells = np.zeros((n, cap), np.int32)
        lens = np.zeros(n, np.int32)
        for i, p in enumerate(paths):
            cells[i, :len(p)] = p
            lens[i] = len(p)
        dc, dl, ds = self.put(cells), self.put(lens), self.buf((n, 5), np.float64)
        self._ck(self.L.pf_score_batch(self.h, C.byref(sp), n, cap, dc.ptr, dl.ptr, ds.ptr))
        return ds.download()

    # ------------------------------------------------------------------ K3
    def decode_batch(self, n, W, start, target, path_cap, d_cells, d_len, d_status, d_wp_cells=None, d_wp_pos=None,
                     sp=None, d_stats=None, allow_diag=True, restrict_corner=True):
        self._ck(self.L.pf_decode_batch(self.h, int(allow_diag), int(restrict_corner), n, W,
                                        d_wp_cells.ptr if d_wp_cells else None, d_wp_pos.ptr if d_wp_pos else None,
                                        int(start), int(target), path_cap, d_cells.ptr, d_len.ptr, d_status.ptr,
                                        C.byref(sp) if sp is not None else None, d_stats.ptr if d_stats else None))
        self._logk("decode")

    def decode_host(self, start, target, wp_cells=None, wp_pos=None, sp=None, path_cap=None, allow_diag=True,
                    restrict_corner=True):
        """wp_cells int[n, W] or wp_pos float[n, W, 2] -> (paths, status, stats or None).  start / target: one cell each for the
        whole batch, or int[n] arrays with one start and one target per agent (decode_multi)."""
        if wp_cells is not None:
            wp = np.ascontiguousarray(wp_cells, np.int32)
            n, W = wp.shape
            dwc, dwp = self.put(wp.reshape(-1) if wp.size else np.zeros(1, np.int32)), None
        else:
            wp = np.ascontiguousarray(wp_pos, np.float64)
            n, W = wp.shape[0], wp.shape[1]
            dwc, dwp = None, self.put(wp.reshape(-1) if wp.size else np.zeros(1))
        cap = int(path_cap or self.default_path_cap(W))
        m = max(n, 1)
        dc, dl, dst = self.buf((m, cap), np.int32), self.buf(m, np.int32), self.buf(m, np.int32)
        dstat = self.buf((m, 5), np.float64) if sp is not None else None
        if np.ndim(start) or np.ndim(target):
            st_, tg_ = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(target, np.int32)
            if st_.shape != (n,) or tg_.shape != (n,):
                raise ValueError("decode_multi_host: one start and one target per agent")
            ds, dt = self.put(st_ if n else np.zeros(1, np.int32)), self.put(tg_ if n else np.zeros(1, np.int32))
            self.decode_multi(n, W, ds, dt, cap, dc, dl, dst, dwc, dwp, sp, dstat, allow_diag, restrict_corner)
        else:
            self.decode_batch(n, W, start, target, cap, dc, dl, dst, dwc, dwp, sp, dstat, allow_diag, restrict_corner)
        cells, lens, st = dc.download(), dl.download(), dst.download()
        paths = [cells[i, :lens[i]].copy() for i in range(n)]
        return paths, st[:n], (dstat.download()[:n] if dstat is not None else None)

    def decode_multi(self, n, W, d_start, d_target, path_cap, d_cells, d_len, d_status, d_wp_cells=None, d_wp_pos=None,
                     sp=None, d_stats=None, allow_diag=True, restrict_corner=True):
        """decode_batch with a start and a target cell per agent (d_start, d_target: int32[n] buffers)."""
        self._ck(self.L.pf_decode_batch_multi(self.h, int(allow_diag), int(restrict_corner), n, W,
                                              d_wp_cells.ptr if d_wp_cells else None, d_wp_pos.ptr if d_wp_pos else None,
                                              d_start.ptr, d_target.ptr, path_cap, d_cells.ptr, d_len.ptr, d_status.ptr,
                                              C.byref(sp) if sp is not None else None, d_stats.ptr if d_stats else None))
        self._logk("decode")

    def decode_multi_host(self, starts, targets, **kw):
        """decode_host with per-agent endpoints: starts / targets int[n]."""
        return self.decode_host(np.atleast_1d(starts), np.atleast_1d(targets), **kw)

    # ------------------------------------------------------------------ K6
    def pso_update(self, n, W, w, c1, c2, max_vel, d_pos, d_vel, d_pbest, d_gbest, seed, it, agent0=0):
        self._ck(self.L.pf_pso_update(self.h, n, W, w, c1, c2, max_vel, d_pos.ptr, d_vel.ptr, d_pbest.ptr,
                                      d_gbest.ptr, int(seed), int(it), int(agent0)))

    def pso_update_keep_raw(self, n, W, w, c1, c2, max_vel, pos_ptr, vel_ptr, pbest_ptr, gbest_ptr, seed, it, agent0, pos_keep_ptr, vel_keep_ptr):
        """pso_update on raw pointers + the pre-update position / velocity kept for the roll-back; nothing synchronises."""
        self._ck(self.L.pf_pso_update_keep(self.h, n, W, w, c1, c2, max_vel, pos_ptr, vel_ptr, pbest_ptr, gbest_ptr,
                                           int(seed), int(it), int(agent0), pos_keep_ptr, vel_keep_ptr))

    def pso_commit_raw(self, m, W, path_cap, n_final, improver, pos_ptr, vel_ptr, pos_keep_ptr, vel_keep_ptr, stats_ptr, len_ptr, cells_ptr,
                       pbest_ptr, pbf_ptr, pb_cells_ptr, pb_len_ptr, gb_ptr, gstats_ptr, gpath_ptr):
        """One round of the asynchronous sweep committed in one launch (pbest + paths, gbest move, roll-back); nothing synchronises."""
        self._ck(self.L.pf_pso_commit(self.h, int(m), int(W), int(path_cap), int(n_final), int(improver), pos_ptr, vel_ptr, pos_keep_ptr,
                                      vel_keep_ptr, stats_ptr, len_ptr, cells_ptr, pbest_ptr, pbf_ptr, pb_cells_ptr, pb_len_ptr, gb_ptr,
                                      gstats_ptr, gpath_ptr))

    def decode_raw(self, n, W, start, target, path_cap, cells_ptr, len_ptr, status_ptr, wp_pos_ptr, sp, stats_ptr,
                   allow_diag=True, restrict_corner=True):
        self._ck(self.L.pf_decode_batch(self.h, int(allow_diag), int(restrict_corner), n, W, None, wp_pos_ptr,
                                        int(start), int(target), path_cap, cells_ptr, len_ptr, status_ptr,
                                        C.byref(sp), stats_ptr))
        self._logk("decode")

    def pso_scan(self, n, stats_ptr, len_ptr, status_ptr, pbf_ptr, gbest_fit, sync_mode):
        """-> (index of the gbest improver in the batch or -1, its fitness, overflowed particles); one 16-byte D2H."""
        i, f, o = C.c_int32(-1), C.c_double(INF), C.c_int32(0)
        self._ck(self.L.pf_pso_scan(self.h, n, stats_ptr, len_ptr, status_ptr, pbf_ptr, float(gbest_fit), int(sync_mode),
                                    C.byref(i), C.byref(f), C.byref(o)))
        return i.value, f.value, o.value

    def d2h_counts(self):
        """(small copies <= 64 B, bulk copies, bulk bytes) this handle has made device -> host."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.L.pf_d2h_counts(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def span_begin(self):
        """Open a HIP-event timed span on the engine's stream (closed by span_end; not nested, nothing synchronises)."""
        self._ck(self.L.pf_span_begin(self.h))

    def span_end(self):
        self._ck(self.L.pf_span_end(self.h))

    def span_total(self, reset=True):
        """(milliseconds, spans) summed since the last reset; synchronises the stream."""
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        self._ck(self.L.pf_span_total(self.h, C.byref(ms), C.byref(cnt), 1 if reset else 0))
        return ms.value, cnt.value

    def read(self, ptr, count, dtype):
        """A small typed read from device memory (row reads on demand)."""
        out = np.empty(int(count), dtype)
        if out.nbytes:
            self._ck(self.L.pf_d2h(self.h, out.ctypes.data, ptr, out.nbytes))
        return out

    # ------------------------------------------------------------------ K4/K5
    def maaco_setup(self, params):
        self._mp = params
        self._ck(self.L.pf_maaco_setup(self.h, C.byref(params)))

    def maaco_walk(self, it, seed, ant0, n, path_cap, d_cells, d_len, d_plen, d_turns, d_status):
        self._ck(self.L.pf_maaco_walk_batch(self.h, int(it), int(seed), int(ant0), n, path_cap, d_cells.ptr,
                                            d_len.ptr, d_plen.ptr, d_turns.ptr, d_status.ptr))
        self._logk("maaco_walk")

    def maaco_update(self, n, path_cap, d_cells, d_len, d_plen, best_len_overall):
        """MAACO.py:304-332 in one pass over tau (evaporate, ordered deposits, clip): the single-GPU form of the three calls below."""
        self._ck(self.L.pf_maaco_update(self.h, n, path_cap, d_cells.ptr, d_len.ptr, d_plen.ptr, float(best_len_overall)))

    def maaco_iterate(self, it, seed, ant0, n, path_cap, d_cells, d_len, d_plen, d_turns, d_status, best_len, best_turns):
        """One whole iteration (walks, best scan, take-over test, pheromone update) enqueued back to back; one 104-byte block back
        (mirrored by the device into pinned host memory: the call returns once the take-over test is known).
        -> maaco_out13 of it."""
        out = self._out13
        self._ck(self.L.pf_maaco_iterate(self.h, int(it), int(seed), int(ant0), int(n), int(path_cap), d_cells.ptr, d_len.ptr, d_plen.ptr,
                                         d_turns.ptr, d_status.ptr, float(best_len), float(best_turns), C.addressof(out)))
        self._logk("maaco_walk")
        return maaco_out13(out)

    def maaco_best_path(self, cap):
        """The overall best ant's cells as pf_maaco_iterate keeps them in HBM (empty: none yet)."""
        out = np.empty(int(cap), np.int32)
        L = C.c_int32(0)
        self._ck(self.L.pf_maaco_best_path(self.h, out.ctypes.data, int(cap), C.byref(L)))
        return out[:L.value].copy()

    def maaco_evaporate(self):
        self._ck(self.L.pf_maaco_evaporate(self.h))

    def maaco_deposit(self, n, path_cap, d_cells, d_len, d_plen):
        self._ck(self.L.pf_maaco_deposit(self.h, n, path_cap, d_cells.ptr, d_len.ptr, d_plen.ptr))

    def maaco_deposit_begin(self, n, path_cap, d_cells, d_len, d_plen):
        self._ck(self.L.pf_maaco_deposit_begin(self.h, n, path_cap, d_cells.ptr, d_len.ptr, d_plen.ptr))

    def maaco_deposit_cells(self, cell0, cell1):
        self._ck(self.L.pf_maaco_deposit_cells(self.h, int(cell0), int(cell1)))

    def maaco_best_dev(self, n, d_plen, d_turns):
        """MAACO.py:343-349 over device columns -> (best_len, best_turns, best_idx); one 24-byte D2H."""
        out = np.zeros(3)
        self._ck(self.L.pf_maaco_best_dev(self.h, int(n), d_plen.ptr, d_turns.ptr, out.ctypes.data))
        return float(out[0]), float(out[1]), int(out[2])

    @property
    def tau_buf(self):
        """The pheromone matrix in HBM as a buffer object (R*C doubles, owned by the library)."""
        return _View(self, self.L.pf_maaco_tau_dev(self.h), self.R * self.C, np.float64)

    def maaco_clip(self, best_len_overall):
        self._ck(self.L.pf_maaco_clip(self.h, float(best_len_overall)))

    def maaco_get_pheromone(self):
        t = np.empty((self.R, self.C), np.float64)
        self._ck(self.L.pf_maaco_get_pheromone(self.h, t.ctypes.data))
        return t

    def maaco_set_pheromone(self, tau):
        t = np.ascontiguousarray(tau, np.float64)
        assert t.size == self.R * self.C
        self._ck(self.L.pf_maaco_set_pheromone(self.h, t.ctypes.data))

    def maaco_tau_ptr(self):
        return self.L.pf_maaco_tau_dev(self.h)

    def maaco_best_scan(self, plen, turns, idx0, best_len, best_turns, best_idx):
        plen = np.ascontiguousarray(plen, np.float64)
        turns = np.ascontiguousarray(turns, np.int32)
        bl, bt, bi = C.c_double(best_len), C.c_double(best_turns), C.c_int32(best_idx)
        self._ck(self.L.pf_maaco_best_scan(len(plen), plen.ctypes.data, turns.ctypes.data, int(idx0), C.byref(bl),
                                           C.byref(bt), C.byref(bi)))
        return bl.value, bt.value, bi.value

    # ------------------------------------------------------------------ K7
    def mpa_setup(self, mp, sp):
        """The handle holds ONE solo MPA set-up (parameters, memoised initial path, pruning bounds) and one set of look-ahead
        level buffers.  The facade object whose set-up it held (mpa_set_owner) is told first (its _own_views()), while the
        level rows its candidate views point into are still there: the next merged sweep rewrites them and may free them."""
        cur = self.mpa_owner()
        self._mpa_owner = None
        if cur is not None:
            cur._own_views()
        self._ck(self.L.pf_mpa_setup(self.h, C.byref(mp), C.byref(sp)))

    def mpa_set_owner(self, owner):
        """`owner` (an MPA facade) has just called mpa_setup: the set-up is its own until the next mpa_setup."""
        self._mpa_owner = weakref.ref(owner)

    def mpa_owner(self):
        return self._mpa_owner() if self._mpa_owner is not None else None

    def mpa_phase(self, phase, CF, it, seed, n, path_cap, d_pop_cells, d_pop_len, d_pop_stats, d_gidx, d_slot,
                  elite_cells_ptr, elite_len, elite_stats_ptr, d_out_cells, d_out_len, d_out_stats, d_status):
        self._ck(self.L.pf_mpa_phase_batch(self.h, int(phase), float(CF), int(it), int(seed), n, path_cap,
                                           d_pop_cells.ptr, d_pop_len.ptr, d_pop_stats.ptr, d_gidx.ptr, d_slot.ptr,
                                           elite_cells_ptr, int(elite_len), elite_stats_ptr, d_out_cells.ptr,
                                           d_out_len.ptr, d_out_stats.ptr, d_status.ptr))

    def mpa_iter(self, phase, CF, it, seed, n, path_cap, d_pop_cells, d_pop_len, d_pop_stats, d_gidx, d_slot,
                 elite_cells_ptr, elite_len, elite_stats_ptr, d_c1_cells, d_c1_len, d_c1_stats, d_c2_cells, d_c2_len,
                 d_c2_stats, d_status):
        self._ck(self.L.pf_mpa_iter_batch(self.h, int(phase), float(CF), int(it), int(seed), n, path_cap,
                                          d_pop_cells.ptr, d_pop_len.ptr, d_pop_stats.ptr, d_gidx.ptr, d_slot.ptr,
                                          elite_cells_ptr, int(elite_len), elite_stats_ptr, d_c1_cells.ptr,
                                          d_c1_len.ptr, d_c1_stats.ptr, d_c2_cells.ptr, d_c2_len.ptr, d_c2_stats.ptr,
                                          d_status.ptr))
        self._logk("mpa_sweep")

    def mpa_iter_ahead(self, levels, seed, n, path_cap, d_pop_cells, d_pop_len, d_pop_stats, d_gidx, d_slot, elite_cells_ptr,
                       elite_len, elite_stats_ptr, d_c1_cells, d_c1_len, d_c1_stats, d_c2_cells, d_c2_len, d_c2_stats, d_status):
        """mpa_iter for the iterations `levels` = [(phase, CF, it), ...] in one sweep (pf_mpa_iter_ahead): the first is applied,
        the others wait for mpa_ahead_take.  -> predators the first one changed."""
        D = len(levels)
        ph = (C.c_int32 * D)(*[int(l[0]) for l in levels])
        cf = (C.c_double * D)(*[float(l[1]) for l in levels])
        its = (C.c_int32 * D)(*[int(l[2]) for l in levels])
        acc = C.c_int32(0)
        self._ck(self.L.pf_mpa_iter_ahead(self.h, D, C.addressof(ph), C.addressof(cf), C.addressof(its), int(seed), n, path_cap,
                                          d_pop_cells.ptr, d_pop_len.ptr, d_pop_stats.ptr, d_gidx.ptr, d_slot.ptr,
                                          elite_cells_ptr, int(elite_len), elite_stats_ptr, d_c1_cells.ptr, d_c1_len.ptr,
                                          d_c1_stats.ptr, d_c2_cells.ptr, d_c2_len.ptr, d_c2_stats.ptr, d_status.ptr, C.byref(acc)))
        self._logk("mpa_sweep")
        return acc.value

    def mpa_ahead_take(self, it, d_slot, d_pop_cells, d_pop_len, d_pop_stats):
        """Iteration `it` from a level of the last merged sweep -> predators changed, or -1 when the level is not (or no longer)
        that iteration's.  No search runs, so nothing is logged."""
        acc = C.c_int32(-1)
        self._ck(self.L.pf_mpa_ahead_take(self.h, int(it), d_slot.ptr, d_pop_cells.ptr, d_pop_len.ptr, d_pop_stats.ptr, C.byref(acc)))
        return acc.value

    def mpa_ahead_level_bufs(self, n, path_cap):
        """Views of the candidate rows of the level applied last (c1 cells / len / stats, c2 cells / len / stats, status), or None
        after a single-level sweep."""
        out = (C.c_void_p * 7)()
        self._ck(self.L.pf_mpa_ahead_level_bufs(self.h, C.addressof(out)))
        if not out[0]:
            return None
        shapes = [((n, path_cap), np.int32), ((n,), np.int32), ((n, 5), np.float64)] * 2 + [((n,), np.int32)]
        views = []
        for p, (shape, dt) in zip(out, shapes):
            v = _View(self, p, int(np.prod(shape)), dt)
            v.shape = shape
            views.append(v)
        return views

    def mpa_ahead_drop(self):
        self._ck(self.L.pf_mpa_ahead_drop(self.h))

    def mpa_ahead_stats(self):
        out = (C.c_int64 * 6)()
        self._ck(self.L.pf_mpa_ahead_stats(self.h, C.addressof(out)))
        return dict(zip(("cap", "always", "merged_sweeps", "levels_ahead", "served", "stale"), (int(v) for v in out)))

    # ------------------------------------------------------------------ GA generation in HBM
    def ga_select(self, seed, gen, n, k, d_fit_all, d_gorder, d_psid):
        self._ck(self.L.pf_ga_select_dev(self.h, int(seed), int(gen), int(n), int(k), d_fit_all.ptr, d_gorder.ptr, d_psid.ptr))

    def ga_breed(self, seed, gen, N, W, cx, mut, d_chrom_all, d_psid, child0, nchild, d_out):
        self._ck(self.L.pf_ga_breed_dev(self.h, int(seed), int(gen), int(N), int(W), float(cx), float(mut), d_chrom_all.ptr, d_psid.ptr,
                                        int(child0), int(nchild), d_out.ptr))

    def ga_assemble(self, n_loc, W, cap, lo, kid_len, kid_chrom, kid_stats, kid_cells, psid, chrom_old, stats_old, cells_old, len_old,
                    old_lo, old_hi, chrom_new, stats_new, cells_new, len_new):
        self._ck(self.L.pf_ga_assemble_dev(self.h, int(n_loc), int(W), int(cap), int(lo), kid_len.ptr, kid_chrom.ptr, kid_stats.ptr,
                                           kid_cells.ptr, psid.ptr, chrom_old.ptr, stats_old.ptr, cells_old.ptr, len_old.ptr,
                                           int(old_lo), int(old_hi), chrom_new.ptr, stats_new.ptr, cells_new.ptr, len_new.ptr))

    # ------------------------------------------------------------------ K GA populations in one generation (GABatch)
    def ga_select_batch(self, d_seeds, gen, K, N, k, d_fit_all, d_gorder, d_psid):
        self._ck(self.L.pf_ga_select_batch(self.h, d_seeds.ptr, int(gen), int(K), int(N), int(k), d_fit_all.ptr, d_gorder.ptr, d_psid.ptr))

    def ga_breed_batch(self, d_seeds, gen, K, N, W, cx, mut, d_chrom_all, d_psid, d_out):
        self._ck(self.L.pf_ga_breed_batch(self.h, d_seeds.ptr, int(gen), int(K), int(N), int(W), float(cx), float(mut), d_chrom_all.ptr,
                                          d_psid.ptr, d_out.ptr))

    def ga_assemble_batch(self, K, N, W, cap, kid_len, kid_chrom, kid_stats, kid_cells, psid, chrom_old, stats_old, cells_old, len_old,
                          chrom_new, stats_new, cells_new, len_new):
        self._ck(self.L.pf_ga_assemble_batch(self.h, int(K), int(N), int(W), int(cap), kid_len.ptr, kid_chrom.ptr, kid_stats.ptr,
                                             kid_cells.ptr, psid.ptr, chrom_old.ptr, stats_old.ptr, cells_old.ptr, len_old.ptr,
                                             chrom_new.ptr, stats_new.ptr, cells_new.ptr, len_new.ptr))

    # ------------------------------------------------------------------ K PSO swarms in one batched sweep (pathfit.PSOBatch)
    def pso_update_batch(self, n, K, N, W, w, c1, c2, max_vel, it, d_seeds, d_tab, d_starts, d_targets, d_pos, d_vel, d_pbest, d_gbest,
                         s_pos, s_vel, s_start, s_target, s_row):
        self._ck(self.L.pf_pso_update_batch(self.h, int(n), int(K), int(N), int(W), w, c1, c2, max_vel, int(it), d_seeds.ptr, d_tab.ptr,
                                            d_starts.ptr, d_targets.ptr, d_pos.ptr, d_vel.ptr, d_pbest.ptr, d_gbest.ptr, s_pos.ptr, s_vel.ptr,
                                            s_start.ptr, s_target.ptr, s_row.ptr))

    def pso_scan_batch(self, K, N, sync_mode, d_tab, s_stats, s_len, s_status, d_pbf, d_gfit, d_rec, out):
        """-> out, a structured array [K] of (idx, ovf, fit): every swarm's improver of the round; ONE copy of 16 K bytes."""
        self._ck(self.L.pf_pso_scan_batch(self.h, int(K), int(N), int(sync_mode), d_tab.ptr, s_stats.ptr, s_len.ptr, s_status.ptr, d_pbf.ptr,
                                          d_gfit.ptr, d_rec.ptr, out.ctypes.data))
        return out

    def pso_commit_batch(self, n, K, N, W, cap, sync_mode, d_tab, d_rec, s_row, s_pos, s_vel, s_stats, s_len, s_cells, d_pos, d_vel, d_stats,
                         d_len, d_cells, d_pbest, d_pbf, d_pb_cells, d_pb_len, d_gbest, d_gstats, d_gpath, d_gfit):
        self._ck(self.L.pf_pso_commit_batch(self.h, int(n), int(K), int(N), int(W), int(cap), int(sync_mode), d_tab.ptr, d_rec.ptr, s_row.ptr,
                                            s_pos.ptr, s_vel.ptr, s_stats.ptr, s_len.ptr, s_cells.ptr, d_pos.ptr, d_vel.ptr, d_stats.ptr,
                                            d_len.ptr, d_cells.ptr, d_pbest.ptr, d_pbf.ptr, d_pb_cells.ptr, d_pb_len.ptr, d_gbest.ptr,
                                            d_gstats.ptr, d_gpath.ptr, d_gfit.ptr))

    def sort_order_by_key_seg(self, K, n, d_vals, stride, offset, d_order):
        """K stable sorts of n keys each: segment k of d_order (position -> local id) by d_vals[(k n + id) * stride + offset]."""
        self._ck(self.L.pf_sort_order_by_key_seg(self.h, int(K), int(n), d_vals.ptr, int(stride), int(offset), d_order.ptr))

    def best_rows_seg(self, K, N, d_stats, d_order, out):
        """out [K][6] = (local id at the head of segment k, its five stats): one copy."""
        self._ck(self.L.pf_best_rows_seg(self.h, int(K), int(N), d_stats.ptr, d_order.ptr, out.ctypes.data))
        return out

    def sort_order_by_key(self, n, d_vals, stride, offset, d_order):
        self._ck(self.L.pf_sort_order_by_key(self.h, int(n), d_vals.ptr, int(stride), int(offset), d_order.ptr))

    def sorted_head(self, d_order, d_vals, stride=1, offset=0):
        """(id at the head of the sorted list, its key): one 16-byte copy."""
        out = np.zeros(2)
        self._ck(self.L.pf_sorted_head(self.h, d_order.ptr, d_vals.ptr, int(stride), int(offset), out.ctypes.data))
        return int(out[0]), float(out[1])

    def vec_add(self, n, d_a, d_b, sign, d_out):
        """d_out = d_a + sign * d_b (sign +1 / -1) on device columns."""
        self._ck(self.L.pf_vec_add_f64(self.h, int(n), d_a.ptr, d_b.ptr, float(sign), d_out.ptr))

    def gather_col(self, n, d_src, stride, offset, d_dst):
        self._ck(self.L.pf_gather_col(self.h, int(n), d_src.ptr, int(stride), int(offset), d_dst.ptr))

    def mpa_elite_bufs(self):
        """(cells, len, stats) views of the library's elite buffer."""
        c, l, s_ = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._ck(self.L.pf_mpa_elite_buf(self.h, C.byref(c), C.byref(l), C.byref(s_)))
        return (_View(self, c.value, self.R * self.C, np.int32), _View(self, l.value, 1, np.int32), _View(self, s_.value, 5, np.float64))

    def mpa_pick_elite(self, path_cap, d_pop_cells, d_pop_len, d_pop_stats, d_order, first_id=0):
        self._ck(self.L.pf_mpa_pick_elite(self.h, int(path_cap), d_pop_cells.ptr, d_pop_len.ptr, d_pop_stats.ptr, d_order.ptr, int(first_id)))

    def mpa_local_view(self, N, d_gorder, lo, hi, d_gidx, d_slot):
        self._ck(self.L.pf_mpa_local_view(self.h, int(N), d_gorder.ptr, int(lo), int(hi), d_gidx.ptr, d_slot.ptr))

    def mpa_fads(self, CF, it, seed, n, path_cap, d_gidx, d_slot, d_pop_cells, d_pop_len, d_pop_stats, d_status):
        self._ck(self.L.pf_mpa_fads_batch(self.h, float(CF), int(it), int(seed), n, path_cap, d_gidx.ptr, d_slot.ptr,
                                          d_pop_cells.ptr, d_pop_len.ptr, d_pop_stats.ptr, d_status.ptr))

    def mpa_memory(self, n, path_cap, d_slot, d_cand_cells, d_cand_len, d_cand_stats, d_pop_cells, d_pop_len,
                   d_pop_stats):
        self._ck(self.L.pf_mpa_memory(self.h, n, path_cap, d_slot.ptr, d_cand_cells.ptr, d_cand_len.ptr,
                                      d_cand_stats.ptr, d_pop_cells.ptr, d_pop_len.ptr, d_pop_stats.ptr))
