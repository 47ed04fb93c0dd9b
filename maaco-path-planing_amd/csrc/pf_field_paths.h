// pf_field_paths.h -- routing trees: DijkstraSolver's paths to many targets from one distance field (pf_dist_field_parents,
// pf_dist_field_paths).
//
// Why the paths are dijkstra.py's, cell for cell.  dijkstra.py:59-96 pops heap entries (g, (r, c)) in that order.  Every weight
// is >= 1, so a cell's final label is set by a cell with a strictly smaller label: every cell of label g holds its final label
// before the first cell of label g is popped, and the pop order is the order of (D[v], v), v = r C + c ordering like the tuple.
// came_from[v] is overwritten only on a strict improvement (:84), so the parent that stays is the EARLIEST-popped cell that
// offers the final label:
//     parent(v) = the u with the smallest (D[u], u) among the cells u with a legal move u -> v and fl(D[u] + w) == D[v].
// The rule needs the field alone: no pop order, no heap.
//
// k_dist_field_parent_map_thread_per_cell: one thread per cell, looping over the fields.  A move u -> v and the move v -> u cut the same
// two corners, so legality is symmetric under all four policies and bit opp(k) of mm[v] says whether u = v - step(k) may move
// into v (opposites 0<->1, 2<->3, 4<->7, 5<->6): one mask byte per thread, and a set bit means u lies inside the grid.  The
// fields were written by an earlier kernel on the same stream: plain loads.  Bandwidth-bound (8 B of label and 1 B of mask in,
// 1 B out per cell; the eight neighbour labels come out of L2 / L1, neighbouring threads read neighbouring words); an LDS tile
// with a halo was NOT built -- DESIGN.md 4.12 has the measurement that decided it.
//
// k_dist_field_trace_query_lanes: one lane per query (field, target).  The chain is walked TWICE: first counted, then written.  A
// row is written only once the length is known to fit, so an overflowing query leaves its row untouched, either direction is
// one forward pass of stores (row[len - 1 - i] or row[i]) and there is no compaction pass; the second walk re-reads bytes the
// first one has just pulled into the cache.  A step is one dependent byte load.  The walk is bounded by min(path_cap, RC) cells
// whatever bytes the map holds, and never leaves [0, RC): a corrupt map ends as PF_ST_OVERFLOW.
#pragma once

namespace pf {

#define PF_FP_THREADS 256                       /* parent map: cells per workgroup */
#define PF_FP_TRACE_THREADS 64                  /* trace: queries per workgroup (one wavefront: short chains retire their workgroup) */
#define PF_FP_SOURCE 8                          /* parent code of the source cell */
#define PF_FP_NONE 255                          /* parent code of an obstacle / a cell out of reach */

__global__ __launch_bounds__(PF_FP_THREADS) void k_dist_field_parent_map_thread_per_cell(const uint8_t* __restrict__ mm, int RC, int C, int K,
                                                                                   const double* __restrict__ fields, uint8_t* __restrict__ parents, int* err) {
  const int v = (int)blockIdx.x * PF_FP_THREADS + (int)threadIdx.x;
  if (v >= RC) return;
  const unsigned m = mm[v];
  for (int f = (int)blockIdx.y; f < K; f += (int)gridDim.y) {
    const double* const D = fields + (size_t)f * (size_t)RC;
    const double dv = D[v];
    const unsigned long long vb = __builtin_bit_cast(unsigned long long, dv);
    unsigned code = PF_FP_NONE;
    if (vb == 0ull) code = PF_FP_SOURCE;                             // D == +0.0: the source (unique, the weights being >= 1)
    else if (vb < PF_DF_INF_BITS) {                                  // finite: a parent exists in a fixed-point field
      unsigned long long best = ~0ull;
      int bu = 0x7FFFFFFF;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int opp = k < 4 ? (k ^ 1) : 11 - k;
        if (!((m >> opp) & 1u)) continue;
        const int u = v - (move_dr(k) * C + move_dc(k));
        const double du = D[u];
        if (du + (k < 4 ? 1.0 : PF_SQRT2) != dv) continue;
        const unsigned long long ub = __builtin_bit_cast(unsigned long long, du);   // (non-negative doubles order as their bits)
        if (ub < best || (ub == best && u < bu)) { best = ub; bu = u; code = (unsigned)k; }
      }
      if (code == PF_FP_NONE) *err = 1;                              // (cannot happen for a fixed point; the byte is still written)
    }
    parents[(size_t)f * (size_t)RC + (size_t)v] = (uint8_t)code;
  }
}

// status / length / chosen field per query; a row of d_cells is written only when the status is PF_ST_OK
__global__ __launch_bounds__(PF_FP_TRACE_THREADS) void k_dist_field_trace_query_lanes(const uint8_t* __restrict__ parents, const double* __restrict__ fields, int RC, int C,
                                                                                int K, int n, const int* __restrict__ field_idx, const int* __restrict__ target,
                                                                                int reverse, int path_cap, int* __restrict__ cells, int* __restrict__ len,
                                                                                int* __restrict__ status, int* __restrict__ chosen) {
  const int q = (int)blockIdx.x * PF_FP_TRACE_THREADS + (int)threadIdx.x;
  if (q >= n) return;
  const int t = target[q];
  int f = -1, st = PF_ST_INFEASIBLE, L = 0;
  if (t >= 0 && t < RC) {
    if (field_idx) {
      f = field_idx[q];
      if (f < 0 || f >= K) f = -1;
    } else {                                                         // the nearest source: the first minimum over the fields
      unsigned long long best = ~0ull;
      for (int j = 0; j < K; ++j) {
        const unsigned long long b = __builtin_bit_cast(unsigned long long, fields[(size_t)j * (size_t)RC + (size_t)t]);
        if (b < best) { best = b; f = j; }
      }
    }
  }
  if (f >= 0) {
    const uint8_t* const P = parents + (size_t)f * (size_t)RC;
    unsigned code = P[t];
    if (code != PF_FP_NONE) {
      const int lim = path_cap < RC ? path_cap : RC;                 // a path visits a cell once
      int cell = t, cnt = 1;
      bool ok = true;
      while (code != PF_FP_SOURCE) {                                 // the first walk counts
        if (code > 7u || cnt >= lim) { ok = false; break; }
        cell -= move_dr((int)code) * C + move_dc((int)code);
        if (cell < 0 || cell >= RC) { ok = false; break; }
        code = P[cell];
        cnt += 1;
      }
      if (ok) {                                                      // the second walk writes: every code on it was checked above
        int* const row = cells + (size_t)q * (size_t)path_cap;
        cell = t;
        for (int i = 0; i < cnt; ++i) {
          row[reverse ? i : cnt - 1 - i] = cell;
          if (i + 1 < cnt) { code = P[cell]; cell -= move_dr((int)code) * C + move_dc((int)code); }
        }
        st = PF_ST_OK; L = cnt;
      } else st = PF_ST_OVERFLOW;
    }
  }
  len[q] = L;
  status[q] = st;
  if (chosen) chosen[q] = f;
}

}  // namespace pf
