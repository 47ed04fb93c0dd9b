// pf_widest.h -- widest-path fields over a clearance field: w[b][v] = the largest, over all walks from a source of set b to v, of
// the smallest move capacity on the walk (pf_clearance_widest).  Everything is int32 and exact.
//
// The rule.  The capacity of a move u -> v is min(d2[u], d2[v]); a diagonal move under restrict_corner also takes the two side
// cells' d2 into the minimum, and does not exist without allow_diag.  w[b][s] = d2[s] on a source s with d2[s] >= 1, and w is the
// least fixed point of  w[v] = max(w[v], min(w[u], cap(u, v)))  above those seeds; 0 where no source reaches with capacity >= 1
// (every cell with d2 == 0 among them).  w[u] <= d2[u] holds from the seeds on, so min(w[u], cap(u, v)) is min(w[u], d2[v]) for a
// straight move and min(w[u], d2[v], side, side) for a restricted diagonal: a cell keeps d2[v] and four side minima in registers
// and a sweep reads nothing but the eight neighbours' w.  Equivalently, for every t >= 1: w[b][v] >= t iff v and a source of set
// b lie in one component of the map whose obstacles are the cells with d2 < t.  d2 is read only; the occupancy never is.
//
//   k_widest_seed_sets              one thread per listed source (tq_seed_sets): an atomic exchange of d2[s] into w[b][s] (the first one
//                                   to find 0 there counts the source: a source listed twice counts once, one with d2 == 0 never),
//                                   and the source's tile goes on the first queue.
//   k_widest_relax_tiles_in_lds     one workgroup per queued (set, tile), a tile being PF_WD_TW x PF_WD_TH cells, four per thread:
//                                   loads its cells and a one-cell halo of w and d2 into LDS (0 beyond the grid: such a cell offers
//                                   and takes nothing), sweeps until one whole sweep raises nothing -- the tile's own fixed point
//                                   under the halo it read; a sweep relaxes a cell from its eight neighbours and then carries w
//                                   along the tile row by a wave-wide (max, min) scan (wd_row_scan; -DPF_WD_ROW_SCAN=0: without) --,
//                                   stores the words that rose and queues, for the next launch, the neighbour tiles that hold a
//                                   risen cell in their halo.  Opening and closing the visit, the queues, flags and parity are
//                                   pf_tile_queue.h's.
//   k_widest_info_sum / k_widest_write_info   the cells with w >= 1 and the smallest such w with the smallest cell id that
//                                   attains it, as one 64-bit atomic min of (w << 32) | id per set; then the four words of `info`.
//
// Rounds and cost.  One launch per round over the queued tiles of all B sets; the host reads the next queue's length (4 bytes) after
// each and stops at 0.  After round k every cell whose widest walk crosses tile borders at most k - 1 times holds its final value
// (induction over the crossings: the tile before the last crossing was final a round earlier and queued this one), so the rounds
// are at most 1 + the largest number of tile-border crossings a widest walk needs: they grow with the TILES a widest route
// crosses, not with its cells -- a corridor that winds inside one tile costs sweeps in LDS, not launches.  A simple walk crosses
// fewer than R C borders, which is the bound the host enforces.  A tile may be visited again whenever a wider route reaches its
// halo later than a narrower one; pf_clearance_widest_work reports launches, tile visits and words raised.
//
// Why this is exact.  Values only rise: every value ever stored in w[v] is the capacity of some real walk from a source to v, so a
// halo word read old (the neighbour tile may be raising it in the same launch) is a valid lower bound, and a tile relaxed from old
// halo words ends at or below the least fixed point, never above it.  w[v] is an aligned 32-bit word with one writer per launch,
// and whoever raises a border cell queues its readers for the next launch (pf_tile_queue.h has this half of the argument, and
// which accesses are agent-scope atomics: here wd_load, wd_store and the seed's exchange): at the end the whole array is a fixed
// point above the seeds, at or below the least one by the first half and at or above it because it is a fixed point above the
// seeds.  The least fixed point is unique, so the result does not depend on timing and is identical run to run.
#pragma once

namespace pf {

#ifndef PF_WD_ROW_SCAN
#define PF_WD_ROW_SCAN 1                        /* 1: a sweep also carries w along each tile row by a wave-wide (max, min) scan; 0: neighbour sweeps alone */
#endif
#define PF_WD_THREADS 256
#define PF_WD_TW 64                             /* the tile: 64 x 16 cells, four per thread; a wavefront holds one tile row */
#define PF_WD_TH 16
#define PF_WD_LW (PF_WD_TW + 2)                 /* the tile and its halo in LDS */
#define PF_WD_LH (PF_WD_TH + 2)

__device__ __forceinline__ int wd_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void wd_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(PF_WD_THREADS) void k_widest_seed_sets(const int* __restrict__ d2, int RC, int C, int tiles_x, int ntiles, int B,
                                                                          const int* __restrict__ off, const int* __restrict__ src, int* __restrict__ w_rows,
                                                                          int* __restrict__ flag, int* __restrict__ queue, int* __restrict__ count,
                                                                          unsigned long long* __restrict__ nsrc) {
  tq_seed_sets<PF_WD_THREADS, PF_WD_TW, PF_WD_TH>(RC, C, tiles_x, ntiles, B, off, src, flag, queue, count, nsrc, [&](int b, int s) {
    const int dv = d2[s];
    return dv >= 1 && __hip_atomic_exchange(w_rows + (size_t)b * (size_t)RC + (size_t)s, dv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;   // != 0: listed twice
  });
}

// The 64 cells of a tile row lie in the 64 lanes of one wavefront.  Straight moves along the row alone carry w[j] to cell i at
// min(w[j], the smallest d2 strictly after j up to i) (w[j] <= d2[j]), a (max, min) scan: the pair (value at the segment's far end,
// smallest d2 of the segment) composes associatively, so six shuffle steps each way do what 63 sweeps would.  Every value it
// produces is the capacity of a real walk, so the fixed point is the same; a corridor along a row costs one sweep, not 64.
__device__ __forceinline__ int wd_row_scan(int w, int d, int lane) {
  int rw = w, rm = d, lw_ = w, lm = d;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const int ow = __shfl_up(rw, k), om = __shfl_up(rm, k);          // the segment that ends k lanes to the left
    if (lane >= k) { const int t = ow < rm ? ow : rm; rw = t > rw ? t : rw; rm = om < rm ? om : rm; }
    const int pw = __shfl_down(lw_, k), pm = __shfl_down(lm, k);     // ... that begins k lanes to the right
    if (lane + k < 64) { const int t = pw < lm ? pw : lm; lw_ = t > lw_ ? t : lw_; lm = pm < lm ? pm : lm; }
  }
  return rw > lw_ ? rw : lw_;
}

__global__ __launch_bounds__(PF_WD_THREADS) void k_widest_relax_tiles_in_lds(const int* __restrict__ d2, int R, int C, int allow_diag, int restrict_corner, int tiles_x,
                                                                            int tiles_y, int* w_rows, const int* __restrict__ queue, int nqueue, int first, int* flag_now, int* count_now,
                                                                            int* flag_next, int* __restrict__ queue_next, int* count_next,
                                                                            unsigned long long* __restrict__ raised_total) {
  constexpr int PER = PF_WD_TW * PF_WD_TH / PF_WD_THREADS, LW = PF_WD_LW, LN = PF_WD_LW * PF_WD_LH;
  __shared__ int lw[LN];
  __shared__ int ld[LN];
  if ((int)blockIdx.x >= nqueue) return;
  const int tid = (int)threadIdx.x;
  [[maybe_unused]] const int lane = tid & 63;
  const tq_visit visit = tq_entry(queue, tiles_x, tiles_y);
  const int r0 = visit.ty * PF_WD_TH, c0 = visit.tx * PF_WD_TW;
  int* const w = w_rows + (size_t)visit.b * (size_t)R * (size_t)C;
  tq_open(visit, flag_now, count_now);
  for (int i = tid; i < LN; i += PF_WD_THREADS) {
    const int r = r0 + i / LW - 1, c = c0 + i % LW - 1;
    int dv = 0, wv = 0;
    if (r >= 0 && r < R && c >= 0 && c < C) {
      const size_t v = (size_t)r * (size_t)C + (size_t)c;
      dv = d2[v];
      wv = wd_load(w + v);
    }
    ld[i] = dv; lw[i] = wv;
  }
  __syncthreads();
  constexpr int TOP = 0x7FFFFFFF;
  int li[PER], dv[PER], s_nw[PER], s_ne[PER], s_sw[PER], s_se[PER], w0[PER], cur[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_WD_THREADS;
    li[j] = (i / PF_WD_TW + 1) * LW + i % PF_WD_TW + 1;
    const int l = li[j];
    dv[j] = ld[l];
    const int n = ld[l - LW], s = ld[l + LW], wst = ld[l - 1], e = ld[l + 1];
    // what a diagonal neighbour's w is cut to on its way in: nothing without diagonals, the two side cells under restrict_corner
    s_nw[j] = !allow_diag ? 0 : !restrict_corner ? TOP : (n < wst ? n : wst);
    s_ne[j] = !allow_diag ? 0 : !restrict_corner ? TOP : (n < e ? n : e);
    s_sw[j] = !allow_diag ? 0 : !restrict_corner ? TOP : (s < wst ? s : wst);
    s_se[j] = !allow_diag ? 0 : !restrict_corner ? TOP : (s < e ? s : e);
    w0[j] = cur[j] = lw[l];
  }
  // Sweeps in place: a thread writes its own four words only and reads its neighbours' while they may be rising (whole 32-bit LDS
  // words, values only rise).  A sweep in which nobody wrote saw one state throughout: the fixed point under this halo.
  volatile int* const vw = lw;
  int changed;
  do {
    changed = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int l = li[j];
      int best = vw[l - 1];
      int x = vw[l + 1]; best = x > best ? x : best;
      x = vw[l - LW]; best = x > best ? x : best;
      x = vw[l + LW]; best = x > best ? x : best;
      x = vw[l - LW - 1]; x = x < s_nw[j] ? x : s_nw[j]; best = x > best ? x : best;
      x = vw[l - LW + 1]; x = x < s_ne[j] ? x : s_ne[j]; best = x > best ? x : best;
      x = vw[l + LW - 1]; x = x < s_sw[j] ? x : s_sw[j]; best = x > best ? x : best;
      x = vw[l + LW + 1]; x = x < s_se[j] ? x : s_se[j]; best = x > best ? x : best;
      best = best < dv[j] ? best : dv[j];
      best = best > cur[j] ? best : cur[j];
#if PF_WD_ROW_SCAN
      best = wd_row_scan(best, dv[j], lane);
#endif
      if (best > cur[j]) { cur[j] = best; vw[l] = best; changed = 1; }
    }
  } while (__syncthreads_or(changed));
  int sides = 0, raised = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const bool rose = cur[j] > w0[j];                                // (a cell beyond the grid has d2 0 and never rises)
    if (!rose && !(first && cur[j] > 0)) continue;                   // the first launch: a seed rose in the seeding kernel, its neighbours are told here
    const int i = tid + j * PF_WD_THREADS, lr = i / PF_WD_TW, lc = i % PF_WD_TW;
    if (rose) {
      wd_store(w + (size_t)(r0 + lr) * (size_t)C + (size_t)(c0 + lc), cur[j]);
      raised += 1;
    }
    sides |= tq_side_bits<PF_WD_TW, PF_WD_TH>(lr, lc);
  }
  tq_close(visit, sides, raised, allow_diag, tiles_x, tiles_y, flag_next, queue_next, count_next, raised_total);
}

// keys[b] = the smallest (w << 32) | id over the cells of row b with w >= 1 (preset to all ones), cells[b] += their number
__global__ __launch_bounds__(PF_WD_THREADS) void k_widest_info_sum(const int* __restrict__ w_rows, int RC, int B, unsigned long long* __restrict__ keys,
                                                                     unsigned long long* __restrict__ cells) {
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const int* const w = w_rows + (size_t)b * (size_t)RC;
    unsigned long long best = ~0ull;
    int n = 0;
    for (int v = (int)(blockIdx.x * PF_WD_THREADS + threadIdx.x); v < RC; v += (int)(gridDim.x * PF_WD_THREADS)) {
      const int x = w[v];
      if (x < 1) continue;
      n += 1;
      const unsigned long long key = ((unsigned long long)(unsigned)x << 32) | (unsigned long long)(unsigned)v;
      best = key < best ? key : best;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(best, d);
      best = o < best ? o : best;
      n += __shfl_xor(n, d);
    }
    if ((threadIdx.x & 63u) == 0 && n) {
      atomicMin(keys + b, best);
      atomicAdd(cells + b, (unsigned long long)n);
    }
  }
}

__global__ __launch_bounds__(PF_WD_THREADS) void k_widest_write_info(int B, const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ cells,
                                                                          const unsigned long long* __restrict__ nsrc, long long* __restrict__ info) {
  const int b = (int)(blockIdx.x * PF_WD_THREADS + threadIdx.x);
  if (b >= B) return;
  const long long n = (long long)cells[b];
  info[4 * (size_t)b + 0] = (long long)nsrc[b];
  info[4 * (size_t)b + 1] = n;
  info[4 * (size_t)b + 2] = n ? (long long)(keys[b] >> 32) : -1;
  info[4 * (size_t)b + 3] = n ? (long long)(keys[b] & 0xFFFFFFFFull) : -1;
}

}  // namespace pf
