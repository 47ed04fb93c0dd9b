// pf_cost_field.h -- cost fields: exact weighted shortest paths over a per-cell cost map c (pf_cost_field, pf_cost_field_parents,
// pf_cost_paths).  The block-wise fast iterative method on min-plus labels, bit-reproducible, no priority queue.
//
// The rule.  c is a double per cell, finite with 1 <= c <= 2^20 on every free cell (obstacle words are never read for a result).
// A legal move u -> v by move k (legality: the mask byte pf_dist_field_merged uses) weighs
//     w = m (k < 4),  w = fl(PF_SQRT2 m) (k >= 4),  m = fl(0.5 fl(c[u] + c[v]))
// -- symmetric, and exactly 1 / PF_SQRT2 when c == 1.  D[b] is the least fixed point of  D[s] = 0 on the free sources of set b,
// D[v] = min over legal moves u -> v of fl(D[u] + w(u, v))  elsewhere; +inf on obstacles and out of reach.  w >= 1 makes every
// parent's label strictly smaller and the sources the only zeros; c <= 2^20 keeps the labels far below 2^53.
//
//   k_cost_validate_free_cells     a reduction over the free cells: the smallest cell id whose cost is not in [1, 2^20] (NaN fails
//                                  both comparisons).  The host reads the word before anything is written: a refused call leaves
//                                  every output untouched.
//   k_cost_fill_inf / k_cost_seed_sets   the rows become +inf; one thread per listed source (tq_seed_sets): skipped on an obstacle, an atomic
//                                  min of 0 on the label (the one that found +inf counts the source: listed twice counts once),
//                                  and the source's tile goes on the first queue.
//   k_cost_relax_tiles_in_lds      one workgroup per queued (set, tile), the tile of pf_widest.h (64 x 16 cells, four per thread):
//                                  loads D and c of its cells and a one-cell halo into LDS (+inf / 1 beyond the grid), forms the
//                                  eight incoming weights of each of its cells ONCE into registers (+inf for a move the mask
//                                  forbids and for every move into an obstacle, whose own mask byte is not zero: the occupancy
//                                  says so; obstacle costs never enter a sum), then sweeps: every thread reads the eight
//                                  neighbour labels of its cells and forms min fl(D[u] + w); barrier; the cells that fell are
//                                  written; barrier -- until one whole sweep lowers nothing: the tile's own fixed point under the
//                                  halo it read.  It stores the words that fell and queues, for the next launch, the neighbour
//                                  tiles that hold a lowered cell in their halo.  Opening and closing the visit, the queues,
//                                  flags and parity are pf_tile_queue.h's.
//   k_cost_info_largest / _arg / k_cost_write_info   cells with a finite label and the largest finite label per set (one atomic
//                                  max on the label's bits: non-negative doubles order as their bits), then the smallest cell
//                                  that attains it, then the four words.
//   k_cost_parent_map_thread_per_cell   pf_field_paths.h's rule with w(u, v) in place of 1 / PF_SQRT2: the u with the smallest
//                                  (D[u], u) among the cells with a legal move u -> v and fl(D[u] + w(u, v)) == D[v].
//   k_cost_paths_one_wave_per_row  the lanes form the weights of 64 consecutive steps and check them (a king move between cells
//                                  inside the grid); the sum is then taken left to right, one fl(total + w) per step.
//
// Why the sweeps are read / barrier / write and not in place.  A label is a 64-bit word.  pf_widest.h sweeps 32-bit words in
// place; nothing we can cite says that an aligned 64-bit LDS access is read and written whole against a concurrent access of
// another wavefront, and a word mixed from two labels need not be the cost of any walk -- it could lie BELOW the answer, which
// no later sweep repairs.  So no thread writes a label while another may read it.
//
// Why this is exact (the transpose of pf_widest.h's argument).  (1) Values only fall, and every value ever stored in D[v] is
// fl(D'[u] + w(u, v)) for a value D'[u] that was stored in D[u] earlier (or the seed 0): by induction it is the left-to-right
// rounded cost of a real walk from a source.  Along any walk, fl(. + w) is monotone, so by induction over an OPTIMAL walk's
// prefix order no walk's rounded cost lies below the least fixed point's label of its end: every stored value is >= the answer.
// Nothing is ever summed ahead: there is no segment scan here (a pre-summed segment rounds differently).  (2) A halo word that
// the neighbour tile is lowering in the same launch may be read old or new: what is read was stored (cf_load, cf_store and the
// seed's minimum are whole-word 64-bit agent-scope relaxed atomics), and by (1) it is a valid upper bound.  pf_tile_queue.h has
// the rest of this half -- one writer per (set, tile) per launch, whoever lowers a border cell queues its readers for the next
// launch, no other synchronisation --: when no tile is queued, the whole row is a fixed point above the seeds.  (3) A fixed
// point with D[s] = 0 on the seeds is <= the least one's label along every optimal walk (induction along the walk, fl monotone),
// so with (1) it IS the least fixed point, whatever the timing: identical run to run, bit for bit.
//
// Rounds.  After round k every cell with an optimal walk that crosses tile borders at most k - 1 times is final (the tile before
// the last crossing was final a round earlier and queued this one; the rest of the walk lies inside the tile, which runs to its
// own fixed point).  w >= 1 makes an optimal walk simple, so the rounds stay below R C + 2, which the host enforces.  Unlike the
// level kernel of pf_dist_field.h the rounds do not grow with the labels, only with the tiles an optimal walk crosses -- and
// a tile may be visited again whenever a cheaper route reaches its halo later than a dearer one.
#pragma once

namespace pf {

#define PF_CF_THREADS 256
#define PF_CF_COST_MAX 1048576.0                /* 2^20 */

__device__ __forceinline__ double cf_load(const double* p) {
  return __builtin_bit_cast(double, __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void cf_store(double* p, double v) {
  __hip_atomic_store((unsigned long long*)p, __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the weight of move k between cells of cost cu and cv (either direction: the sum commutes)
PF_DEV double cf_weight(double cu, double cv, int k) {
  const double m = 0.5 * (cu + cv);
  return k < 4 ? m : PF_SQRT2 * m;
}

__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_validate_free_cells(const uint8_t* __restrict__ occ, const double* __restrict__ cost, int RC, int* bad) {
  int first = 0x7FFFFFFF;
  for (int v = (int)(blockIdx.x * PF_CF_THREADS + threadIdx.x); v < RC; v += (int)(gridDim.x * PF_CF_THREADS)) {
    if (occ[v] == 1) continue;
    const double c = cost[v];
    if (!(c >= 1.0 && c <= PF_CF_COST_MAX)) first = v < first ? v : first;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(first, d); first = o < first ? o : first; }
  if ((threadIdx.x & 63u) == 0 && first != 0x7FFFFFFF) atomicMin(bad, first);
}

__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_fill_inf(unsigned long long* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * PF_CF_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * PF_CF_THREADS) p[i] = PF_DF_INF_BITS;
}

__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_seed_sets(const uint8_t* __restrict__ occ, int RC, int C, int tiles_x, int ntiles, int B,
                                                                    const int* __restrict__ off, const int* __restrict__ src, double* __restrict__ rows,
                                                                    int* __restrict__ flag, int* __restrict__ queue, int* __restrict__ count,
                                                                    unsigned long long* __restrict__ nsrc) {
  tq_seed_sets<PF_CF_THREADS, PF_WD_TW, PF_WD_TH>(RC, C, tiles_x, ntiles, B, off, src, flag, queue, count, nsrc, [&](int b, int s) {
    if (occ[s] == 1) return false;                                   // a source ON an obstacle is no source
    unsigned long long* const word = (unsigned long long*)(rows + (size_t)b * (size_t)RC + (size_t)s);
    return __hip_atomic_fetch_min(word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == PF_DF_INF_BITS;   // otherwise: listed twice
  });
}

__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_relax_tiles_in_lds(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, const double* __restrict__ cost, int R, int C, int allow_diag,
                                                                             int tiles_x, int tiles_y, double* d_rows, const int* __restrict__ queue, int nqueue, int first,
                                                                             int* flag_now, int* count_now, int* flag_next, int* __restrict__ queue_next, int* count_next,
                                                                             unsigned long long* __restrict__ lowered_total) {
  constexpr int PER = PF_WD_TW * PF_WD_TH / PF_CF_THREADS, LW = PF_WD_LW, LN = PF_WD_LW * PF_WD_LH;
  __shared__ double ld[LN];
  __shared__ double lc[LN];
  if ((int)blockIdx.x >= nqueue) return;
  const int tid = (int)threadIdx.x;
  const tq_visit visit = tq_entry(queue, tiles_x, tiles_y);
  const int r0 = visit.ty * PF_WD_TH, c0 = visit.tx * PF_WD_TW;
  double* const D = d_rows + (size_t)visit.b * (size_t)R * (size_t)C;
  const double inf = __builtin_bit_cast(double, PF_DF_INF_BITS);
  tq_open(visit, flag_now, count_now);
  for (int i = tid; i < LN; i += PF_CF_THREADS) {
    const int r = r0 + i / LW - 1, c = c0 + i % LW - 1;
    double dv = inf, cv = 1.0;
    if (r >= 0 && r < R && c >= 0 && c < C) {
      const size_t v = (size_t)r * (size_t)C + (size_t)c;
      cv = cost[v];
      dv = cf_load(D + v);
    }
    ld[i] = dv; lc[i] = cv;
  }
  __syncthreads();
  int li[PER];
  double w[PER][8], w0[PER], cur[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_CF_THREADS, lr = i / PF_WD_TW, lcn = i % PF_WD_TW;
    li[j] = (lr + 1) * LW + lcn + 1;
    const int l = li[j];
    const int r = r0 + lr, c = c0 + lcn;
    unsigned m = 0u;                                                 // beyond the grid or on an obstacle: takes nothing (an obstacle's own byte is not zero)
    if (r < R && c < C) { const size_t v = (size_t)r * (size_t)C + (size_t)c; m = occ[v] == 1 ? 0u : mm[v]; }
    const double cv = lc[l];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                    // u = v - step(k) moves into v by move k: bit opp(k) of v's own byte
      const int opp = k < 4 ? (k ^ 1) : 11 - k;
      const double cu = lc[l - (move_dr(k) * LW + move_dc(k))];
      w[j][k] = ((m >> opp) & 1u) ? cf_weight(cu, cv, k) : inf;
    }
    w0[j] = cur[j] = ld[l];
  }
  int changed;
  do {
    changed = 0;
    double nb[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int l = li[j];
      double best = cur[j];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double x = ld[l - (move_dr(k) * LW + move_dc(k))] + w[j][k];
        best = x < best ? x : best;
      }
      nb[j] = best;
    }
    __syncthreads();                                                 // every read of this sweep is done: now the writes
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (nb[j] < cur[j]) { cur[j] = nb[j]; ld[li[j]] = nb[j]; changed = 1; }
  } while (__syncthreads_or(changed));
  int sides = 0, lowered = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const bool fell = cur[j] < w0[j];                                // (a cell beyond the grid or on an obstacle stays +inf)
    if (!fell && !(first && cur[j] == 0.0)) continue;                // the first launch: a seed fell in the seeding kernel, its neighbours are told here
    const int i = tid + j * PF_CF_THREADS, lr = i / PF_WD_TW, lcn = i % PF_WD_TW;
    if (fell) {
      cf_store(D + (size_t)(r0 + lr) * (size_t)C + (size_t)(c0 + lcn), cur[j]);
      lowered += 1;
    }
    sides |= tq_side_bits<PF_WD_TW, PF_WD_TH>(lr, lcn);
  }
  tq_close(visit, sides, lowered, allow_diag, tiles_x, tiles_y, flag_next, queue_next, count_next, lowered_total);
}

// largest[b] = the largest finite label's bits of row b (preset to 0), cells[b] += the cells with a finite label
__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_info_largest(const double* __restrict__ rows, int RC, int B, unsigned long long* __restrict__ largest,
                                                                       unsigned long long* __restrict__ cells) {
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const unsigned long long* const D = (const unsigned long long*)(rows + (size_t)b * (size_t)RC);
    unsigned long long best = 0ull;
    int n = 0;
    for (int v = (int)(blockIdx.x * PF_CF_THREADS + threadIdx.x); v < RC; v += (int)(gridDim.x * PF_CF_THREADS)) {
      const unsigned long long x = D[v];
      if (x >= PF_DF_INF_BITS) continue;
      n += 1;
      best = x > best ? x : best;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(best, d);
      best = o > best ? o : best;
      n += __shfl_xor(n, d);
    }
    if ((threadIdx.x & 63u) == 0 && n) {
      atomicMax(largest + b, best);
      atomicAdd(cells + b, (unsigned long long)n);
    }
  }
}

// arg[b] = the smallest cell of row b whose label's bits are largest[b] (preset to 0x7FFFFFFF)
__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_info_arg(const double* __restrict__ rows, int RC, int B, const unsigned long long* __restrict__ largest,
                                                                   int* __restrict__ arg) {
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const unsigned long long* const D = (const unsigned long long*)(rows + (size_t)b * (size_t)RC);
    const unsigned long long want = largest[b];
    int first = 0x7FFFFFFF;
    for (int v = (int)(blockIdx.x * PF_CF_THREADS + threadIdx.x); v < RC; v += (int)(gridDim.x * PF_CF_THREADS))
      if (D[v] == want) first = v < first ? v : first;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(first, d); first = o < first ? o : first; }
    if ((threadIdx.x & 63u) == 0 && first != 0x7FFFFFFF) atomicMin(arg + b, first);
  }
}

__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_write_info(int B, const unsigned long long* __restrict__ cells, const unsigned long long* __restrict__ nsrc,
                                                                     const int* __restrict__ arg, long long* __restrict__ info) {
  const int b = (int)(blockIdx.x * PF_CF_THREADS + threadIdx.x);
  if (b >= B) return;
  const long long n = (long long)cells[b];
  info[4 * (size_t)b + 0] = (long long)nsrc[b];
  info[4 * (size_t)b + 1] = n;
  info[4 * (size_t)b + 2] = n ? (long long)arg[b] : -1;
  info[4 * (size_t)b + 3] = 0;
}

// One thread per cell, looping over the fields: pf_field_paths.h's kernel with the move's weight formed from the two costs.
// Bandwidth-bound in the same way (8 B of label, 8 B of cost and 1 B of mask in, 1 B out per cell; the neighbours' words come
// out of L2 / L1).  The fields were written by earlier kernels on the same stream: plain loads.
__global__ __launch_bounds__(PF_FP_THREADS) void k_cost_parent_map_thread_per_cell(const uint8_t* __restrict__ mm, const double* __restrict__ cost, int RC, int C, int K,
                                                                                     const double* __restrict__ fields, uint8_t* __restrict__ parents, int* err) {
  const int v = (int)blockIdx.x * PF_FP_THREADS + (int)threadIdx.x;
  if (v >= RC) return;
  const unsigned m = mm[v];
  const double cv = cost[v];
  double wk[8];
  int uk[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int opp = k < 4 ? (k ^ 1) : 11 - k;
    uk[k] = ((m >> opp) & 1u) ? v - (move_dr(k) * C + move_dc(k)) : -1;   // a set bit means u lies inside the grid
    wk[k] = uk[k] >= 0 ? cf_weight(cost[uk[k]], cv, k) : 0.0;
  }
  for (int f = (int)blockIdx.y; f < K; f += (int)gridDim.y) {
    const double* const D = fields + (size_t)f * (size_t)RC;
    const double dv = D[v];
    const unsigned long long vb = __builtin_bit_cast(unsigned long long, dv);
    unsigned code = PF_FP_NONE;
    if (vb == 0ull) code = PF_FP_SOURCE;                             // D == +0.0: a source (the weights being >= 1, nothing else)
    else if (vb < PF_DF_INF_BITS) {
      unsigned long long best = ~0ull;
      int bu = 0x7FFFFFFF;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (uk[k] < 0) continue;
        const double du = D[uk[k]];
        if (du + wk[k] != dv) continue;
        const unsigned long long ub = __builtin_bit_cast(unsigned long long, du);   // (non-negative doubles order as their bits)
        if (ub < best || (ub == best && uk[k] < bu)) { best = ub; bu = uk[k]; code = (unsigned)k; }
      }
      if (code == PF_FP_NONE) *err = 1;                              // (cannot happen for a fixed point; the byte is still written)
    }
    parents[(size_t)f * (size_t)RC + (size_t)v] = (uint8_t)code;
  }
}

// The path-row scorer, one wavefront per row (also pf_turn_field.h's): the lanes form the weights of 64 consecutive steps and
// check them, then the sum is taken left to right.  -> the sum; at = -1, or the first step that is no king move between cells
// inside the grid (0 for an empty row, a length beyond path_cap or a lone cell outside the grid; the sum means nothing then).
// UNIT_IF_NULL: a null cost map is a map of ones.  step(i, a, dr, dc, w, mark) -> what step i = a -> a + (dr, dc) of weight w adds
// to the sum, and may set the lane's mark (0 before); trip(mark) runs once for every 64 steps that passed the check.
template <bool UNIT_IF_NULL, typename Step, typename Trip>
__device__ __forceinline__ double cf_score_row(const double* __restrict__ cost, int RC, int C, const int* __restrict__ row, int L, int path_cap, int lane, int& at,
                                               Step step, Trip trip) {
  double sum = 0.0;
  at = -1;
  if (L < 1 || L > path_cap) at = 0;
  else if (L == 1 && (unsigned)row[0] >= (unsigned)RC) at = 0;
  for (int base = 0; at < 0 && base + 1 < L; base += 64) {           // (uniform: the whole wavefront)
    const int i = base + lane;                                       // the step row[i] -> row[i + 1]
    double e = 0.0;
    int off = 0, mark = 0;
    if (i + 1 < L) {
      const int a = row[i], b = row[i + 1];
      if ((unsigned)a >= (unsigned)RC || (unsigned)b >= (unsigned)RC) off = 1;
      else {
        const int dr = b / C - a / C, dc = b % C - a % C;
        if (dr < -1 || dr > 1 || dc < -1 || dc > 1 || (dr == 0 && dc == 0)) off = 1;
        else {
          const bool unit = UNIT_IF_NULL && !cost;
          e = step(i, a, dr, dc, cf_weight(unit ? 1.0 : cost[a], unit ? 1.0 : cost[b], (dr != 0 && dc != 0) ? 4 : 0), mark);
        }
      }
    }
    const unsigned long long offs = __ballot(off);
    if (offs) { at = base + __builtin_ctzll(offs); break; }
    trip(mark);
    const int steps = L - 1 - base < 64 ? L - 1 - base : 64;
    for (int t = 0; t < steps; ++t) sum += __shfl(e, t);             // one rounded addition per step, in the row's order
  }
  return sum;
}

// total[p] = the left-to-right sum of the weights of row p's steps, bad[p] = -1; or NaN and the first bad step (cf_score_row)
__global__ __launch_bounds__(64) void k_cost_paths_one_wave_per_row(const double* __restrict__ cost, int RC, int C, int n, int path_cap, const int* __restrict__ cells,
                                                                      const int* __restrict__ len, double* __restrict__ total, int* __restrict__ bad) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (p >= n) return;
  int at;
  const double sum = cf_score_row<false>(cost, RC, C, cells + (size_t)p * (size_t)path_cap, len[p], path_cap, lane, at,
                                         [](int, int, int, int, double w, int&) { return w; }, [](int) {});
  if (lane == 0) {
    total[p] = at >= 0 ? __builtin_bit_cast(double, 0x7FF8000000000000ull) : sum;
    bad[p] = at;
  }
}

}  // namespace pf
