// pf_turn_field.h -- turn fields: the exact optimum of length plus a turn penalty, over (cell, heading) states (pf_turn_field,
// pf_turn_field_paths, pf_turn_paths).  The block-wise fast iterative method of pf_cost_field.h on eight min-plus
// labels per cell, bit-reproducible, no priority queue.
//
// The rule.  Moves, legality and the move weight w(u, v, k) are pf_cost_field.h's (c == 1 everywhere when there is no cost map: the
// same bits as a map of ones).  wt is the turn weight, finite in [0, 2^20].  T[d][v] is the cheapest cost of a walk from a source
// that ENTERS v by move d: 0 for all eight d on a free source (the first move of a path is no turn), and elsewhere, with
// u = v - step(d) and the move u -> v legal,
//     T[d][v] = min( fl(T[d][u] + w),  fl(M[u] + fl(w + wt)) ),   M[u] = min over d' of T[d'][u]
// -- the same as min over d' of fl(T[d'][u] + e(d', d)), e = w for d' == d and fl(w + wt) otherwise, because fl(x + e) is monotone in x
// and in e (and w <= fl(w + wt)).  +inf where the move is illegal, on obstacles and out of reach.  best[v] = M[v].
//
//   k_turn_seed_sets               one thread per listed source: skipped on an obstacle, an atomic min of 0 on best[s] (the one that
//                                  found +inf counts the source and stores 0 into the eight states), the source's tile is queued.
//   k_turn_relax_tiles_in_lds      one workgroup per queued (set, tile) of PF_TF_TW x PF_TF_TH cells: the costs of the tile and a
//                                  one-cell halo pass through LDS once and the eight incoming weights of each cell are formed ONCE
//                                  into registers, w and fl(w + wt) (+inf for a move the mask forbids and for every move into an
//                                  obstacle); then the eight labels of the cells and the halo are loaded and M is formed: nine
//                                  doubles per cell in LDS.  A sweep: every thread reads, for each state (v, d) of its cells, the
//                                  two words T[d][u] and M[u] of u = v - step(d); barrier; the states that fell and the new M are
//                                  written; barrier -- until one whole sweep lowers nothing.  The words that fell are stored (the
//                                  states and best) and the neighbour tiles that hold a lowered cell in their halo are queued for
//                                  the next launch.  Opening and closing the visit, the queues, flags and parity are
//                                  pf_tile_queue.h's.
//   k_turn_trace_query_lanes       the route rule, one lane per query, the field alone: at the target the heading with the smallest
//                                  (T[d][t], d); at (v, d) step to u = v - step(d); stop when M[u] == 0; otherwise the d' with the
//                                  smallest (T[d'][u], d') among those with fl(T[d'][u] + e(d', d)) == T[d][v] bit for bit.  Labels
//                                  fall strictly along the chase (e >= 1).  Walked twice (counted, then written) as
//                                  pf_field_paths.h's trace; bounded by min(path_cap, R C) cells whatever the words hold.
//   k_turn_paths_one_wave_per_row  the rule's left-to-right cost of any path rows and their turn count (helper.py's count_turns).
//
// Why the sweeps are read / barrier / write: pf_cost_field.h's reason, a label is a 64-bit LDS word.
//
// Why this is exact (pf_cost_field.h's argument, over states).  (1) Values only fall, and every value ever stored in T[d][v] is
// fl(T'[d'][u] + e(d', d)) for a value stored in T[d'][u] earlier (or a seed's 0): by induction the left-to-right rounded cost of a
// real walk from a source that enters v by d (a walk may pass a cell twice: into (v, d) when u is a dead end reachable only through
// v).  fl(. + e) is monotone, so by induction over an optimal walk's prefixes no walk's rounded cost lies below the least fixed
// point's label of its end state: every stored value is >= the answer.  M is a minimum of such values.  Nothing is summed ahead.
// (2) A halo word that the neighbour tile is lowering in the same launch may be read old or new: what is read was stored (whole
// 64-bit words, cf_load and cf_store) and by (1) is a valid upper bound; the eight words of a halo cell may be of different ages,
// each is valid on its own and so is their minimum.  pf_tile_queue.h has the rest of this half -- one writer per (set, tile) per
// launch, whoever lowers a border cell's state queues its readers for the next launch, no other synchronisation --: when no tile
// is queued, the whole array is a fixed point above the seeds.  (3) A fixed point with T[.][s] = 0 on the seeds
// is <= the least one's label along every optimal walk (induction along the walk), so with (1) it IS the least fixed point,
// whatever the timing: identical run to run, bit for bit.
//
// Bounds, never tuning knobs.  A walk that is optimal into its end state visits a STATE once (e >= 1), so inside a tile a sweep
// count above its states + 2 cannot happen: the loop stops there and raises the error word.  A walk that is optimal into a best
// state is simple in cells (a loop costs two weights and saves no turn), but the states of the field as a whole need walks of up
// to 8 R C states: the host stops after 8 R C + 2 rounds.  Either way the call fails with a message and never spins.
#pragma once

namespace pf {

#ifndef PF_TF_TW
#define PF_TF_TW 32                             /* the tile: 32 x 16 cells, two per thread; a wavefront holds two tile rows (DESIGN.md 4.20 has the measurement */
#endif                                          /* against 64 x 8, 64 x 16 and 32 x 8: -DPF_TF_TW / -DPF_TF_TH build the others, scripts/probe_turn_field.py) */
#ifndef PF_TF_TH
#define PF_TF_TH 16
#endif
#define PF_TF_THREADS 256
#define PF_TF_LW (PF_TF_TW + 2)                 /* the tile and its halo in LDS */
#define PF_TF_LH (PF_TF_TH + 2)
#define PF_TF_PER (PF_TF_TW * PF_TF_TH / PF_TF_THREADS)
#define PF_TF_SWEEP_BOUND (8 * PF_TF_TW * PF_TF_TH + 2)
#define PF_TF_WEIGHT_MAX 1048576.0              /* 2^20 */

static_assert(PF_TF_PER >= 1 && PF_TF_PER * PF_TF_THREADS == PF_TF_TW * PF_TF_TH, "the tile is a whole number of cells per thread");

__global__ __launch_bounds__(PF_TF_THREADS) void k_turn_seed_sets(const uint8_t* __restrict__ occ, int RC, int C, int tiles_x, int ntiles, int B,
                                                                    const int* __restrict__ off, const int* __restrict__ src, double* __restrict__ states,
                                                                    double* __restrict__ best, int* __restrict__ flag, int* __restrict__ queue,
                                                                    int* __restrict__ count, unsigned long long* __restrict__ nsrc) {
  tq_seed_sets<PF_TF_THREADS, PF_TF_TW, PF_TF_TH>(RC, C, tiles_x, ntiles, B, off, src, flag, queue, count, nsrc, [&](int b, int s) {
    if (occ[s] == 1) return false;                                   // a source ON an obstacle is no source
    unsigned long long* const word = (unsigned long long*)(best + (size_t)b * (size_t)RC + (size_t)s);
    if (__hip_atomic_fetch_min(word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != PF_DF_INF_BITS) return false;   // listed twice
    double* state = states + (size_t)b * 8 * (size_t)RC + (size_t)s;
#pragma unroll
    for (int d = 0; d < 8; ++d, state += RC) cf_store(state, 0.0);
    return true;
  });
}

// counters[0] += the state words lowered; counters[1] = 1 when a tile hit the sweep bound
__global__ __launch_bounds__(PF_TF_THREADS) void k_turn_relax_tiles_in_lds(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, const double* __restrict__ cost, double wt,
                                                                             int R, int C, int allow_diag, int tiles_x, int tiles_y, double* d_states, double* d_best,
                                                                             const int* __restrict__ queue, int nqueue, int first, int* flag_now, int* count_now, int* flag_next,
                                                                             int* __restrict__ queue_next, int* count_next, unsigned long long* __restrict__ counters) {
  constexpr int PER = PF_TF_PER, LW = PF_TF_LW, LN = PF_TF_LW * PF_TF_LH;
  __shared__ double lt[9][LN];                                       // planes 0..7: T[d]; plane 8: M (and, before the labels come, the costs)
  if ((int)blockIdx.x >= nqueue) return;
  const int tid = (int)threadIdx.x;
  const tq_visit visit = tq_entry(queue, tiles_x, tiles_y);
  const int r0 = visit.ty * PF_TF_TH, c0 = visit.tx * PF_TF_TW;
  const size_t RC = (size_t)R * (size_t)C;
  double* const T = d_states + (size_t)visit.b * 8 * RC;
  double* const Mg = d_best + (size_t)visit.b * RC;
  const double inf = __builtin_bit_cast(double, PF_DF_INF_BITS);
  tq_open(visit, flag_now, count_now);
  for (int i = tid; i < LN; i += PF_TF_THREADS) {
    const int r = r0 + i / LW - 1, c = c0 + i % LW - 1;
    double cv = 1.0;
    if (cost && r >= 0 && r < R && c >= 0 && c < C) cv = cost[(size_t)r * (size_t)C + (size_t)c];
    lt[8][i] = cv;
  }
  __syncthreads();
  int li[PER];
  double w[PER][8], wturn[PER][8];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_TF_THREADS, lr = i / PF_TF_TW, lcn = i % PF_TF_TW;
    li[j] = (lr + 1) * LW + lcn + 1;
    const int l = li[j];
    const int r = r0 + lr, c = c0 + lcn;
    unsigned m = 0u;                                                 // beyond the grid or on an obstacle: takes nothing (an obstacle's own byte is not zero)
    if (r < R && c < C) { const size_t v = (size_t)r * (size_t)C + (size_t)c; m = occ[v] == 1 ? 0u : mm[v]; }
    const double cv = lt[8][l];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                    // u = v - step(k) moves into v by move k: bit opp(k) of v's own byte
      const int opp = k < 4 ? (k ^ 1) : 11 - k;
      const double cu = lt[8][l - (move_dr(k) * LW + move_dc(k))];
      w[j][k] = ((m >> opp) & 1u) ? cf_weight(cu, cv, k) : inf;
      wturn[j][k] = w[j][k] + wt;
    }
  }
  __syncthreads();                                                   // the costs are in registers: plane 8 becomes M
  for (int i = tid; i < LN; i += PF_TF_THREADS) {
    const int r = r0 + i / LW - 1, c = c0 + i % LW - 1;
    const bool in = r >= 0 && r < R && c >= 0 && c < C;
    const size_t v = in ? (size_t)r * (size_t)C + (size_t)c : 0;
    double least = inf;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const double x = in ? cf_load(T + (size_t)d * RC + v) : inf;
      lt[d][i] = x;
      least = x < least ? x : least;
    }
    lt[8][i] = least;
  }
  __syncthreads();
  double cur[PER][8], curm[PER];
  unsigned fell[PER];                                                // bits 0..7: the states that fell in this visit; bit 8: M
#pragma unroll
  for (int j = 0; j < PER; ++j) {
#pragma unroll
    for (int d = 0; d < 8; ++d) cur[j][d] = lt[d][li[j]];
    curm[j] = lt[8][li[j]];
    fell[j] = 0u;
  }
  int sweeps = 0, stuck = 0;
  for (;;) {
    unsigned now[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int l = li[j];
      now[j] = 0u;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const int lu = l - (move_dr(d) * LW + move_dc(d));
        const double straight = lt[d][lu] + w[j][d], turned = lt[8][lu] + wturn[j][d];
        const double x = straight < turned ? straight : turned;
        if (x < cur[j][d]) { cur[j][d] = x; now[j] |= 1u << d; }
      }
    }
    __syncthreads();                                                 // every read of this sweep is done: now the writes
    int changed = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (!now[j]) continue;
      changed = 1;
      fell[j] |= now[j];
      double least = curm[j];
#pragma unroll
      for (int d = 0; d < 8; ++d)
        if ((now[j] >> d) & 1u) { lt[d][li[j]] = cur[j][d]; least = cur[j][d] < least ? cur[j][d] : least; }
      if (least < curm[j]) { curm[j] = least; lt[8][li[j]] = least; fell[j] |= 256u; }
    }
    sweeps += 1;
    if (!__syncthreads_or(changed)) break;
    if (sweeps >= PF_TF_SWEEP_BOUND) { stuck = 1; break; }           // (uniform: cannot happen, see the header)
  }
  int sides = 0, lowered = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (!fell[j] && !(first && curm[j] == 0.0)) continue;            // the first launch: a seed fell in the seeding kernel, its neighbours are told here
    const int i = tid + j * PF_TF_THREADS, lr = i / PF_TF_TW, lcn = i % PF_TF_TW;
    const size_t v = (size_t)(r0 + lr) * (size_t)C + (size_t)(c0 + lcn);   // (a cell beyond the grid or on an obstacle stays +inf: never here)
#pragma unroll
    for (int d = 0; d < 8; ++d)
      if ((fell[j] >> d) & 1u) cf_store(T + (size_t)d * RC + v, cur[j][d]);
    if (fell[j] & 256u) cf_store(Mg + v, curm[j]);
    lowered += __builtin_popcount(fell[j] & 255u);
    sides |= tq_side_bits<PF_TF_TW, PF_TF_TH>(lr, lcn);
  }
  tq_close(visit, sides, lowered, allow_diag, tiles_x, tiles_y, flag_next, queue_next, count_next, counters);
  if (tid == 0 && stuck) counters[1] = 1ull;
}

// One walk of the route rule from target t through the states T [8][RC] of one set: the cells go to row (WRITE: cnt_known of them,
// counted by the walk before) -> the number of cells, 0 where the target has no finite state, -1 where the walk would pass lim
// cells, leave the grid or finds no state that offers the label (words that are no fixed point).
template <bool WRITE>
PF_DEV int tf_walk(const double* __restrict__ T, const double* __restrict__ cost, double wt, int R, int C, int t, int lim, int* row, int reverse, int cnt_known) {
  const size_t RC = (size_t)R * (size_t)C;
  unsigned long long lab = ~0ull;
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned long long x = __builtin_bit_cast(unsigned long long, T[(size_t)k * RC + (size_t)t]);   // (non-negative doubles order as their bits)
    if (x < lab) { lab = x; d = k; }
  }
  if (lab >= PF_DF_INF_BITS) return 0;
  int v = t, cnt = 1;
  if (WRITE) row[reverse ? 0 : cnt_known - 1] = t;
  if (lab == 0ull) return 1;                                         // the target is a source
  for (;;) {
    if (cnt >= lim) return -1;
    const int r = v / C, c = v - r * C, ur = r - move_dr(d), uc = c - move_dc(d);
    if (ur < 0 || ur >= R || uc < 0 || uc >= C) return -1;
    const int u = ur * C + uc;
    cnt += 1;
    if (WRITE) row[reverse ? cnt - 1 : cnt_known - cnt] = u;
    const double wd = cf_weight(cost ? cost[u] : 1.0, cost ? cost[v] : 1.0, d), wtd = wd + wt;
    unsigned long long least = ~0ull, pick = ~0ull;
    int nd = -1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double x = T[(size_t)k * RC + (size_t)u];
      const unsigned long long xb = __builtin_bit_cast(unsigned long long, x);
      least = xb < least ? xb : least;
      if (xb >= PF_DF_INF_BITS) continue;
      const double offer = x + (k == d ? wd : wtd);
      if (__builtin_bit_cast(unsigned long long, offer) == lab && xb < pick) { pick = xb; nd = k; }
    }
    if (least == 0ull) return cnt;                                   // M[u] == 0: a source
    if (nd < 0) return -1;
    v = u; d = nd; lab = pick;
  }
}

// status / length per query; a row of d_cells is written only when the status is PF_ST_OK
__global__ __launch_bounds__(PF_FP_TRACE_THREADS) void k_turn_trace_query_lanes(const double* __restrict__ cost, double wt, int R, int C, int B, const double* __restrict__ states,
                                                                                  int n, const int* __restrict__ set_idx, const int* __restrict__ target, int reverse,
                                                                                  int path_cap, int* __restrict__ cells, int* __restrict__ len, int* __restrict__ status) {
  const int q = (int)blockIdx.x * PF_FP_TRACE_THREADS + (int)threadIdx.x;
  if (q >= n) return;
  const int RC = R * C, t = target[q], b = set_idx[q];
  int st = PF_ST_INFEASIBLE, L = 0;
  if (t >= 0 && t < RC && b >= 0 && b < B) {
    const double* const T = states + (size_t)b * 8 * (size_t)RC;
    const int lim = path_cap < RC ? path_cap : RC;                   // a route visits a cell once
    int* const row = cells + (size_t)q * (size_t)path_cap;
    const int cnt = tf_walk<false>(T, cost, wt, R, C, t, lim, row, reverse, 0);
    if (cnt > 0) {                                                   // the second walk writes: the first one has checked every step of it
      tf_walk<true>(T, cost, wt, R, C, t, lim, row, reverse, cnt);
      st = PF_ST_OK; L = cnt;
    } else if (cnt < 0) st = PF_ST_OVERFLOW;
  }
  len[q] = L;
  status[q] = st;
}

// total[p] = the rule's left-to-right cost of row p (a step weighs w, or fl(w + wt) when its move differs from the step's before),
// turns[p] = the steps that turned, bad[p] = -1; or NaN, 0 and the first step that is no king move between cells inside the grid
// (0 for an empty row, a length beyond path_cap or a lone cell outside the grid)
__global__ __launch_bounds__(64) void k_turn_paths_one_wave_per_row(const double* __restrict__ cost, double wt, int RC, int C, int n, int path_cap, const int* __restrict__ cells,
                                                                      const int* __restrict__ len, double* __restrict__ total, int* __restrict__ turns, int* __restrict__ bad) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (p >= n) return;
  const int* const row = cells + (size_t)p * (size_t)path_cap;
  int at, nturns = 0;
  const double sum = cf_score_row<true>(cost, RC, C, row, len[p], path_cap, lane, at,
                                        [&](int i, int a, int dr, int dc, double w, int& turn) {
                                          if (i >= 1) {              // (a bad step before this one ends the row at that step)
                                            const int z = row[i - 1];
                                            if ((unsigned)z < (unsigned)RC) turn = (a / C - z / C != dr) || (a % C - z % C != dc);
                                          }
                                          return turn ? w + wt : w;
                                        },
                                        [&](int turn) { nturns += __builtin_popcountll(__ballot(turn)); });
  if (lane == 0) {
    total[p] = at >= 0 ? __builtin_bit_cast(double, 0x7FF8000000000000ull) : sum;
    turns[p] = at >= 0 ? 0 : nturns;
    bad[p] = at;
  }
}

}  // namespace pf
