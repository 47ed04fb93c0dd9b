// pf_turn_repair.h -- turn-field repair: the exact update of turn fields after a few cells changed (pf_turn_field_repair, DESIGN.md
// 4.23).  pf_cost_repair.h's two phases over (cell, heading) states on the turn tile (PF_TF_TW x PF_TF_TH): state words that lost
// their support are RAISED to +inf and best is rewritten, then pf_turn_field.h's relax kernel, unchanged, lowers from there.
//
// The rule.  T, best are a least fixed point of pf_turn_field.h for some map, masks and cost map; occupancy, masks and costs are the
// NEW ones and differ from the old at most on the listed cells; the policy and the turn weight wt are the ones the rows were
// computed under.  A state (v, d) is SUPPORTED when v is free and T[d][v] is 0 (e >= 1: a free source of the set, nothing else
// holds a 0), or v is free with a finite label, the move u -> v, u = v - step(d), is legal under the new mask and SOME d' gives
//     fl(T[d'][u] + e(d', d)) == T[d][v]      for u's CURRENT labels,  e = w_new for d' == d and fl(w_new + wt) otherwise
// -- w_new and fl(w_new + wt) each rounded on their own, as the relax kernel forms them, the sum never fused.  Every finite state
// on an obstacle and every unsupported finite state becomes +inf; this repeats until nothing changes.  best[v] is rewritten as the
// minimum of the states that survive: it may rise to a finite value, not only to +inf.  Then every free source takes 0 in its
// eight states and in best, and the lowering engine starts from the (set, tile) pairs that had a state word raised, that meet the
// 3 x 3 block about a listed cell or that hold a source whose nine words were not all 0.
//
// Which form of the rule the kernel evaluates: the LITERAL one, eight reads a state, everywhere.  The relax kernel's two-read
// form, fl(T[d][u] + w) == x || fl(M[u] + fl(w + wt)) == x, is not this rule in general: M[u] rises while states are raised, so
// support by M can APPEAR after it was absent (M[u] climbs to the value that happens to offer x), and the raised set would depend
// on the order of the sweeps.  The two agree at a cell whose incoming weights and masks are the old map's -- there
// x <= fl(M_old[u] + e) <= fl(M_cur[u] + e) <= fl(T[d'][u] + e), so a literal supporter forces all of them equal, and when the
// minimum is attained at d' = d the old fixed point gives x <= fl(T[d][u] + w) <= fl(M + e) -- but not inside the 3 x 3 blocks of
// the listed cells, where a weight may have fallen.  There the two DO differ: tests/turn_repair_checkers.py's two_read_case (4 x 4,
// wt = 0, integer costs) has a state at a changed cell that keeps its label by a supporter d' that is neither d nor the minimum
// of u; the literal form keeps it (18 states raised), the two-read form raises it (19) -- the same final field, another count.
// A kernel with both forms would need the listed cells' blocks as a per-cell mask in every visit; the literal form needs
// nothing and its proof below has no case distinction.  What it costs is LDS reads, and the probe says they are not what a
// repair's time is made of: a variant of the sweep that skipped every state whose u had no word raised in the sweep before (one
// 4-byte read instead of eight 8-byte ones) moved the repair's time by -15 ... +6 %, the launches and tile visits
// being the same; it was not kept.  The CPU model is the same literal form; the count of raised state words does not depend on
// the schedule and is asserted against it.
//
//   k_turn_repair_queue_changed_blocks  one thread per (listed cell, set): the (at most four) turn tiles that meet the 3 x 3 block
//                                   about the cell go on queue 0, the raise phase's first queue (tr_enqueue_block, the turn
//                                   tile's sibling of cr_enqueue_block).  Both ends of a diagonal that a closing cell makes
//                                   illegal under restrict_corner lie in the block, as does every cell with a changed weight.
//   k_turn_raise_tiles_in_lds       one workgroup per queued (set, tile): the costs of the tile and its halo pass through LDS,
//                                   w and fl(w + wt) are formed once into registers exactly as the relax kernel forms them (+inf
//                                   for a move the mask forbids and for every move into an obstacle; no cost map: ones); the
//                                   eight state planes come into LDS with a one-cell halo; finite states on obstacles are raised;
//                                   then sweeps of read / barrier / write / barrier -- a finite non-source state (v, d) with no
//                                   d' such that lt[d'][u] + e(d', d) == label is written +inf -- until one sweep raises nothing.
//                                   The raised words are stored, best is recomputed and stored where it changed, the (set,
//                                   tile)'s touched flag is set, the neighbour tiles that hold a cell with a raised state in
//                                   their halo are queued for the next launch (tq_close's side bits) and the raised words are
//                                   added to a counter of their own.  (The load and the weights repeat the relax kernel's
//                                   prologue instead of sharing it: that kernel stays as it is)
//   k_turn_repair_queue_lower       the lower phase's first queue: the touched (set, tile) pairs, the tiles of the listed cells'
//                                   blocks, and one thread per DISTINCT listed source (the host sorts each set and drops the
//                                   repeats): a free one counts for d_info[b][0], and one whose nine words are not all 0 takes 0
//                                   in all nine and puts its tile on the queue.
//
// Why the raise phase is exact (pf_tile_queue.h has the protocol's half).  (1) Words only rise, and state words only to +inf.  A
// supporter's label is strictly smaller (e >= 1), so support is well founded over STATES: the set S of states that keep their
// label -- those with a chain of supporters down to a zero on a free source -- is unique, whatever the order of the sweeps.  No
// sweep raises a state of S (induction up the chain: its supporter is in S and still holds its label), and every finite state
// outside S is raised eventually (the smallest finite label outside S has no supporter left once the sweeps stop: a supporter
// would be smaller, hence in S, hence the state itself in S).  The comparison reads u's eight state words only, never M: nothing
// it reads can come to offer a label that it did not offer before.  (2) Every label of S is the left-to-right rounded cost of a
// real walk in the NEW map that enters v by d: follow the chain down to the zero; each step (u, d') -> (v, d) is a legal move of
// the new mask and adds w_new, or fl(w_new + wt) where it turns, rounded once -- the two operations the relax kernel performs,
// never fused.  (A walk may pass a cell twice, as pf_turn_field.h's may.)  best is the minimum of such labels.  So after the
// re-seed the rows satisfy what pf_turn_field.h's points (1)-(3) ask of a start state: every stored state word is the rounded cost
// of a real walk into that state, hence >= the answer; best is the minimum of the eight; the sources hold 0.  (3) A halo word that
// the neighbour tile raises in the same launch may be read old: that can only keep a state finite one launch too long.  Whoever
// raised a state of a border cell queues the reader for the next launch, across the kernel boundary; when no tile is queued,
// every tile's last sweep saw halo words that did not change afterwards: the rows are a fixed point of the raise rule, by (1) S.
//
// Why an unqueued tile is at its fixed point when the lower phase starts: its incoming weights and masks are the old ones (it
// meets no 3 x 3 block), none of its words moved (not touched, no new seed), so every state label is still the minimum it was --
// the labels around it only rose or stayed -- and still attained, by its supporter; its best words are the minima they were.
// Tiles whose halo changes later are queued by whoever lowers the halo word.
//
// Bounds.  A raise launch with a non-empty queue either raises a state word or is the last but one; at most 8 R C state words are
// raised per set and a launch serves all sets: at most 8 R C + 1 raise rounds, and the lower phase has pf_turn_field.h's bound.
// Every sweep but a visit's last raises at least one of the tile's 8 PF_TF_TW PF_TF_TH state words, so a sweep count of
// PF_TF_SWEEP_BOUND cannot be reached: the loop stops there and raises the error word.  Either way the call fails with a message
// and never spins.
#pragma once

namespace pf {

// the TW x TH tiles that meet the 3 x 3 block about cell x go on the queue, for set b
template <int TW, int TH>
__device__ __forceinline__ void tr_enqueue_block(int x, int b, int R, int C, int tiles_x, int ntiles, int* __restrict__ flag, int* __restrict__ queue,
                                                 int* __restrict__ count) {
  const int r = x / C, c = x - r * C;
  const int ty0 = (r > 0 ? r - 1 : 0) / TH, ty1 = (r + 1 < R ? r + 1 : R - 1) / TH;
  const int tx0 = (c > 0 ? c - 1 : 0) / TW, tx1 = (c + 1 < C ? c + 1 : C - 1) / TW;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) tq_enqueue(b * ntiles + ty * tiles_x + tx, flag, queue, count);
}

__global__ __launch_bounds__(PF_TF_THREADS) void k_turn_repair_queue_changed_blocks(int R, int C, int tiles_x, int ntiles, int B, int n_changed,
                                                                                      const int* __restrict__ changed, int* __restrict__ flag,
                                                                                      int* __restrict__ queue, int* __restrict__ count) {
  const int RC = R * C;
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y)
    for (int i = (int)(blockIdx.x * PF_TF_THREADS + threadIdx.x); i < n_changed; i += (int)(gridDim.x * PF_TF_THREADS)) {
      const int x = changed[i];
      if ((unsigned)x < (unsigned)RC) tr_enqueue_block<PF_TF_TW, PF_TF_TH>(x, b, R, C, tiles_x, ntiles, flag, queue, count);   // (the host has checked the ids)
    }
}

// words[0] += the state words raised; words[1] = 1 when a tile hit the sweep bound
__global__ __launch_bounds__(PF_TF_THREADS) void k_turn_raise_tiles_in_lds(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, const double* __restrict__ cost, double wt,
                                                                             int R, int C, int allow_diag, int tiles_x, int tiles_y, double* d_states, double* d_best,
                                                                             const int* __restrict__ queue, int nqueue, int* flag_now, int* count_now, int* flag_next,
                                                                             int* __restrict__ queue_next, int* count_next, int* __restrict__ touched,
                                                                             unsigned long long* __restrict__ words) {
  constexpr int PER = PF_TF_PER, LW = PF_TF_LW, LN = PF_TF_LW * PF_TF_LH;
  __shared__ double lt[8][LN];                                       // planes 0..7: T[d] (and, before the labels come, plane 0 holds the costs)
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
    lt[0][i] = cv;
  }
  __syncthreads();
  int li[PER];
  double w[PER][8], wturn[PER][8];
  bool open[PER];                                                    // a free cell inside the grid
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_TF_THREADS, lr = i / PF_TF_TW, lcn = i % PF_TF_TW;
    li[j] = (lr + 1) * LW + lcn + 1;
    const int l = li[j];
    const int r = r0 + lr, c = c0 + lcn;
    unsigned m = 0u;                                                 // beyond the grid or on an obstacle: nothing arrives, no supporter
    open[j] = false;
    if (r < R && c < C) { const size_t v = (size_t)r * (size_t)C + (size_t)c; open[j] = occ[v] != 1; m = open[j] ? mm[v] : 0u; }
    const double cv = lt[0][l];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                    // u = v - step(k) moves into v by move k: bit opp(k) of v's own byte
      const int opp = k < 4 ? (k ^ 1) : 11 - k;
      const double cu = lt[0][l - (move_dr(k) * LW + move_dc(k))];
      w[j][k] = ((m >> opp) & 1u) ? cf_weight(cu, cv, k) : inf;
      wturn[j][k] = w[j][k] + wt;
    }
  }
  __syncthreads();                                                   // the costs are in registers: plane 0 takes its labels
  for (int i = tid; i < LN; i += PF_TF_THREADS) {
    const int r = r0 + i / LW - 1, c = c0 + i % LW - 1;
    const bool in = r >= 0 && r < R && c >= 0 && c < C;
    const size_t v = in ? (size_t)r * (size_t)C + (size_t)c : 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) lt[d][i] = in ? cf_load(T + (size_t)d * RC + v) : inf;
  }
  __syncthreads();
  double cur[PER][8], oldm[PER];
  unsigned rose[PER];                                                // bits 0..7: the states raised in this visit
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    double least = inf;
    rose[j] = 0u;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      cur[j][d] = lt[d][li[j]];
      least = cur[j][d] < least ? cur[j][d] : least;
      if (!open[j] && __builtin_bit_cast(unsigned long long, cur[j][d]) < PF_DF_INF_BITS) {   // a finite state on an obstacle (beyond the grid every word is +inf)
        cur[j][d] = inf; lt[d][li[j]] = inf; rose[j] |= 1u << d;     // (this thread's own word: nobody reads it before the barrier)
      }
    }
    oldm[j] = least;
  }
  __syncthreads();
  int sweeps = 0, stuck = 0;
  for (;;) {
    unsigned up[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int l = li[j];
      up[j] = 0u;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const double x = cur[j][d];
        const unsigned long long bits = __builtin_bit_cast(unsigned long long, x);
        if (bits >= PF_DF_INF_BITS || (bits == 0ull && open[j])) continue;   // +inf has nothing to lose (a NaN or a negative word of a caller out of contract: left alone); a zero on a free cell is a source
        const int lu = l - (move_dr(d) * LW + move_dc(d));
        bool held = false;
#pragma unroll
        for (int k = 0; k < 8; ++k) held = held || (lt[k][lu] + (k == d ? w[j][d] : wturn[j][d]) == x);   // (on an obstacle every weight is +inf: no sum equals a finite label)
        if (!held) up[j] |= 1u << d;
      }
    }
    __syncthreads();                                                 // every read of this sweep is done: now the writes
    int changed = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (!up[j]) continue;
      changed = 1;
      rose[j] |= up[j];
#pragma unroll
      for (int d = 0; d < 8; ++d)
        if ((up[j] >> d) & 1u) { cur[j][d] = inf; lt[d][li[j]] = inf; }
    }
    sweeps += 1;
    if (!__syncthreads_or(changed)) break;
    if (sweeps >= PF_TF_SWEEP_BOUND) { stuck = 1; break; }           // (uniform: cannot happen, see the header)
  }
  int sides = 0, raised = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (!rose[j]) continue;
    const int i = tid + j * PF_TF_THREADS, lr = i / PF_TF_TW, lcn = i % PF_TF_TW;
    const size_t v = (size_t)(r0 + lr) * (size_t)C + (size_t)(c0 + lcn);   // (a raised word was finite: a cell inside the grid)
    double least = inf;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      if ((rose[j] >> d) & 1u) cf_store(T + (size_t)d * RC + v, inf);
      least = cur[j][d] < least ? cur[j][d] : least;
    }
    if (__builtin_bit_cast(unsigned long long, least) != __builtin_bit_cast(unsigned long long, oldm[j])) cf_store(Mg + v, least);
    raised += __builtin_popcount(rose[j]);
    sides |= tq_side_bits<PF_TF_TW, PF_TF_TH>(lr, lcn);
  }
  tq_close(visit, sides, raised, allow_diag, tiles_x, tiles_y, flag_next, queue_next, count_next, words);
  if (tid == 0 && tq_lds().moved) touched[visit.q] = 1;              // (after tq_close's barrier; read by a later kernel only)
  if (tid == 0 && stuck) words[1] = 1ull;
}

// The lower phase's first queue (queue 0) and the sources that count.  reseed == 0: count only, nothing is written but nsrc.
__global__ __launch_bounds__(PF_TF_THREADS) void k_turn_repair_queue_lower(const uint8_t* __restrict__ occ, int R, int C, int tiles_x, int ntiles, int B, int T,
                                                                             const int* __restrict__ touched, int n_changed, const int* __restrict__ changed,
                                                                             const int* __restrict__ off, const int* __restrict__ src, int reseed,
                                                                             double* __restrict__ states, double* __restrict__ best, int* __restrict__ flag,
                                                                             int* __restrict__ queue, int* __restrict__ count, unsigned long long* __restrict__ nsrc) {
  const int RC = R * C;
  const int t0 = (int)(blockIdx.x * PF_TF_THREADS + threadIdx.x), step = (int)(gridDim.x * PF_TF_THREADS);
  if (reseed && blockIdx.y == 0)
    for (int q = t0; q < T; q += step)
      if (touched[q]) tq_enqueue(q, flag, queue, count);
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    if (reseed)
      for (int i = t0; i < n_changed; i += step) {
        const int x = changed[i];
        if ((unsigned)x < (unsigned)RC) tr_enqueue_block<PF_TF_TW, PF_TF_TH>(x, b, R, C, tiles_x, ntiles, flag, queue, count);
      }
    const int end = off[b + 1];
    int counted = 0;
    for (int j = off[b] + t0; j < end; j += step) {                  // (distinct within the set: the host's doing)
      const int s = src[j];
      if ((unsigned)s >= (unsigned)RC || occ[s] == 1) continue;      // a source ON an obstacle is no source
      counted += 1;
      if (!reseed) continue;
      double* const bword = best + (size_t)b * (size_t)RC + (size_t)s;
      double* const sword = states + (size_t)b * 8 * (size_t)RC + (size_t)s;
      unsigned long long any = __builtin_bit_cast(unsigned long long, cf_load(bword));
#pragma unroll
      for (int d = 0; d < 8; ++d) any |= __builtin_bit_cast(unsigned long long, cf_load(sword + (size_t)d * (size_t)RC));
      if (any == 0ull) continue;
#pragma unroll
      for (int d = 0; d < 8; ++d) cf_store(sword + (size_t)d * (size_t)RC, 0.0);
      cf_store(bword, 0.0);
      const int r = s / C, c = s - r * C;
      tq_enqueue(b * ntiles + (r / PF_TF_TH) * tiles_x + c / PF_TF_TW, flag, queue, count);
    }
    if (counted) atomicAdd(nsrc + b, (unsigned long long)counted);
  }
}

}  // namespace pf
