// pf_cost_repair.h -- cost-field repair: the exact update of cost fields after a few cells changed (pf_cost_field_repair, DESIGN.md
// 4.22).  Two phases on the tile-queue engine over the tile of pf_widest.h: labels that lost their support are RAISED to +inf, then
// pf_cost_field.h's relax kernel lowers from there.  The work follows the tiles the invalid region crosses, not the map.
//
// The rule.  D is a least fixed point of pf_cost_field.h for some map, masks and cost map; occupancy, masks and costs are the NEW
// ones and differ from the old at most on the listed cells.  A cell v is SUPPORTED when it is free and holds 0 (weights >= 1: the
// free sources of its set and nothing else), or is free with a finite label and some u has a legal move u -> v under the new
// mask with fl(D[u] + w_new(u, v)) == D[v] for u's CURRENT label.  A finite label on an obstacle, and every unsupported finite
// label, becomes +inf; this repeats until nothing changes.  Then every free source of the set takes 0 (one that was an obstacle
// before), and the lowering engine starts from the tiles that had a word raised, that meet the 3 x 3 block about a listed cell or
// that hold a re-seeded source.
//
//   k_repair_queue_changed_blocks   one thread per (listed cell, set): the (at most four) tiles that meet the 3 x 3 block about
//                                   the cell go on queue 0 -- the raise phase's first queue.  A closing cell also makes the
//                                   diagonals that pass it illegal under restrict_corner; both ends of such a move lie in the
//                                   block, as does every cell with a changed incoming weight.
//   k_cost_raise_tiles_in_lds       one workgroup per queued (set, tile): loads D and c with a one-cell halo into LDS, forms the
//                                   eight incoming weights of its cells once into registers as the relax kernel does (+inf for a
//                                   move the mask forbids and for every move into an obstacle), raises the finite labels on its
//                                   obstacles, then sweeps read / barrier / write / barrier: a cell with a finite non-zero label
//                                   and no u with ld[u] + w == label is written +inf -- until one sweep raises nothing.  It
//                                   stores the raised words, sets the (set, tile)'s touched flag and queues, for the next
//                                   launch, the neighbour tiles that hold a raised cell in their halo (tq_close's side bits).
//                                   (The load and the weights repeat the relax kernel's prologue instead of sharing it: that
//                                   kernel stays as it is, its time depends on the order of its prologue)
//   k_repair_queue_lower            the lower phase's first queue: the touched (set, tile) pairs, the tiles of the listed cells'
//                                   blocks, and one thread per DISTINCT listed source (the host sorts each set and drops the
//                                   repeats): a free one counts for d_info[b][0] -- a fresh call's count; the seed kernel's rule
//                                   "found +inf" does not apply, the label may be 0 already -- and one whose label is not 0 takes
//                                   0 and puts its tile on the queue.
//
// Why the raise phase is exact (the half of the argument that is this file's; pf_tile_queue.h has the protocol's).  (1) Words only
// rise, and only to +inf.  A supporter's label is strictly smaller (w >= 1), so support is well founded: the set S of cells that
// keep their label -- those with a chain of supporters down to a free zero -- is unique, whatever the order of the sweeps.  No
// sweep raises a cell of S (induction up the chain: its supporter is in S and still holds its label), and every finite cell
// outside S is raised eventually (the smallest finite label outside S has no supporter left once the sweeps stop).  (2) Every
// label of S is the left-to-right rounded cost of a real walk in the NEW map: follow the chain down to the zero; each step is a
// legal move of the new mask and adds the new weight, rounded once -- the comparison is one rounded addition of a weight that
// was rounded on its own, the same two operations the relax kernel performs, never fused.  So after the re-seed the rows satisfy
// what pf_cost_field.h's points (1)-(3) ask of a start state: every stored label is the rounded cost of a real walk, hence >= the
// answer, and the sources hold 0.  (3) A halo word that the neighbour tile raises in the same launch may be read old: that can
// only keep a cell finite one launch too long.  Whoever raised the word queues the reader for the next launch, across the kernel
// boundary, as in the lowering engine; when no tile is queued, every tile's last sweep saw halo words that did not change
// afterwards: the whole row is a fixed point of the raise rule, which by (1) is S.  Old parent maps and old costs are not needed.
//
// Why an unqueued tile is at its fixed point when the lower phase starts: its incoming weights and masks are the old ones (it
// meets no 3 x 3 block), none of its words moved (not touched, no new seed), so every label is still the minimum it was -- the
// labels around it only rose or stayed -- and still attained, by its supporter.  Tiles whose halo changes later are queued by
// whoever lowers the halo word.
//
// Rounds.  A raise launch with a non-empty queue either raises a word or is the last but one: a tile is queued by a raised halo
// word or by the first queue.  At most R C words are raised per set, a launch serves all sets: at most R C + 1 raise rounds, and
// the lower phase has pf_cost_field.h's bound.  The sweeps inside a visit raise at least one of the tile's 1024 words each.
#pragma once

namespace pf {

// the tiles that meet the 3 x 3 block about cell x go on the queue, for set b
__device__ __forceinline__ void cr_enqueue_block(int x, int b, int R, int C, int tiles_x, int ntiles, int* __restrict__ flag, int* __restrict__ queue,
                                                 int* __restrict__ count) {
  const int r = x / C, c = x - r * C;
  const int ty0 = (r > 0 ? r - 1 : 0) / PF_WD_TH, ty1 = (r + 1 < R ? r + 1 : R - 1) / PF_WD_TH;
  const int tx0 = (c > 0 ? c - 1 : 0) / PF_WD_TW, tx1 = (c + 1 < C ? c + 1 : C - 1) / PF_WD_TW;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) tq_enqueue(b * ntiles + ty * tiles_x + tx, flag, queue, count);
}

__global__ __launch_bounds__(PF_CF_THREADS) void k_repair_queue_changed_blocks(int R, int C, int tiles_x, int ntiles, int B, int n_changed, const int* __restrict__ changed,
                                                                                 int* __restrict__ flag, int* __restrict__ queue, int* __restrict__ count) {
  const int RC = R * C;
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y)
    for (int i = (int)(blockIdx.x * PF_CF_THREADS + threadIdx.x); i < n_changed; i += (int)(gridDim.x * PF_CF_THREADS)) {
      const int x = changed[i];
      if ((unsigned)x < (unsigned)RC) cr_enqueue_block(x, b, R, C, tiles_x, ntiles, flag, queue, count);   // (the host has checked the ids)
    }
}

__global__ __launch_bounds__(PF_CF_THREADS) void k_cost_raise_tiles_in_lds(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, const double* __restrict__ cost, int R, int C, int allow_diag,
                                                                             int tiles_x, int tiles_y, double* d_rows, const int* __restrict__ queue, int nqueue,
                                                                             int* flag_now, int* count_now, int* flag_next, int* __restrict__ queue_next, int* count_next,
                                                                             int* __restrict__ touched, unsigned long long* __restrict__ raised_total) {
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
  double w[PER][8], cur[PER];
  bool was[PER], open[PER];                                          // the word was finite when the visit began; a free cell inside the grid
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_CF_THREADS, lr = i / PF_WD_TW, lcn = i % PF_WD_TW;
    li[j] = (lr + 1) * LW + lcn + 1;
    const int l = li[j];
    const int r = r0 + lr, c = c0 + lcn;
    unsigned m = 0u;                                                 // beyond the grid or on an obstacle: nothing arrives, no supporter
    open[j] = false;
    if (r < R && c < C) { const size_t v = (size_t)r * (size_t)C + (size_t)c; open[j] = occ[v] != 1; m = open[j] ? mm[v] : 0u; }
    const double cv = lc[l];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                    // u = v - step(k) moves into v by move k: bit opp(k) of v's own byte
      const int opp = k < 4 ? (k ^ 1) : 11 - k;
      const double cu = lc[l - (move_dr(k) * LW + move_dc(k))];
      w[j][k] = ((m >> opp) & 1u) ? cf_weight(cu, cv, k) : inf;
    }
    cur[j] = ld[l];
    was[j] = __builtin_bit_cast(unsigned long long, cur[j]) < PF_DF_INF_BITS;   // (a NaN or a negative word of a caller out of contract: left alone)
  }
  int changed;
  do {
    changed = 0;
    bool up[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int l = li[j];
      const unsigned long long bits = __builtin_bit_cast(unsigned long long, cur[j]);
      bool held = (bits == 0ull && open[j]) || bits >= PF_DF_INF_BITS;   // a zero on a free cell is a source; +inf has nothing to lose
#pragma unroll
      for (int k = 0; k < 8; ++k)                                    // (on an obstacle every weight is +inf: no sum equals a finite label)
        held = held || (ld[l - (move_dr(k) * LW + move_dc(k))] + w[j][k] == cur[j]);
      up[j] = !held;
    }
    __syncthreads();                                                 // every read of this sweep is done: now the writes
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (up[j]) { cur[j] = inf; ld[li[j]] = inf; changed = 1; }
  } while (__syncthreads_or(changed));
  int sides = 0, raised = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (!was[j] || cur[j] != inf) continue;
    const int i = tid + j * PF_CF_THREADS, lr = i / PF_WD_TW, lcn = i % PF_WD_TW;
    cf_store(D + (size_t)(r0 + lr) * (size_t)C + (size_t)(c0 + lcn), inf);   // (was finite: a cell inside the grid)
    raised += 1;
    sides |= tq_side_bits<PF_WD_TW, PF_WD_TH>(lr, lcn);
  }
  tq_close(visit, sides, raised, allow_diag, tiles_x, tiles_y, flag_next, queue_next, count_next, raised_total);
  if (tid == 0 && tq_lds().moved) touched[visit.q] = 1;              // (after tq_close's barrier; read by a later kernel only)
}

// The lower phase's first queue (queue 0) and the sources that count.  reseed == 0: count only, nothing is written but nsrc.
__global__ __launch_bounds__(PF_CF_THREADS) void k_repair_queue_lower(const uint8_t* __restrict__ occ, int R, int C, int tiles_x, int ntiles, int B, int T,
                                                                        const int* __restrict__ touched, int n_changed, const int* __restrict__ changed,
                                                                        const int* __restrict__ off, const int* __restrict__ src, int reseed, double* __restrict__ rows,
                                                                        int* __restrict__ flag, int* __restrict__ queue, int* __restrict__ count,
                                                                        unsigned long long* __restrict__ nsrc) {
  const int RC = R * C;
  const int t0 = (int)(blockIdx.x * PF_CF_THREADS + threadIdx.x), step = (int)(gridDim.x * PF_CF_THREADS);
  if (reseed && blockIdx.y == 0)
    for (int q = t0; q < T; q += step)
      if (touched[q]) tq_enqueue(q, flag, queue, count);
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    if (reseed)
      for (int i = t0; i < n_changed; i += step) {
        const int x = changed[i];
        if ((unsigned)x < (unsigned)RC) cr_enqueue_block(x, b, R, C, tiles_x, ntiles, flag, queue, count);
      }
    const int end = off[b + 1];
    int counted = 0;
    for (int j = off[b] + t0; j < end; j += step) {                  // (distinct within the set: the host's doing)
      const int s = src[j];
      if ((unsigned)s >= (unsigned)RC || occ[s] == 1) continue;      // a source ON an obstacle is no source
      counted += 1;
      if (!reseed) continue;
      double* const word = rows + (size_t)b * (size_t)RC + (size_t)s;
      if (__builtin_bit_cast(unsigned long long, cf_load(word)) == 0ull) continue;
      cf_store(word, 0.0);
      const int r = s / C, c = s - r * C;
      tq_enqueue(b * ntiles + (r / PF_WD_TH) * tiles_x + c / PF_WD_TW, flag, queue, count);
    }
    if (counted) atomicAdd(nsrc + b, (unsigned long long)counted);
  }
}

}  // namespace pf
