// pf_dist_field.h -- exact one-to-all path lengths from K source cells or sets (pf_dist_field_batch / _merged): dijkstra.py's
// relaxation with no target, WITHOUT the pop order.
//
// Why this is exact.  The table dijkstra_host builds is the least fixed point of
//     D[src] = 0,   D[v] = min over legal moves u -> v of fl(D[u] + w),   w = 1 (k < 4) or PF_SQRT2,
// and any label-correcting schedule reaches it bit for bit (fl(. + w) is monotone: the argument at the top of pf_settle.h).
// Every weight is >= 1, so unit-width buckets need no inner iteration: if fl(D[u] + w) = D[v] lies in [i, i + 1) then
// D[u] < i (had D[u] >= i the rounded sum would be >= i + 1, which is representable, and rounding is monotone).  Once all
// buckets below i have been relaxed every cell whose label lies in bucket i = (int)D is final, and level i relaxes the cells
// of bucket i in any order, in parallel, into buckets i + 1 and i + 2 (D[u] < i + 1 and w < 1.4143: never i + 3).
//
// Mapping.  One workgroup per source set; gridDim.x workgroups loop over the sets b, b + gridDim.x, ...  Labels are
// non-negative doubles, so their bit patterns order as unsigned 64-bit integers: ONE atomicMin on the label word of the output
// row compares and updates, +inf is the initial value.  The thread whose atomic returns an old value of ANOTHER bucket than
// its new one appends the cell to the new bucket's list (exactly one thread sees each transition).  A label only falls, so a
// cell enters a given bucket at most once: a list never holds more than RC entries, and a cell is appended at most twice
// (first reached from level i in i + 1 or i + 2, improved at most into i + 1).  An entry whose label has left the level's
// bucket is stale and skipped.  Three rolling lists of RC cells per workgroup live in HBM (the handle's slots); their fill
// counts live in LDS, four rolling words so that the count of bucket i - 1 is cleared during level i, when nobody reads or
// appends to it: one workgroup barrier per level.  Eight lanes share a list entry, one move each: the eight offers of a
// cell leave in one instruction and a level's chain is list entry -> label and mask -> atomic -> append.  Measured
// (DESIGN.md 4.11): 1024 threads beat 512 and 256, eight lanes per entry beat one lane making the eight offers, and reading
// the neighbour's label first to save the atomics that lose costs more than they do (PF_DF_THREADS / _LANES / _PREFILTER).
//
// Visibility.  The row is touched by ONE workgroup.  The atomics execute in L2, so every read of a label is an agent-scope
// relaxed atomic load (a plain load may hit a line this CU's L1 holds from before the atomic); the +inf fill is plain
// stores drained by an agent-scope release fence in front of the first barrier.  List entries are plain stores read by the
// same workgroup after the level's barrier.
//
// Cost.  Time is proportional to the number of levels, floor(largest finite label) + 1, each at least a barrier and three
// dependent memory round trips: a serpentine map serialises into about RC / 2 levels.
#pragma once

namespace pf {

#ifndef PF_DF_THREADS
#define PF_DF_THREADS 1024                      /* workgroup size: 128 list entries per pass, eight lanes each */
#endif
#ifndef PF_DF_LANES
#define PF_DF_LANES 8                           /* lanes that share a list entry: 8 (one move each) or 1 (all eight moves) */
#endif
#ifndef PF_DF_PREFILTER
#define PF_DF_PREFILTER 0                       /* 1: read the neighbour's label before offering; measured slower */
#endif
#define PF_DF_INF_BITS 0x7FF0000000000000ull
#define PF_DF_ERR_LEVELS 1                      /* *err: the level counter passed 2 RC + 4 (no finite label exceeds sqrt(2) RC) */
#define PF_DF_ERR_LIST 2                        /* *err: a list was offered more than RC entries */

// one offer: fl(du + w) to the neighbour of u across move k; the thread that sees v enter a bucket appends it
PF_DEV void df_offer(unsigned long long* D, int* L, int* cnt, int* err, int RC, int C, int u, double du, int k, unsigned& n_set, unsigned& n_off,
                     unsigned& n_app) {
  const int v = u + move_dr(k) * C + move_dc(k);
  const double t = du + (k < 4 ? 1.0 : PF_SQRT2);
  const unsigned long long tb = __builtin_bit_cast(unsigned long long, t);
  n_off += 1;
#if PF_DF_PREFILTER
  if (tb >= __hip_atomic_load(&D[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
#endif
  const unsigned long long old = __hip_atomic_fetch_min(&D[v], tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tb >= old) return;
  const int nb = (int)t;                                             // the level + 1 or + 2
  const bool fresh = old == PF_DF_INF_BITS;
  n_set += fresh ? 1u : 0u;
  if (fresh || (int)__builtin_bit_cast(double, old) != nb) {         // the one thread that sees v enter bucket nb
    const int at = __hip_atomic_fetch_add(&cnt[nb & 3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (at < RC) L[(size_t)(nb % 3) * (size_t)RC + (size_t)at] = v;
    else *err = PF_DF_ERR_LIST;                                      // (cannot happen: a cell enters a bucket once)
    n_app += 1;
  }
}

// The one level-synchronous kernel: row b is the field of source set b, sets (device) = {off[B + 1], ids[off[B]]}; a single source
// is a set of one (pf_dist_field_batch uploads off = 0..K).  Seeding: after the +inf fill, the release fence and the barrier the
// threads stride over the set's sources, skip those on an obstacle and make one agent-scope atomic min of 0 on the label; the
// thread that saw +inf appends the cell to list 0, so a source listed twice enters once, and a set with no free source leaves a
// +inf row.  Why a seed of several cells is as exact as a seed of one: pf_nearest_field.h.
// info (or null): int64 [B][4] = {levels that held a live cell, cells with a finite label, relaxations offered, list appends}, the
// seeds counting as cells reached and as appends
__global__ __launch_bounds__(PF_DF_THREADS) void k_dist_field_merged_source_sets(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, int RC, int C, int B,
                                                                                      const int* __restrict__ off, const int* __restrict__ src, double* out, int* lists,
                                                                                      long long* info, int* err) {
  __shared__ int cnt[4], live[4];
  __shared__ unsigned long long acc[3];
  const int tid = (int)threadIdx.x, sub = tid % PF_DF_LANES, grp = tid / PF_DF_LANES;
  int* const L = lists + (size_t)blockIdx.x * 3 * (size_t)RC;
  const int bound = 2 * RC + 4;                                      // (RC <= 2^24)
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    unsigned long long* const D = (unsigned long long*)(out + (size_t)b * (size_t)RC);
    if (tid == 0) { for (int i = 0; i < 4; ++i) { cnt[i] = 0; live[i] = 0; } acc[0] = acc[1] = acc[2] = 0ull; }
    for (int i = tid; i < RC; i += PF_DF_THREADS) D[i] = PF_DF_INF_BITS;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");               // the fill is in L2 before the first atomic lands there
    __syncthreads();
    unsigned n_set = 0, n_off = 0, n_app = 0;
    const int hi = off[b + 1];
    for (int j = off[b] + tid; j < hi; j += PF_DF_THREADS) {         // the seeds: bucket 0
      const int s = src[j];
      if (occ[s] == 1) continue;                                     // a source ON an obstacle is no source
      if (__hip_atomic_fetch_min(&D[s], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != PF_DF_INF_BITS) continue;   // listed before
      const int at = __hip_atomic_fetch_add(&cnt[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (at < RC) L[at] = s;
      else *err = PF_DF_ERR_LIST;                                    // (cannot happen: a cell enters once)
      n_set += 1; n_app += 1;
    }
    int levels = 0;                                                  // (thread 0's)
    for (int lv = 0;; ++lv) {
      __syncthreads();                                               // the appends and the label stores of level lv - 1 are done
      const int cur = lv & 3;
      const int n = cnt[cur];
      const int waiting = n + cnt[(lv + 1) & 3] + cnt[(lv + 2) & 3];
      if (tid == 0) { levels += live[(lv + 3) & 3]; live[(lv + 3) & 3] = 0; cnt[(lv + 3) & 3] = 0; }   // bucket lv - 1 is history
      if (waiting == 0) break;
      if (lv > bound) { if (tid == 0) *err = PF_DF_ERR_LEVELS; break; }
      const int* const Lc = L + (size_t)(lv % 3) * (size_t)RC;
      for (int e = grp; e < n; e += PF_DF_THREADS / PF_DF_LANES) {
        const int u = Lc[e];
        const double du = __builtin_bit_cast(double, __hip_atomic_load(&D[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if ((int)du != lv) continue;                                 // stale: improved into bucket lv - 1 and relaxed there
        if (sub == 0) live[cur] = 1;
        const unsigned m = mm[u];
#if PF_DF_LANES == 8
        if ((m >> sub) & 1u) df_offer(D, L, cnt, err, RC, C, u, du, sub, n_set, n_off, n_app);
#else
#pragma unroll
        for (int mv = 0; mv < 8; ++mv)
          if ((m >> mv) & 1u) df_offer(D, L, cnt, err, RC, C, u, du, mv, n_set, n_off, n_app);
#endif
      }
    }
    if (info) {
      if (n_set) __hip_atomic_fetch_add(&acc[0], (unsigned long long)n_set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (n_off) __hip_atomic_fetch_add(&acc[1], (unsigned long long)n_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (n_app) __hip_atomic_fetch_add(&acc[2], (unsigned long long)n_app, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (tid == 0 && info) {
      long long* o = info + 4 * (size_t)b;
      o[0] = levels; o[1] = (long long)acc[0]; o[2] = (long long)acc[1]; o[3] = (long long)acc[2];
    }
  }
}

}  // namespace pf
