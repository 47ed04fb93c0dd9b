// pf_nearest_field.h -- nearest-source fields: ONE field seeded with a whole source set, and the owner of every cell
// (pf_dist_field_merged, pf_dist_field_owners).
//
// Why the merged field is exact.  The table is the least fixed point of
//     D[s] = 0 for every free source s of the set,   D[v] = min over legal moves u -> v of fl(D[u] + w)   otherwise,
// which any label-correcting schedule reaches bit for bit (fl(. + w) is monotone: pf_settle.h).  A chain of fl(. + w) that starts
// at 0 in one source is a chain of that source's own field, so the fixed point is the elementwise minimum of the single-source
// fields.  Nothing in pf_dist_field.h's bucket argument needs ONE cell of label 0: every weight is >= 1, so a label of bucket
// i is set from a bucket below i, and level i relaxes bucket i into i + 1 and i + 2.  k_dist_field_merged_source_sets
// is that kernel with another seeding step: after the +inf fill, the release fence and the barrier the threads stride over the
// set's sources, skip those on an obstacle and make one agent-scope atomic min of 0 on the label; the thread that saw +inf
// appends the cell to list 0, so a source listed twice enters once.  One workgroup per set on the handle's list slots; a row and
// a slot belong to one workgroup; labels are read with agent-scope relaxed atomic loads.
//
// Owners.  pf_dist_field_parents turns the merged rows into parent maps (every D == 0 cell gets code 8): a forest, one tree
// per free source cell, and the tree a cell hangs in is the tree a dijkstra.py-shaped search seeded with the whole set leaves
// (the pop order is the order of (D[v], v) whatever the number of seeds: pf_field_paths.h).  The owner of a cell is the root
// of its chain, NOT the lowest index among the sources at the same distance.  The roots are found by pointer doubling between
// two int32 [B][RC] buffers, one launch per round, kernel boundaries the only synchronisation:
//     k_nearest_owner_links   word = the parent's cell id (0 <= id < RC, checked against the grid's edges),
//                                          PF_NF_NONE for code 255, PF_NF_ROOT for code 8; any other byte raises the error word
//     k_nearest_owner_stamp_ranks   every source whose cell is a root: atomic max of -(index in its set) - 2 on the
//                                          root's word -- the LOWEST index of a cell listed more than once wins
//     k_nearest_owner_doubling     next[v] = cur[v] if negative (resolved), else cur[cur[v]]: a resolved cell hands its
//                                          rank on, an unresolved one doubles its stride.  After round t every cell at most
//                                          2^t - 1 steps from its root is resolved: ceil(log2(n)) rounds for chains of n cells
//     k_nearest_owner_write_and_count      owner = -word - 2, -1 for PF_NF_NONE; a word that is still a cell id (a chain longer
//                                          than the bound: a cycle, or a d_info of another field) or a root that no source
//                                          names raises the error word and writes -1.  Counts: one 64-bit integer atomic per
//                                          run of neighbouring lanes of a wavefront that share an owner.
// Every id a word can hold was range-checked when it was written, so no round reads out of range whatever bytes the map holds.
#pragma once

namespace pf {

#define PF_NF_THREADS 256                       /* owner kernels: cells per workgroup */
#define PF_NF_NONE (-1)                         /* link word: an obstacle / a cell out of reach */
#define PF_NF_ROOT ((int)0x80000000)            /* link word: a root no source has claimed yet */
#define PF_NF_ERR_CODE 4                        /* *err: a parent code outside 0..8 and 255, or a step off the grid */
#define PF_NF_ERR_CHAIN 8                       /* *err: a chain longer than the bound */
#define PF_NF_ERR_ROOT 16                       /* *err: a root that is no source of its set */

// sets (device): {off[B + 1], ids[off[B]]}; info (or null): int64 [B][4] as k_dist_field_level_synchronous's, the seeds
// counting as cells reached and as appends
template <int PF_LATE = 0>
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

PF_DEV void nf_raise(int* err, int bit) { __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // (the kinds add up)

template <int PF_LATE = 0>
__global__ __launch_bounds__(PF_NF_THREADS) void k_nearest_owner_links(const uint8_t* __restrict__ parents, int RC, int C, int B, int* __restrict__ link,
                                                                                   int* err) {
  const int v = (int)blockIdx.x * PF_NF_THREADS + (int)threadIdx.x;
  if (v >= RC) return;
  const int r = v / C, c = v - r * C, R = RC / C;
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const unsigned code = parents[(size_t)b * (size_t)RC + (size_t)v];
    int w = PF_NF_NONE;
    if (code == PF_FP_SOURCE) w = PF_NF_ROOT;
    else if (code < 8u) {
      const int pr = r - move_dr((int)code), pc = c - move_dc((int)code);
      if (pr >= 0 && pr < R && pc >= 0 && pc < C) w = pr * C + pc;
      else nf_raise(err, PF_NF_ERR_CODE);
    } else if (code != PF_FP_NONE) nf_raise(err, PF_NF_ERR_CODE);
    link[(size_t)b * (size_t)RC + (size_t)v] = w;
  }
}

// sets: {off[B + 1], ids[off[B]]}, every id inside [0, RC) (checked on the host)
template <int PF_LATE = 0>
__global__ __launch_bounds__(PF_NF_THREADS) void k_nearest_owner_stamp_ranks(int RC, int B, const int* __restrict__ off, const int* __restrict__ src, int* link) {
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const int lo = off[b], hi = off[b + 1];
    int* const Lk = link + (size_t)b * (size_t)RC;
    for (int j = lo + (int)blockIdx.x * PF_NF_THREADS + (int)threadIdx.x; j < hi; j += (int)gridDim.x * PF_NF_THREADS) {
      const int s = src[j];
      if (Lk[s] >= PF_NF_NONE) continue;                             // no root: an obstacle, or a map of another set (ROOT and ranks lie below)
      __hip_atomic_fetch_max(&Lk[s], -(j - lo) - 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int PF_LATE = 0>
__global__ __launch_bounds__(PF_NF_THREADS) void k_nearest_owner_doubling(int RC, int B, const int* __restrict__ cur, int* __restrict__ next) {
  const int v = (int)blockIdx.x * PF_NF_THREADS + (int)threadIdx.x;
  if (v >= RC) return;
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const int* const P = cur + (size_t)b * (size_t)RC;
    int p = P[v];
    if (p >= 0) p = P[p];                                            // (p was range-checked when it was written)
    next[(size_t)b * (size_t)RC + (size_t)v] = p;
  }
}

// count (or null): int64 [off[B]], zeroed by the caller
template <int PF_LATE = 0>
__global__ __launch_bounds__(PF_NF_THREADS) void k_nearest_owner_write_and_count(int RC, int B, const int* __restrict__ off, const int* __restrict__ link,
                                                                                int* __restrict__ owner, unsigned long long* count, int* err) {
  const int v = (int)blockIdx.x * PF_NF_THREADS + (int)threadIdx.x;
  const bool inside = v < RC;                                        // (no early return: the whole wavefront takes part in the ballot below)
  const unsigned lane = __lane_id();
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    int o = -1;
    if (inside) {
      const int w = link[(size_t)b * (size_t)RC + (size_t)v];
      if (w >= 0) nf_raise(err, PF_NF_ERR_CHAIN);
      else if (w == PF_NF_ROOT) nf_raise(err, PF_NF_ERR_ROOT);
      else if (w != PF_NF_NONE) o = -w - 2;
      owner[(size_t)b * (size_t)RC + (size_t)v] = o;
    }
    if (count) {                                                     // one atomic per run of neighbouring lanes with the same owner
      const int before = __shfl_up(o, 1);
      const bool head = lane == 0u || before != o;
      const unsigned long long heads = __builtin_amdgcn_ballot_w64(head);
      if (head && o >= 0) {
        const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
        const int run = above ? __builtin_ctzll(above) + 1 : 64 - (int)lane;
        __hip_atomic_fetch_add(&count[(size_t)off[b] + (size_t)o], (unsigned long long)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

}  // namespace pf
