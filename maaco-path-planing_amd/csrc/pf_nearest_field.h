// pf_nearest_field.h -- nearest-source fields: ONE field seeded with a whole source set, and the owner of every cell
// (pf_dist_field_merged, pf_dist_field_owners).
//
// Why the merged field is exact.  The table is the least fixed point of
//     D[s] = 0 for every free source s of the set,   D[v] = min over legal moves u -> v of fl(D[u] + w)   otherwise,
// which any label-correcting schedule reaches bit for bit (fl(. + w) is monotone: pf_settle.h).  A chain of fl(. + w) that starts
// at 0 in one source is a chain of that source's own field, so the fixed point is the elementwise minimum of the single-source
// fields.  Nothing in pf_dist_field.h's bucket argument needs ONE cell of label 0: every weight is >= 1, so a label of bucket
// i is set from a bucket below i, and level i relaxes bucket i into i + 1 and i + 2.  So k_dist_field_merged_source_sets
// (pf_dist_field.h) seeds bucket 0 with every free source of the set and is the only level kernel: one workgroup per set on the
// handle's list slots; a row and a slot belong to one workgroup.
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

PF_DEV void nf_raise(int* err, int bit) { __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // (the kinds add up)

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
