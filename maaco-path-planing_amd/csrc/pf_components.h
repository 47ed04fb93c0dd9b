// pf_components.h -- connected components of the free cells under one move policy: labels, sizes, reachability queries
// (pf_components, pf_component_sizes, pf_components_same).
//
// The rule.  A cell is free iff its occupancy byte is not 1.  Two free cells are adjacent iff the policy's move mask allows the move
// (symmetric under all four policies: a diagonal asks for the same two side cells in both directions).  labels[v] = -1 on an
// obstacle, else the rank of v's component when the components are ordered by their smallest cell id.
//
// The algorithm: union-find over one int32 parent word per cell, the root of a tree its smallest cell id (Playne-Hawick, Komura,
// ECL-CC).  Every parent points at a cell of the same component with a smaller id (or at itself), so the forest has no cycle
// whatever order the links land in, and the root a component ends with is its smallest cell: the result does not depend on timing.
// (the link step below is the global form, PF_CC_TILED = 0; the shipped tiled form replaces these two kernels, see further down)
//     k_cc_init_parent_lowest_back_neighbour  parent[v] = the first legal one of NW, N, NE, W (ids v - C - 1, v - C, v - C + 1, v - 1), else
//                                   v; -1 on an obstacle.  A launch of its own: the link kernel may write any free cell's word.
//     k_cc_link_forward_edges       one thread per cell, edges E, S, SE, SW (every edge is seen from its lower end).  SE is skipped when E
//                                   or S is legal and SW when S or W is: the side cell that move proves free joins the two ends by
//                                   two orthogonal moves, which every policy allows.  link(a, b): find both roots, CAS the higher
//                                   root's word from itself to the lower root; a failed CAS returns the word's value, and the
//                                   find starts again from it.
//     k_cc_flatten_and_count_roots  root[v] by chasing the parents (nobody writes them in this launch) into the caller's label
//                                   words, and the number of roots per 256-cell block
//     k_cc_scan_block_counts        one workgroup: exclusive scan of the block counts in block order; the total is `count`
//     k_cc_rank_roots               rank[v] = block offset + the roots in front of v in its block, for every root v: the exclusive
//                                   scan of the "is root" flags in cell order.  size[rank] = 0, first[rank] is v itself
//     k_cc_write_labels             labels[v] = rank[root[v]], -1 on an obstacle (each thread reads and writes its own label word)
//     k_cc_histogram                sizes: one integer atomic per distinct label of a 64-cell group; the label of the group's first
//                                   counted lane runs on over 16 groups and costs one atomic per change; also the free cells and
//                                   first[] where they are asked for
//     k_cc_largest / k_cc_write_info_block  the largest size, the lowest label on a tie, as one 64-bit atomic max of
//                                   (size << 32) | ~label; then the four words of `info`
//
// Visibility.  Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  The link
// kernel is the only launch in which a thread reads words another workgroup may write, and EVERY access to the parent array in it is
// an agent-scope atomic: relaxed __hip_atomic_load in the finds, an atomic min (no return) for path halving, a CAS for the link.
// The link is correct under finds that followed outdated parents: a word changes from v (root) to a smaller id of the same
// component once, by a CAS, and afterwards only to still smaller ids of that component (halving, atomic min), so any value ever read
// from p[x] is a cell of x's component with an id <= x, and a find from it ends in a cell that was a root when its word was read.
// If it is no root any more the CAS fails and hands back the value to go on from; ids only fall, so the loop ends.  Every other kernel
// reads data nobody writes in its launch (or its own words only); kernel boundaries are the only synchronisation.  No spin-wait,
// no cooperative launch, no fence.
#pragma once

namespace pf {

#ifndef PF_CC_TILED
#define PF_CC_TILED 1                           /* 1: label tiles in LDS first, link only the tile borders in HBM; 0: the global form */
#endif
#define PF_CC_THREADS 256                       /* cells per workgroup, all per-cell kernels */
#define PF_CC_TW 64                             /* the tiled form's tile: 64 x 16 cells, four per thread; a tile row is one 64-byte mask line */
#define PF_CC_TH 16
#define PF_CC_HIST_PER 16                       /* k_cc_histogram: consecutive 64-cell groups a wavefront folds before it flushes */
#define PF_CC_SCAN_THREADS 1024                 /* the one workgroup that scans the block counts */
#define PF_CC_CTL_WORDS 8                       /* control block (64-bit words): [0] count, [1] free cells, [2] largest key */

// SCOPE: __HIP_MEMORY_SCOPE_AGENT on the parent words in HBM, __HIP_MEMORY_SCOPE_WORKGROUP on a tile's words in LDS
template <int SCOPE>
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// the root of x's tree as far as this thread can see; every word on the way is pulled one step closer (path halving)
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* p, int x) {
  int cur = cc_load<SCOPE>(p + x);
  while (cur != x) {
    const int nxt = cc_load<SCOPE>(p + cur);
    if (nxt != cur) (void)__hip_atomic_fetch_min(p + x, nxt, __ATOMIC_RELAXED, SCOPE);
    x = cur; cur = nxt;
  }
  return x;
}

template <int SCOPE>
__device__ __forceinline__ void cc_link(int* p, int a, int b) {
  a = cc_find<SCOPE>(p, a); b = cc_find<SCOPE>(p, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int seen = hi;
    if (__hip_atomic_compare_exchange_strong(p + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) break;
    a = cc_find<SCOPE>(p, seen);                                     // hi had been linked meanwhile: go on from what its word holds
    b = cc_find<SCOPE>(p, lo);
  }
}

__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_init_parent_lowest_back_neighbour(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, int RC, int C,
                                                                                       int* __restrict__ parent) {
  const int v = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  if (v >= RC) return;
  int p = -1;
  if (occ[v] != 1) {
    const unsigned m = mm[v];
    p = (m & 0x80u) ? v - C - 1 : (m & 0x08u) ? v - C : (m & 0x40u) ? v - C + 1 : (m & 0x02u) ? v - 1 : v;
  }
  parent[v] = p;
}

__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_link_forward_edges(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, int RC, int C, int* __restrict__ parent) {
  const int v = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  if (v >= RC || occ[v] == 1) return;
  const unsigned m = mm[v];
  if (m & 0x01u) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + 1);
  if (m & 0x04u) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + C);
  if ((m & 0x10u) && !(m & 0x05u)) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + C + 1);
  if ((m & 0x20u) && !(m & 0x06u)) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + C - 1);
}

// ---- the tiled form (PF_CC_TILED = 1): one workgroup labels a tile of PF_CC_TW x PF_CC_TH cells in LDS -- the same union-find over
// local ids lr * PF_CC_TW + lc, which order like the cell ids, with workgroup-scope atomics (LDS atomics never leave the workgroup) --
// and writes parent[v] = the cell id of v's root within the tile; then one thread per cell links the forward edges that leave its
// tile in HBM exactly as the global form does.  Cells of the tile beyond the grid count as obstacles.
__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_label_tiles_in_lds(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, int R, int C, int* __restrict__ parent) {
  constexpr int N = PF_CC_TW * PF_CC_TH, PER = N / PF_CC_THREADS;
  __shared__ int lp[N];
  __shared__ uint8_t lm[N];
  const int r0 = (int)blockIdx.y * PF_CC_TH, c0 = (int)blockIdx.x * PF_CC_TW;
  const int tid = (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_CC_THREADS, lr = i / PF_CC_TW, lc = i % PF_CC_TW, r = r0 + lr, c = c0 + lc;
    int p = -1;
    unsigned m = 0;
    if (r < R && c < C && occ[r * C + c] != 1) {
      m = mm[r * C + c];
      // the moves that stay inside the tile
      if (lc + 1 >= PF_CC_TW) m &= ~0x51u;                             // E, SE, NE
      if (lc == 0) m &= ~0xA2u;                                        // W, SW, NW
      if (lr + 1 >= PF_CC_TH) m &= ~0x34u;                             // S, SE, SW
      if (lr == 0) m &= ~0xC8u;                                        // N, NE, NW
      p = (m & 0x80u) ? i - PF_CC_TW - 1 : (m & 0x08u) ? i - PF_CC_TW : (m & 0x40u) ? i - PF_CC_TW + 1 : (m & 0x02u) ? i - 1 : i;
    }
    lp[i] = p; lm[i] = (uint8_t)m;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_CC_THREADS;
    if (lp[i] < 0) continue;                                         // (-1 is never overwritten: no link names an obstacle)
    const unsigned m = lm[i];
    if (m & 0x01u) cc_link<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, i, i + 1);
    if (m & 0x04u) cc_link<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, i, i + PF_CC_TW);
    if ((m & 0x10u) && !(m & 0x05u)) cc_link<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, i, i + PF_CC_TW + 1);   // (a diagonal inside the tile has both its
    if ((m & 0x20u) && !(m & 0x06u)) cc_link<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, i, i + PF_CC_TW - 1);   //  side cells inside it: the global form's rule holds)
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = tid + j * PF_CC_THREADS, lr = i / PF_CC_TW, lc = i % PF_CC_TW, r = r0 + lr, c = c0 + lc;
    if (r >= R || c >= C) continue;
    int x = lp[i];
    if (x >= 0) { int y = i; while (x != y) { y = x; x = lp[y]; } x = (r0 + x / PF_CC_TW) * C + c0 + x % PF_CC_TW; }
    parent[r * C + c] = x;
  }
}

__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_link_tile_borders(const uint8_t* __restrict__ occ, const uint8_t* __restrict__ mm, int RC, int C, int* __restrict__ parent) {
  const int v = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  if (v >= RC || occ[v] == 1) return;
  const int r = v / C, c = v - r * C;
  const bool right = c % PF_CC_TW == PF_CC_TW - 1, left = c % PF_CC_TW == 0, bottom = r % PF_CC_TH == PF_CC_TH - 1;
  if (!(right || left || bottom)) return;
  const unsigned m = mm[v];
  // A straight border edge repeats its neighbour's one cell back along the border when both ends step back inside their own
  // tiles: (v - C, v) and (v - C + 1, v + 1) are tile edges and (v - C, v - C + 1) crosses the same border.  The first cell of
  // such a run, and of a tile side, links.
  if ((m & 0x01u) && right && !(r % PF_CC_TH != 0 && (m & 0x08u) && (mm[v + 1] & 0x08u))) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + 1);
  if ((m & 0x04u) && bottom && !(!left && (m & 0x02u) && (mm[v + C] & 0x02u))) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + C);
  if ((m & 0x10u) && !(m & 0x05u) && (right || bottom)) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + C + 1);
  if ((m & 0x20u) && !(m & 0x06u) && (left || bottom)) cc_link<__HIP_MEMORY_SCOPE_AGENT>(parent, v, v + C - 1);
}

// the number of set flags in the lanes below this one, and in the whole workgroup (-> *total, every thread); wsum: 2 * waves ints
__device__ __forceinline__ int cc_block_prefix(bool flag, int* wsum, int* total) {
  const unsigned long long bal = __ballot(flag);
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
  const int below = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < nw; ++w) { const int s = wsum[w]; before += w < wave ? s : 0; all += s; }
  *total = all;
  return before + below;
}

__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_flatten_and_count_roots(int RC, const int* __restrict__ parent, int* __restrict__ root, int* __restrict__ block_roots) {
  __shared__ int wsum[PF_CC_THREADS / 64];
  const int v = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  int r = -1;
  if (v < RC) {
    r = parent[v];
    if (r >= 0) { int x = v; while (r != x) { x = r; r = parent[x]; } }
    root[v] = r;
  }
  int total;
  (void)cc_block_prefix(v < RC && r == v, wsum, &total);
  if (threadIdx.x == 0) block_roots[blockIdx.x] = total;
}

// in place: counts -> exclusive offsets; ctl[0] = the total
__global__ __launch_bounds__(PF_CC_SCAN_THREADS) void k_cc_scan_block_counts(int nblocks, int* __restrict__ block_roots, unsigned long long* __restrict__ ctl) {
  __shared__ int wsum[PF_CC_SCAN_THREADS / 64];
  __shared__ int carry_s;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < nblocks; base += PF_CC_SCAN_THREADS) {
    const int i = base + tid;
    const int x = i < nblocks ? block_roots[i] : 0;
    int incl = x;                                                    // inclusive scan inside the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(incl, d); if (lane >= d) incl += y; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = carry_s, all = 0;
    for (int w = 0; w < PF_CC_SCAN_THREADS / 64; ++w) { const int s = wsum[w]; before += w < wave ? s : 0; all += s; }
    if (i < nblocks) block_roots[i] = before + incl - x;
    __syncthreads();
    if (tid == 0) carry_s += all;
    __syncthreads();
  }
  if (tid == 0) ctl[0] = (unsigned long long)carry_s;
}

__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_rank_roots(int RC, const int* __restrict__ parent, const int* __restrict__ block_off, int* __restrict__ rank,
                                                                int* __restrict__ size) {
  __shared__ int wsum[PF_CC_THREADS / 64];
  const int v = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  const bool is_root = v < RC && parent[v] == v;
  int total;
  const int k = block_off[blockIdx.x] + cc_block_prefix(is_root, wsum, &total);
  if (is_root) { rank[v] = k; size[k] = 0; }
}

__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_write_labels(int RC, const int* __restrict__ rank, int* __restrict__ labels) {
  const int v = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  if (v >= RC) return;
  const int r = labels[v];                                           // the root k_cc_flatten_and_count_roots left here
  labels[v] = r < 0 ? -1 : rank[r];
}

// sizes[l] += the cells of label l, labels outside [0, count) ignored (count: *d_count when given); first (or null): atomic min of
// the cell id, over unsigned words preset to 0xFFFFFFFF; nfree (or null): += the cells counted.  A wavefront walks PF_CC_HIST_PER
// consecutive 64-cell groups and makes one atomic per distinct label of a group, from that label's lowest lane; the label of the
// group's first counted lane is folded into a running (label, cells) pair instead, flushed when that label changes and at the end.
template <typename T>
__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_histogram(int RC, const int* __restrict__ labels, const unsigned long long* __restrict__ d_count, int count,
                                                               T* __restrict__ sizes, unsigned* __restrict__ first, unsigned long long* __restrict__ nfree) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long wave = (long long)blockIdx.x * (PF_CC_THREADS / 64) + (long long)(threadIdx.x >> 6);
  const long long base = wave * (PF_CC_HIST_PER * 64);
  if (d_count) count = (int)*d_count;
  int run_label = -1, run_cells = 0, counted = 0;                    // (wave-uniform)
  for (int j = 0; j < PF_CC_HIST_PER; ++j) {
    const long long v = base + (long long)j * 64 + lane;
    if (base + (long long)j * 64 >= RC) break;
    const int l = v < RC ? labels[v] : -1;
    const bool on = l >= 0 && l < count;
    const unsigned long long act = __ballot(on);
    if (!act) continue;
    counted += __popcll(act);
    unsigned long long rest = act;
    for (bool head = true; rest; head = false) {                     // one turn per distinct label of the group, lowest lane first
      const int lead = __ffsll((long long)rest) - 1;
      const int l0 = __shfl(l, lead);
      const unsigned long long same = __ballot(on && l == l0);
      rest &= ~same;
      if (head) {                                                    // the group's first label goes on with, or replaces, the running pair
        if (l0 != run_label) {
          if (run_cells && lane == 0 && sizes) atomicAdd(sizes + run_label, (T)run_cells);
          run_label = l0; run_cells = 0;
          if (first && lane == lead) atomicMin(first + l0, (unsigned)v);   // (a running label's earlier groups hold lower ids)
        }
        run_cells += __popcll(same);
      } else if (lane == lead) {
        if (sizes) atomicAdd(sizes + l0, (T)__popcll(same));
        if (first) atomicMin(first + l0, (unsigned)v);
      }
    }
  }
  if (lane == 0) {
    if (run_cells && sizes) atomicAdd(sizes + run_label, (T)run_cells);
    if (nfree && counted) atomicAdd(nfree, (unsigned long long)counted);
  }
}

__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_largest(const int* __restrict__ size, unsigned long long* __restrict__ ctl) {
  const int count = (int)ctl[0];
  unsigned long long best = 0ull;
  for (int l = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x); l < count; l += (int)(gridDim.x * PF_CC_THREADS)) {
    const unsigned long long key = ((unsigned long long)(unsigned)size[l] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)l);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(best, d); best = o > best ? o : best; }
  if ((threadIdx.x & 63u) == 0 && best) atomicMax(ctl + 2, best);
}

__global__ void k_cc_write_info_block(const unsigned long long* __restrict__ ctl, long long* __restrict__ info) {
  if (blockIdx.x || threadIdx.x) return;
  const long long count = (long long)ctl[0];
  info[0] = count;
  info[1] = (long long)ctl[1];
  info[2] = count ? (long long)(ctl[2] >> 32) : 0;
  info[3] = count ? (long long)(0xFFFFFFFFu - (unsigned)(ctl[2] & 0xFFFFFFFFull)) : -1;
}

template <typename T>
__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_fill_words_with_a_value(T* __restrict__ dst, int n, T value) {
  const int i = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  if (i < n) dst[i] = value;
}

// same[i] = 1 iff both ids lie in [0, RC), both labels are >= 0 and equal
__global__ __launch_bounds__(PF_CC_THREADS) void k_cc_same_pairs(int RC, const int* __restrict__ labels, int n, const int* __restrict__ a, const int* __restrict__ b,
                                                                int* __restrict__ same) {
  const int i = (int)(blockIdx.x * PF_CC_THREADS + threadIdx.x);
  if (i >= n) return;
  const int x = a[i], y = b[i];
  int s = 0;
  if (x >= 0 && x < RC && y >= 0 && y < RC) { const int lx = labels[x]; s = (lx >= 0 && lx == labels[y]) ? 1 : 0; }
  same[i] = s;
}

}  // namespace pf
