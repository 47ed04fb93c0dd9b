// pf_cover.h -- coverage: which p of m sites see or reach the most of n elements, best-improvement additions, swaps and drops
// over bit masks (pf_cover_pack, pf_cover_improve).
//
// A problem is m masks of W = ceil(n / 64) words, element j being bit j & 63 of word j >> 6 and every bit at j >= n zero.  A start
// is Placement's row sel[0 .. p - 1]: a site or -1 per slot, no site twice, the slots below `fixed` never empty and never changed.
// cnt(sel, j) counts the non-empty slots whose mask holds j, cov(sel) the j with cnt > 0, open(sel) the non-empty slots; the key is
// (n - cov, open).  One sweep looks, for every slot o in [fixed, p), at every site i not in the row (sel[o] = i) and, where slot o
// is not empty, at the drop (sel[o] = -1, written i = m), and takes the smallest (key, o, i); it is applied iff its key is strictly
// below the row's and fewer than max_moves moves were applied (include/pathfit.h holds the rule line by line).
// k_cover_pack: a wavefront takes 64 consecutive targets of one source row, a lane a target; the word is one __ballot, stored by
//   lane 0.  A lane past n votes 0, so the tail bits of the last word are 0.
// k_cover_group_per_start: a workgroup of 1024 threads per start, the move loop in the kernel.  Two planes of W words per start:
//   any[w] the union of the row's masks and once[w] the elements exactly one slot covers; the head of a sweep fills them, a thread
//   per word scanning the p slots (twice |= any & x; any |= x; once = any & ~twice).  They live in dynamic LDS while
//   W <= PF_COVER_LDS_WORDS (64 KiB for both, so that two workgroups share a CU's 160 KiB) and in a block of the handle's scratch
//   per workgroup above (the template argument; the code is otherwise the same; that form's 82 VGPRs leave room for one
//   workgroup a CU, so its grid is min(B, CUs)).  Taking slot o out of the row leaves
//   base(o) = any & ~(once & M[sel o]), so candidate (o, i) covers sum_w popc(base(o)[w] | M[i][w]), the drop sum_w popc(base(o)[w])
//   and an addition sum_w popc(any[w] | M[i][w]).  Every empty slot has the same candidates with the same keys and the smallest o
//   wins the tie, so only the smallest empty slot is evaluated: the evaluated slots, the non-empty ones of [fixed, p) and that one,
//   stand in ascending order in a list of E <= p entries.
//   The deal PF_COVER_DEAL = 1 (shipped): a wavefront per site (the drop being site m), the words strided over the lanes,
//   eight slots of the list at a time with an accumulator each in registers, one sum over the lanes per (site, slot).  = 0: lane =
//   q P + e with P the power of two >= E, so 64 / P sites share a wavefront; a lane walks all W words of its own candidate, the
//   lanes of one site reading the same M[i][w] and the planes as broadcasts.  The sums are integers: both deals give the same words
//   (scripts/probe_cover.py measures them).
//   A candidate is one 64-bit word (n - cov') << 24 | open' << 17 | o << 11 | i (n - cov' <= 2^20, open' <= 64, o < 64, i <= 1024),
//   so the smallest (key, o, i) is the smallest word: lane exchanges within a wavefront, one exchange through LDS across them.
// Every site read out of a row was checked by k_place_validate_rows before this kernel is launched: it lies in [-1, m), no site
// stands twice, so every mask row is a site in [0, m) (a drop and an idle lane read row 0 and discard it) and every index into the
// taken flags a site in [0, m).  Every plane and mask word index is a w in [0, W); every index into the row a slot in [0, p) and into
// the list an e in [0, E).  An applied candidate was evaluated: o is a listed slot, i a site not in the row or m on a non-empty slot.
// k_cover_pack reads source element k ld + t with k < K and t a target that k_cover_validate_targets found in [0, ld).
#pragma once

#include "pf_place.h"

namespace pf {

#ifndef PF_COVER_SITES_MAX
#define PF_COVER_SITES_MAX 1024
#endif
#ifndef PF_COVER_ELEMS_MAX
#define PF_COVER_ELEMS_MAX 1048576
#endif
#ifndef PF_COVER_OPEN_MAX
#define PF_COVER_OPEN_MAX 64
#endif
#ifndef PF_COVER_DEAL
#define PF_COVER_DEAL 1                         /* 1: a wavefront per site, the words strided over the lanes; 0: lane = (site group, slot), a lane walks the words */
#endif
#ifndef PF_COVER_LDS_WORDS
#define PF_COVER_LDS_WORDS 4096                 /* the planes live in LDS up to this many words each (16 bytes a word for the two) */
#endif
#define PF_COVER_GROUP 1024                     /* the threads of a start's workgroup */
#define PF_COVER_THREADS 256                    /* the pack and validation kernels' */
#define PF_COVER_NONE (~0ull)                   /* the word of an empty minimum */

static_assert(PF_COVER_SITES_MAX == 1024 && PF_COVER_OPEN_MAX == 64 && PF_COVER_ELEMS_MAX == (1 << 20), "a candidate's word is (n - cov) << 24 | open << 17 | o << 11 | i");
static_assert(PF_COVER_LDS_WORDS >= 1 && PF_COVER_LDS_WORDS <= 4096, "two workgroups' planes share a CU's LDS");

typedef unsigned long long cover_u64;

// Every target lies in [0, ld): *bad takes the smallest index of one that does not.
__global__ __launch_bounds__(PF_COVER_THREADS) void k_cover_validate_targets(const int* __restrict__ tgt, int n, int ld, cover_u64* __restrict__ bad) {
  for (int j = (int)(blockIdx.x * PF_COVER_THREADS + threadIdx.x); j < n; j += (int)(gridDim.x * PF_COVER_THREADS)) {
    const int t = tgt[j];
    if (t < 0 || t >= ld) atomicMin(bad, (cover_u64)j);
  }
}

// K source rows at the n targets -> rows row0 .. row0 + K - 1 of mask [.][W].  KIND 0: bytes, the bit is byte != 0; KIND 1: doubles,
// the bit is x <= radius (radius is finite: +inf and NaN give 0).  blockIdx.y is the source row, a wavefront a word.
template <int KIND>
__global__ __launch_bounds__(PF_COVER_THREADS) void k_cover_pack(const void* __restrict__ src, const int* __restrict__ tgt, int n, int ld, double radius, int row0,
                                                                 cover_u64* __restrict__ mask) {
  const int W = (n + 63) >> 6, lane = (int)threadIdx.x & 63;
  const int w = (int)blockIdx.x * (PF_COVER_THREADS / 64) + ((int)threadIdx.x >> 6);      // (wave-uniform)
  if (w >= W) return;
  const int k = (int)blockIdx.y, j = w * 64 + lane;
  bool bit = false;
  if (j < n) {
    const size_t at = (size_t)k * (size_t)ld + (size_t)tgt[j];
    if (KIND == 0) bit = ((const unsigned char*)src)[at] != 0;
    else bit = ((const double*)src)[at] <= radius;
  }
  const cover_u64 word = __ballot(bit ? 1 : 0);
  if (lane == 0) mask[(size_t)(row0 + k) * (size_t)W + (size_t)w] = word;
}

// No mask holds a bit at j >= n: *bad takes the smallest flat row index (b m + i) of one whose last word does.
__global__ __launch_bounds__(PF_COVER_THREADS) void k_cover_validate_tail(const cover_u64* __restrict__ mask, int n, int W, long long rows, cover_u64* __restrict__ bad) {
  const cover_u64 tail = (n & 63) ? ~0ull << (n & 63) : 0ull;
  for (long long e = (long long)blockIdx.x * PF_COVER_THREADS + threadIdx.x; e < rows; e += (long long)gridDim.x * PF_COVER_THREADS)
    if (mask[(size_t)e * (size_t)W + (size_t)(W - 1)] & tail) atomicMin(bad, (cover_u64)e);
}

__device__ __forceinline__ cover_u64 cover_shfl_xor(cover_u64 v, int x) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xFFFFFFFFull), x), hi = __shfl_xor((unsigned)(v >> 32), x);
  return ((cover_u64)hi << 32) | (cover_u64)lo;
}

__device__ __forceinline__ int cover_wave_sum(int v) {
#pragma unroll
  for (int x = 32; x; x >>= 1) v += __shfl_xor(v, x);
  return v;
}

// the sum of v over the workgroup, in every thread (s_red: PF_COVER_GROUP / 64 ints; a barrier stands in front of its reuse)
__device__ __forceinline__ int cover_group_sum(int v, int* s_red, int lane, int wave) {
  v = cover_wave_sum(v);
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int q = 0; q < PF_COVER_GROUP / 64; ++q) t += s_red[q];
  return t;
}

__device__ __forceinline__ cover_u64 cover_word(int n, int cov, int open, int o, int i) {
  return ((cover_u64)(unsigned)(n - cov) << 24) | ((cover_u64)(unsigned)open << 17) | ((cover_u64)(unsigned)o << 11) | (cover_u64)(unsigned)i;
}

template <bool kLds>
__global__ __launch_bounds__(PF_COVER_GROUP) void k_cover_group_per_start(const cover_u64* __restrict__ mask, int m, int n, int p, int fixed, int B, int shared,
                                                                          int max_moves, int* sel, cover_u64* __restrict__ covered, long long* __restrict__ value,
                                                                          int* __restrict__ status, long long* __restrict__ info, cover_u64* planes) {
  constexpr int T = PF_COVER_GROUP, NW = T / 64;
  extern __shared__ cover_u64 s_cover_dyn[];    // any[W], once[W] (kLds)
  __shared__ int s_sel[PF_COVER_OPEN_MAX];
  __shared__ int s_eval[PF_COVER_OPEN_MAX];     // the evaluated slots, ascending
  __shared__ unsigned char s_taken[PF_COVER_SITES_MAX];
  __shared__ cover_u64 s_rk[NW];
  __shared__ int s_red[NW];
  __shared__ int s_E;
  const int W = (n + 63) >> 6;
  cover_u64* const p_any = kLds ? s_cover_dyn : planes + (size_t)blockIdx.x * 2 * (size_t)W;
  cover_u64* const p_once = p_any + W;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const cover_u64* const a = mask + (shared ? (size_t)0 : (size_t)b * (size_t)m * (size_t)W);
    int* const row = sel + (size_t)b * (size_t)p;
    for (int i = tid; i < m; i += T) s_taken[i] = 0;
    __syncthreads();
    if (tid < p) {
      const int v = row[tid];
      s_sel[tid] = v;
      if (v >= 0) s_taken[v] = 1;               // (a valid row: every site once)
    }
    __syncthreads();
    int opn = 0;
    for (int o = 0; o < p; ++o) opn += s_sel[o] >= 0 ? 1 : 0;
    int cov = 0, cov0 = 0, moves = 0, sweeps = 0, drops = 0, st = 2;
    const int opn0 = opn;
    for (int s = 0; s <= max_moves; ++s) {      // at most max_moves moves: at most max_moves + 1 sweeps; the loop ends by a break
      // the head of a sweep: the planes, and the list of the evaluated slots
      int mine = 0;
      for (int w = tid; w < W; w += T) {
        cover_u64 any = 0, twice = 0;
        for (int o = 0; o < p; ++o) {
          const int site = s_sel[o];
          if (site < 0) continue;
          const cover_u64 x = a[(size_t)site * (size_t)W + (size_t)w];
          twice |= any & x;
          any |= x;
        }
        p_any[w] = any;
        p_once[w] = any & ~twice;
        mine += __popcll(any);
      }
      if (tid == 0) {
        int E = 0;
        bool empty = false;
        for (int o = fixed; o < p; ++o) {
          const bool full = s_sel[o] >= 0;
          if (full || !empty) s_eval[E++] = o;
          empty = empty || !full;
        }
        s_E = E;
      }
      if (s == 0) cov = cov0 = cover_group_sum(mine, s_red, lane, wave);
      __syncthreads();
      ++sweeps;
      const int E = s_E;
      cover_u64 best = PF_COVER_NONE;
#if PF_COVER_DEAL == 0
      if (E > 0) {
        // lane = q P + e, the wavefront's sites (it NW + wave) (64 / P) + q, site m the drop; a lane walks the words of its own candidate
        int P = 1;
        while (P < E) P <<= 1;
        const int S = 64 / P, e = lane & (P - 1), q = lane / P;
        const bool has = e < E;
        const int o = has ? s_eval[e] : 0, so = has ? s_sel[o] : -1;
        const cover_u64* const rs = a + (size_t)(so >= 0 ? so : 0) * (size_t)W;
        const cover_u64 sm = so >= 0 ? ~0ull : 0ull;
        for (int i0 = wave * S; i0 <= m; i0 += NW * S) {
          const int i = i0 + q;
          const bool site = has && i < m && !s_taken[i < m ? i : 0];
          const bool live = site || (has && i == m && so >= 0);
          const cover_u64* const r = a + (size_t)(site ? i : 0) * (size_t)W;
          const cover_u64 xm = site ? ~0ull : 0ull;
          int acc = 0;
#pragma unroll 4
          for (int w = 0; w < W; ++w) acc += __popcll((p_any[w] & ~(p_once[w] & rs[w] & sm)) | (r[w] & xm));
          const cover_u64 c = cover_word(n, acc, opn + (so < 0 ? 1 : (i == m ? -1 : 0)), o, i);
          if (live && c < best) best = c;
        }
      }
#else
      // a wavefront per site, site m the drop; the words strided over the lanes, eight listed slots at a time
      for (int i = wave; i <= m; i += NW) {
        if (i < m && s_taken[i]) continue;      // (wave-uniform)
        const bool drop = i == m;
        const cover_u64* const r = a + (size_t)(drop ? 0 : i) * (size_t)W;
        const cover_u64 xm = drop ? 0ull : ~0ull;
        for (int e0 = 0; e0 < E; e0 += 8) {
          const cover_u64* rs[8];
          cover_u64 sm[8];
          int acc[8], slot[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const int o = __builtin_amdgcn_readfirstlane(e0 + t < E ? s_eval[e0 + t] : -1);
            const int so = __builtin_amdgcn_readfirstlane(o >= 0 ? s_sel[o] : -1);
            slot[t] = o;
            rs[t] = a + (size_t)(so >= 0 ? so : 0) * (size_t)W;
            sm[t] = so >= 0 ? ~0ull : 0ull;
            acc[t] = 0;
          }
          for (int w = lane; w < W; w += 64) {
            const cover_u64 any = p_any[w], once = p_once[w], x = r[w] & xm;
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[t] += __popcll((any & ~(once & rs[t][w] & sm[t])) | x);
          }
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const int c = cover_wave_sum(acc[t]);
            const bool full = sm[t] != 0;
            const cover_u64 word = cover_word(n, c, opn + (!full ? 1 : (drop ? -1 : 0)), slot[t] >= 0 ? slot[t] : 0, i);
            if (slot[t] >= 0 && (full || !drop) && word < best) best = word;
          }
        }
      }
#endif
#pragma unroll
      for (int x = 32; x; x >>= 1) {
        const cover_u64 q = cover_shfl_xor(best, x);
        best = q < best ? q : best;
      }
      if (lane == 0) s_rk[wave] = best;
      __syncthreads();
      best = s_rk[0];
#pragma unroll
      for (int q = 1; q < NW; ++q) best = s_rk[q] < best ? s_rk[q] : best;
      // (the same in every thread) no candidate, or none strictly below the row's key (n - cov, open)
      if (best == PF_COVER_NONE || !((best >> 17) < (cover_word(n, cov, opn, 0, 0) >> 17))) { st = 0; break; }
      if (moves == max_moves) { st = 2; break; }                      // a move is there and the cap forbids it
      const int o = (int)(best >> 11) & 63, i = (int)best & 2047;     // an evaluated candidate
      if (tid == 0) {                           // (the row and the flags are read before the exchange above and after the barrier below)
        const int old = s_sel[o];
        if (old >= 0) s_taken[old] = 0;
        s_sel[o] = i == m ? -1 : i;
        if (i < m) s_taken[i] = 1;
      }
      cov = n - (int)(best >> 24);
      opn = (int)(best >> 17) & 127;
      drops += i == m ? 1 : 0;
      ++moves;
      __syncthreads();                          // (also: every thread has read the wavefronts' minima before the next sweep writes them)
    }
    // (no move since the head of the last sweep: the planes are the result's)
    int mine = 0;
    for (int w = tid; w < W; w += T) {
      mine += __popcll(p_once[w]);
      if (covered) covered[(size_t)b * (size_t)W + (size_t)w] = p_any[w];
    }
    const int unique = cover_group_sum(mine, s_red, lane, wave);
    if (tid < p) row[tid] = s_sel[tid];
    if (tid == 0) {
      value[(size_t)b * 4] = cov;
      value[(size_t)b * 4 + 1] = opn;
      value[(size_t)b * 4 + 2] = cov0;
      value[(size_t)b * 4 + 3] = opn0;
      status[b] = st;
      if (info) { info[(size_t)b * 4] = moves; info[(size_t)b * 4 + 1] = sweeps; info[(size_t)b * 4 + 2] = unique; info[(size_t)b * 4 + 3] = drops; }
    }
    __syncthreads();
  }
}

}  // namespace pf
