// pf_place.h -- placement: which p of m candidate sites to open for n demands, best-improvement additions and swaps
// (pf_place_improve).
//
// A problem is an m x n matrix a of doubles, a[i][j] what demand j pays at site i, +inf or in [+0.0, 2^1000].  A start is a row
// sel[0 .. p - 1] of sites, -1 an empty slot, no site twice, the slots below `fixed` never empty and never changed.
// near(sel, j) is the smallest a[sel[s]][j] over the non-empty slots (+inf with none), cost(sel) = (uns, sum, max) the walk over
// j = 0 .. n - 1 in order: uns counts the +inf, sum = fl(sum + near) and max the largest over the others.  The key is (uns, sum) in
// mode 0 and (uns, max, sum) in mode 1.  One sweep looks at every slot o in [fixed, p) and every site i not in the row, the
// candidate being the row with sel[o] = i, and takes the smallest (key, o, i); it is applied iff its key is strictly below the
// row's and fewer than max_moves moves were applied (include/pathfit.h holds the rule word for word).
// k_place_group_per_start: a workgroup of 1024 threads per start, the move loop in the kernel.  Dynamic LDS holds, per demand j,
//   d1[j] = near(sel, j), n1[j] = the smallest slot attaining it (255 with none) and d2[j] = the smallest value over the other
//   slots; static LDS the row and a taken flag per site.  The head of a sweep fills them, a thread per demand scanning the p slots
//   (coalesced over j).  The term of candidate (o, i) at j is min(a[i][j], n1[j] == o ? d2[j] : d1[j]): a minimum is exact, so
//   that is near(row', j) as a word, and the left-to-right walk over j gives the rule's cost without forming row'.
//   The deal (shipped, PF_PLACE_PACK = 2): lane = q P + o with P the power of two >= p, so 64 / P sites share a wavefront and
//   wavefront w takes the sites (it 16 + w) (64 / P) + q; with p > 32 that is a wavefront per site and a lane per slot.  A lane
//   walks its own row a[i][.] through the caches, eight entries in flight (the lanes of one site read the same words), and reads
//   d1, d2 and n1 as LDS broadcasts.  The other form (-DPF_PLACE_PACK=0; =1 uses it for p > 32 only): a wavefront per site and a
//   lane per slot at every p, the wavefront loading 64 consecutive entries of the row, of d1, d2 and n1 coalesced, a lane each, and
//   broadcasting them lane by lane (v_readlane: the operands of a term are wave-uniform); it was 1.9x slower at p = 40 and 64 and
//   6 - 15x slower at p <= 16, where most of its lanes idle (scripts/probe_place.py).  In both a candidate walks j in ascending
//   order in one lane, and a lane meets its sites in ascending order, so a strict < keeps the first smallest; the workgroup's
//   smallest (key, o, i) is found by lane exchanges within a wavefront and one exchange through LDS across the wavefronts.  The
//   applied candidate's cost is the next row's cost: only the cost before the first sweep is walked on its own (thread 0 over d1).
// Every cost is a fixed chain of comparisons and fp64 additions on words that do not depend on the schedule, and the minimum is
// over (key, o, i): rows, owners, values, statuses and infos are the rule's words for either form and every assignment of starts
// to workgroups.  Every applied move lowers the key strictly; the move loop ends after at most max_moves + 1 sweeps.
// Every site read out of a row was checked by k_place_validate_rows before this kernel is launched: it lies in [-1, m), no site
// stands twice.  Every index into d1, d2 and n1 is a demand in [0, n) (a lane past the end of a row's last 64 entries reads
// nothing), every index into the row a slot in [0, p), every index into the taken flags and every matrix row a site in [0, m).
#pragma once

#include "pf_fleet.h"

namespace pf {

#ifndef PF_PLACE_SITES_MAX
#define PF_PLACE_SITES_MAX 1024
#endif
#ifndef PF_PLACE_DEMANDS_MAX
#define PF_PLACE_DEMANDS_MAX 4096
#endif
#ifndef PF_PLACE_OPEN_MAX
#define PF_PLACE_OPEN_MAX 64
#endif
#ifndef PF_PLACE_PACK
#define PF_PLACE_PACK 2                         /* 2: 64 / P sites share a wavefront (P the power of two >= p); 0: a wavefront per site, the terms' operands by v_readlane; 1: 2's form for p <= 32, 0's above */
#endif
#define PF_PLACE_GROUP 1024                     /* the threads of a start's workgroup */
#define PF_PLACE_THREADS 256                    /* the validation kernels' */
#define PF_PLACE_NONE 0x7FFFFFFF                /* the (o, i) word and the unserved count of an empty minimum */
#define PF_PLACE_NO_SLOT 255                    /* n1[j] where no slot reaches demand j */

static_assert(PF_PLACE_SITES_MAX == 1024 && PF_PLACE_OPEN_MAX == 64, "a candidate's word is o << 10 | i, a slot is a lane and a byte");

// Every entry is +inf or a number in [+0.0, 2^1000]: *bad takes the smallest flat index of one that is not.  The sign bit is
// tested on the word (-0.0 is an error: a minimum over +-0.0 would not be a function of the words); NaN fails the comparisons.
__global__ __launch_bounds__(PF_PLACE_THREADS) void k_place_validate_entries(const double* __restrict__ mat, long long total, unsigned long long* __restrict__ bad) {
  for (long long e = (long long)blockIdx.x * PF_PLACE_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * PF_PLACE_THREADS) {
    const double x = mat[e];
    if (__double_as_longlong(x) < 0 || !(x <= tsearch_big() || x == tsearch_inf())) atomicMin(bad, (unsigned long long)e);
  }
}

// Every row holds sites of [-1, m), no site twice, and no empty slot below `fixed`: *bad takes the smallest flat index (b p + s)
// of a slot that lies outside [-1, m), repeats the site of a smaller slot, or is empty below `fixed`.  A thread per (b, s).
__global__ __launch_bounds__(PF_PLACE_THREADS) void k_place_validate_rows(const int* __restrict__ sel, int m, int p, int fixed, long long total,
                                                                          unsigned long long* __restrict__ bad) {
  for (long long e = (long long)blockIdx.x * PF_PLACE_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * PF_PLACE_THREADS) {
    const int s = (int)(e % p);
    const int v = sel[e];
    bool ok = v >= -1 && v < m && (v >= 0 || s >= fixed);
    if (ok && v >= 0)
      for (int t = 0; t < s; ++t) ok = ok && sel[e - s + t] != v;
    if (!ok) atomicMin(bad, (unsigned long long)e);
  }
}

// A cost (uns, sum, max) with the candidate's word oi = o << 10 | i behind it.
struct place_cost {
  int uns;
  double sum, max;
  int oi;
};

__device__ __forceinline__ bool place_key_below(int mode, int ua, double sa, double ma, int ub, double sb, double mb) {
  if (ua != ub) return ua < ub;
  if (mode == 1 && ma != mb) return ma < mb;
  return sa < sb;
}

__device__ __forceinline__ bool place_key_equal(int mode, int ua, double sa, double ma, int ub, double sb, double mb) {
  return ua == ub && sa == sb && (mode == 0 || ma == mb);
}

// (key, o, i) of a before that of b
__device__ __forceinline__ bool place_before(int mode, const place_cost& a, const place_cost& b) {
  if (place_key_below(mode, a.uns, a.sum, a.max, b.uns, b.sum, b.max)) return true;
  return place_key_equal(mode, a.uns, a.sum, a.max, b.uns, b.sum, b.max) && a.oi < b.oi;
}

__device__ __forceinline__ double place_lane_f64(double x, int l) {   // the word lane l holds (l wave-uniform, lane l active)
  const long long w = __double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w & 0xFFFFFFFFll), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)w >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
}

// one term of a walk: near' = min(x, base) joins (uns, sum, mx)
__device__ __forceinline__ void place_term(double x, double base, int& uns, double& sum, double& mx) {
  const double t = x < base ? x : base;
  const bool none = t == tsearch_inf();
  const double s2 = sum + t;
  uns += none ? 1 : 0;
  sum = none ? sum : s2;
  mx = (!none && t > mx) ? t : mx;
}

__global__ __launch_bounds__(PF_PLACE_GROUP) void k_place_group_per_start(const double* __restrict__ mat, int mode, int m, int n, int p, int fixed, int B, int shared,
                                                                          int max_moves, int* sel, int* __restrict__ owner, double* __restrict__ value,
                                                                          int* __restrict__ status, long long* __restrict__ info) {
  constexpr int T = PF_PLACE_GROUP, W = T / 64;
  extern __shared__ double s_dyn[];             // d1[n], d2[n], then n1[n] as bytes
  __shared__ int s_sel[PF_PLACE_OPEN_MAX];
  __shared__ unsigned char s_taken[PF_PLACE_SITES_MAX];
  __shared__ int s_ru[W];
  __shared__ double s_rs[W];
  __shared__ double s_rm[W];
  __shared__ int s_rk[W];
  __shared__ double s_first[2];
  __shared__ int s_first_uns;
  double* const s_d1 = s_dyn;
  double* const s_d2 = s_dyn + n;
  unsigned char* const s_n1 = (unsigned char*)(s_dyn + 2 * (size_t)n);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double inf = tsearch_inf();
#if PF_PLACE_PACK
  int P = 1;
  while (P < p) P <<= 1;
  const bool pack = PF_PLACE_PACK == 2 || P <= 32;
#endif
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const double* const a = mat + (shared ? (size_t)0 : (size_t)b * (size_t)m * (size_t)n);
    int* const row = sel + (size_t)b * (size_t)p;
    for (int i = tid; i < m; i += T) s_taken[i] = 0;
    __syncthreads();
    if (tid < p) {
      const int v = row[tid];
      s_sel[tid] = v;
      if (v >= 0) s_taken[v] = 1;               // (a valid row: every site once)
    }
    __syncthreads();
    int cu = 0, bu = 0, moves = 0, sweeps = 0, st = 2;   // the row's cost (cu, cs, cm); the cost before (bu, bs, bm)
    double cs = 0.0, cm = 0.0, bs = 0.0, bm = 0.0;
    for (int s = 0; s <= max_moves; ++s) {      // at most max_moves moves: at most max_moves + 1 sweeps; the loop ends by a break
      // the head of a sweep: per demand the smallest value with its smallest slot, and the second smallest value
      for (int j = tid; j < n; j += T) {
        double v1 = inf, v2 = inf;
        int k1 = PF_PLACE_NO_SLOT;
        for (int o = 0; o < p; ++o) {
          const int site = s_sel[o];
          if (site < 0) continue;
          const double x = a[(size_t)site * (size_t)n + (size_t)j];
          if (x < v1) {
            v2 = v1;
            v1 = x;
            k1 = o;
          } else if (x < v2) {
            v2 = x;
          }
        }
        s_d1[j] = v1;
        s_d2[j] = v2;
        s_n1[j] = (unsigned char)k1;
      }
      __syncthreads();
      if (s == 0) {                             // the cost before the first sweep: one walk over d1
        if (tid == 0) {
          int u = 0;
          double sm = 0.0, mx = 0.0;
#pragma unroll 8
          for (int j = 0; j < n; ++j) place_term(s_d1[j], inf, u, sm, mx);
          s_first_uns = u;
          s_first[0] = sm;
          s_first[1] = mx;
        }
        __syncthreads();
        cu = bu = s_first_uns;
        cs = bs = s_first[0];
        cm = bm = s_first[1];
      }
      ++sweeps;
      place_cost best{PF_PLACE_NONE, inf, inf, PF_PLACE_NONE};
#if PF_PLACE_PACK
      if (pack) {
        // lane = q P + o, the wavefront's sites (it W + wave) (64 / P) + q; a lane reads its own row
        const int S = 64 / P, o = lane & (P - 1), q = lane / P;
        const bool slot = o >= fixed && o < p;
        for (int i0 = wave * S; i0 < m; i0 += W * S) {
          const int i = i0 + q;
          const bool live = slot && i < m && !s_taken[i < m ? i : 0];
          const double* const r = a + (size_t)(live ? i : 0) * (size_t)n;
          int u = 0;
          double sm = 0.0, mx = 0.0;
          int j = 0;
          for (; j + 8 <= n; j += 8) {
            double x[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = r[j + t];
#pragma unroll
            for (int t = 0; t < 8; ++t) place_term(x[t], s_n1[j + t] == o ? s_d2[j + t] : s_d1[j + t], u, sm, mx);
          }
          for (; j < n; ++j) place_term(r[j], s_n1[j] == o ? s_d2[j] : s_d1[j], u, sm, mx);
          const place_cost c{u, sm, mx, (o << 10) | i};
          if (live && place_before(mode, c, best)) best = c;
        }
      } else
#endif
      {
        // a wavefront per in-site, lane = slot; the operands of a term are broadcast lane by lane
        const int o = lane;
        const bool slot = o >= fixed && o < p;
        for (int i = wave; i < m; i += W) {
          if (s_taken[i]) continue;             // (wave-uniform)
          const double* const r = a + (size_t)i * (size_t)n;
          int u = 0;
          double sm = 0.0, mx = 0.0;
          double xn = lane < n ? r[lane] : inf; // the next 64 entries: loaded a step ahead
          for (int j0 = 0; j0 < n; j0 += 64) {
            const int jl = j0 + lane, cnt = n - j0 < 64 ? n - j0 : 64;
            const bool in = jl < n;
            const double xv = xn;
            const double a1 = in ? s_d1[jl] : inf, a2 = in ? s_d2[jl] : inf;
            const int an = in ? (int)s_n1[jl] : PF_PLACE_NO_SLOT;
            xn = jl + 64 < n ? r[jl + 64] : inf;
            if (cnt == 64) {                    // eight terms a step: the broadcasts of a step are issued together
#pragma unroll 1
              for (int l0 = 0; l0 < 64; l0 += 8) {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                  const int l = l0 + t;
                  place_term(place_lane_f64(xv, l), __builtin_amdgcn_readlane(an, l) == o ? place_lane_f64(a2, l) : place_lane_f64(a1, l), u, sm, mx);
                }
              }
            } else {
#pragma unroll 1
              for (int l = 0; l < cnt; ++l)
                place_term(place_lane_f64(xv, l), __builtin_amdgcn_readlane(an, l) == o ? place_lane_f64(a2, l) : place_lane_f64(a1, l), u, sm, mx);
            }
          }
          const place_cost c{u, sm, mx, (o << 10) | i};
          if (slot && place_before(mode, c, best)) best = c;
        }
      }
#pragma unroll
      for (int x = 32; x; x >>= 1) {
        const place_cost q{__shfl_xor(best.uns, x), __shfl_xor(best.sum, x), __shfl_xor(best.max, x), __shfl_xor(best.oi, x)};
        if (place_before(mode, q, best)) best = q;
      }
      if (lane == 0) {
        s_ru[wave] = best.uns;
        s_rs[wave] = best.sum;
        s_rm[wave] = best.max;
        s_rk[wave] = best.oi;
      }
      __syncthreads();
      best = place_cost{s_ru[0], s_rs[0], s_rm[0], s_rk[0]};
#pragma unroll
      for (int q = 1; q < W; ++q) {
        const place_cost c{s_ru[q], s_rs[q], s_rm[q], s_rk[q]};
        if (place_before(mode, c, best)) best = c;
      }
      // (the same in every thread) no candidate, or none strictly below the row's key
      if (best.oi == PF_PLACE_NONE || !place_key_below(mode, best.uns, best.sum, best.max, cu, cs, cm)) { st = 0; break; }
      if (moves == max_moves) { st = 2; break; }                      // a move is there and the cap forbids it
      const int o = best.oi >> 10, i = best.oi & 1023;                // an evaluated candidate: o in [fixed, p), i in [0, m) not in the row
      if (tid == 0) {
        const int old = s_sel[o];
        if (old >= 0) s_taken[old] = 0;
        s_sel[o] = i;
        s_taken[i] = 1;
      }
      cu = best.uns;
      cs = best.sum;
      cm = best.max;
      ++moves;
      __syncthreads();                          // (also: every thread has read the wavefronts' minima before the next sweep writes them)
    }
    // (no move since the head of the last sweep: d1 and n1 are the result's)
    if (tid < p) row[tid] = s_sel[tid];
    if (owner)
      for (int j = tid; j < n; j += T) {
        const int k1 = (int)s_n1[j];
        owner[(size_t)b * (size_t)n + j] = k1 == PF_PLACE_NO_SLOT ? -1 : s_sel[k1];
      }
    if (tid == 0) {
      value[(size_t)b * 4] = cs;
      value[(size_t)b * 4 + 1] = cm;
      value[(size_t)b * 4 + 2] = bs;
      value[(size_t)b * 4 + 3] = bm;
      status[b] = st;
      if (info) { info[(size_t)b * 4] = moves; info[(size_t)b * 4 + 1] = sweeps; info[(size_t)b * 4 + 2] = cu; info[(size_t)b * 4 + 3] = bu; }
    }
    __syncthreads();
  }
}

}  // namespace pf
