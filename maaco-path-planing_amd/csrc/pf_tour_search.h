// pf_tour_search.h -- tour search: best-improvement 2-opt over up to 1024 stops (pf_tour_improve).
//
// A problem is an n x n matrix d of doubles of which only the upper triangle is read: w(x, y) = d[min(x, y) n + max(x, y)],
// w(x, none) = w(x, x) = +0.0.  A start is an order row: a permutation of the nodes that begins with node 0 (and ends with node
// n - 1 in mode 2); order[n] stands for order[0] in mode 1 and for "none" otherwise.  One sweep looks at every pair
// 1 <= i < j <= hi (hi = n - 1, or n - 2 in mode 2) with a = order[i-1], b = order[i], c = order[j], e = order[j+1]:
//   delta(i, j) = fl(fl(w(a,c) + w(b,e)) - fl(w(a,b) + w(c,e)))
// and takes the smallest delta at the smallest (i, j); if it is < 0 the positions i..j are reversed (a move) and the sweep runs
// again, else the order is a local optimum (include/pathfit.h holds the rule word for word).
// k_tour_search_group_per_start: a workgroup of 1024 threads per start, the order row in LDS, the move loop in the kernel.
//   The pairs are numbered row by row (row i holds hi - i of them) and thread t takes the pairs t, t + T, ..., each decoded in
//   closed form (tsearch_pair), so every thread sees the same number of pairs to within one.  w(a,b) and w(c,e) are legs of the
//   order as it stands: all threads fill leg[k] = w(order[k], order[k+1]) in LDS at the head of a sweep, which leaves two
//   gathers a pair, w(a,c) and w(b,e), read through the caches (every workgroup of a shared matrix reads the same words); a
//   thread has the gathers of four pairs in flight.  It keeps its best (delta, i << 16 | j) -- the pairs come in ascending
//   (i, j), so a strict < keeps the first smallest --; the workgroup's is found by lane exchanges within a wavefront and one
//   exchange through LDS across the wavefronts, lexicographic on (delta, key).  The reversal is (j - i + 1) / 2 swaps, a thread
//   each.  Three barriers a sweep.  The totals are the legs' sums.
// Every delta is three fp64 operations on words that do not depend on the schedule and the minimum is over (delta, i, j): orders,
// values, statuses and infos are the rule's words for every T, unroll and assignment of starts to workgroups.  (A form with the
// matrix mirrored into LDS up to n = 128 and 256-thread workgroups up to n = 256 were measured and dropped: docs/experiments/.)
// Every loop is bounded: a sweep takes pairs / T steps, the move loop ends after at most max_moves + 1 sweeps.  Every node read
// out of an order row was checked to lie in [0, n) by k_tour_search_validate_orders before this kernel is launched.
#pragma once

namespace pf {

#ifndef PF_TOUR_SEARCH_MAX
#define PF_TOUR_SEARCH_MAX 1024
#endif
#ifndef PF_TOUR_SEARCH_GROUP
#define PF_TOUR_SEARCH_GROUP 1024               /* the threads of a start's workgroup (a multiple of 64) */
#endif
#ifndef PF_TOUR_SEARCH_UNROLL
#define PF_TOUR_SEARCH_UNROLL 4                 /* the pairs a thread has in flight: their loads are issued together */
#endif
#define PF_TOUR_SEARCH_THREADS 256              /* the validation kernels' */
#define PF_TOUR_SEARCH_NONE 0x7FFFFFFF          /* the key of an empty minimum */

static_assert(PF_TOUR_SEARCH_MAX == 1024, "a pair's key is i << 16 | j, the order row a static array");
static_assert(PF_TOUR_SEARCH_GROUP % 64 == 0 && PF_TOUR_SEARCH_GROUP >= 64 && PF_TOUR_SEARCH_GROUP <= 1024, "whole wavefronts, one workgroup");

__device__ __forceinline__ double tsearch_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double tsearch_big() { return __longlong_as_double(0x7E70000000000000ll); }   // 2^1000

// Every upper-triangle entry is >= 0 and (<= 2^1000 or +inf): *bad takes the smallest flat index (b n n + i n + j) of one that is
// not (NaN fails the comparisons); has_inf[b] becomes 1 for a matrix with a +inf entry there (zeroed by the host before).
__global__ __launch_bounds__(PF_TOUR_SEARCH_THREADS) void k_tour_search_validate_entries(const double* __restrict__ mat, int n, long long total,
                                                                                         unsigned long long* __restrict__ bad, int* __restrict__ has_inf) {
  const long long nn = (long long)n * n;
  for (long long e = (long long)blockIdx.x * PF_TOUR_SEARCH_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * PF_TOUR_SEARCH_THREADS) {
    const long long r = e % nn;
    if (r / n >= r % n) continue;
    const double x = mat[e];
    if (!(x >= 0.0 && (x <= tsearch_big() || x == tsearch_inf()))) atomicMin(bad, (unsigned long long)e);
    else if (x == tsearch_inf()) has_inf[e / nn] = 1;                 // (every writer stores the same word)
  }
}

// Every start row is a permutation of 0..n-1 with node 0 first (and node n - 1 last in mode 2): *bad takes the smallest flat
// index (b n + p) of a position whose node lies outside [0, n), repeats the node of a smaller position, or breaks a fixed end.
// A workgroup per row; first[v] = the smallest position that holds node v.
__global__ __launch_bounds__(PF_TOUR_SEARCH_THREADS) void k_tour_search_validate_orders(const int* __restrict__ order, int mode, int n, int B,
                                                                                        unsigned long long* __restrict__ bad) {
  __shared__ int first[PF_TOUR_SEARCH_MAX];
  const int tid = (int)threadIdx.x;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const int* const row = order + (size_t)b * (size_t)n;
    for (int v = tid; v < n; v += PF_TOUR_SEARCH_THREADS) first[v] = PF_TOUR_SEARCH_NONE;
    __syncthreads();
    for (int p = tid; p < n; p += PF_TOUR_SEARCH_THREADS) {
      const int v = row[p];
      if (v >= 0 && v < n) atomicMin(&first[v], p);
    }
    __syncthreads();
    for (int p = tid; p < n; p += PF_TOUR_SEARCH_THREADS) {
      const int v = row[p];
      const bool ok = v >= 0 && v < n && first[v] == p && (p != 0 || v == 0) && (mode != 2 || p != n - 1 || v == n - 1);
      if (!ok) atomicMin(bad, (unsigned long long)b * (unsigned long long)n + (unsigned long long)p);
    }
    __syncthreads();
  }
}

// Pair number k -> (i, j), the pairs numbered row by row: row i = 1 .. hi - 1 holds j = i + 1 .. hi, and row r + 1 begins at
// off(r) = r (2 hi - 1 - r) / 2.  0 <= k < hi (hi - 1) / 2.  r is the smaller root of r^2 - (2 hi - 1) r + 2 k = 0, rounded down:
// every integer here lies below 2^24 and is exact as a float, the root may be one off and is put right by the two loops.
__device__ __forceinline__ void tsearch_pair(int k, int hi, int& i, int& j) {
  const int c = 2 * hi - 1;
  int r = (int)(((float)c - sqrtf((float)(c * c - 8 * k))) * 0.5f);
  r = max(0, min(r, hi - 2));
  while (r < hi - 2 && (r + 1) * (c - (r + 1)) / 2 <= k) ++r;
  while (r > 0 && r * (c - r) / 2 > k) --r;
  i = r + 1;
  j = i + 1 + (k - r * (c - r) / 2);
}

__device__ __forceinline__ bool tsearch_before(double av, int ak, double bv, int bk) { return av < bv || (av == bv && ak < bk); }

__global__ __launch_bounds__(PF_TOUR_SEARCH_GROUP) void k_tour_search_group_per_start(const double* __restrict__ mat, const int* __restrict__ has_inf, int mode, int n, int B, int shared,
                                                                   int max_moves, int* order, double* __restrict__ value, int* __restrict__ status,
                                                                   long long* __restrict__ info) {
  constexpr int T = PF_TOUR_SEARCH_GROUP, W = T / 64;
  __shared__ int s_order[PF_TOUR_SEARCH_MAX + 1];
  __shared__ double s_leg[PF_TOUR_SEARCH_MAX];
  __shared__ double s_rv[W];
  __shared__ int s_rk[W];
  const int tid = (int)threadIdx.x;
  const int hi = mode == 2 ? n - 2 : n - 1;
  const int pairs = hi >= 2 ? hi * (hi - 1) / 2 : 0;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const int mi = shared ? 0 : b;
    const double* const m = mat + (size_t)mi * (size_t)n * (size_t)n;
    int* const row = order + (size_t)b * (size_t)n;
    if (has_inf[mi]) {                          // the rule needs finite weights: not searched
      for (int p = tid; p < n; p += T) row[p] = -1;
      if (tid == 0) {
        value[(size_t)b * 2] = tsearch_inf();
        value[(size_t)b * 2 + 1] = tsearch_inf();
        status[b] = 1;
        if (info) { info[(size_t)b * 4] = 0; info[(size_t)b * 4 + 1] = 0; info[(size_t)b * 4 + 2] = 0; info[(size_t)b * 4 + 3] = 0; }
      }
      continue;
    }
    for (int p = tid; p < n; p += T) s_order[p] = row[p];
    if (tid == 0) s_order[n] = mode == 1 ? 0 : -1;
    __syncthreads();
    // w(x, y) for two different nodes; w(x, e) where e may be "none" (-1) or, for n == 1 in mode 1, x itself
    auto w2 = [&](int x, int y) -> double {
      return x < y ? m[(size_t)x * (size_t)n + (size_t)y] : m[(size_t)y * (size_t)n + (size_t)x];
    };
    auto we = [&](int x, int e) -> double { return (e < 0 || e == x) ? 0.0 : w2(x, e); };
    // leg[k] = w(order[k], order[k + 1]), the n legs of the order as it stands: filled by all threads at the head of every sweep,
    // where they serve as w(a, b) = leg[i - 1] and w(c, e) = leg[j]; their left-to-right sum is the total (thread 0 adds them up)
    auto sum_legs = [&]() -> double {
      double t = s_leg[0];
      for (int k = 1; k < n; ++k) t = t + s_leg[k];
      return t;
    };
    double before = 0.0;
    int moves = 0, sweeps = 0, st = 2;
    for (int s = 0; s <= max_moves; ++s) {      // at most max_moves moves: at most max_moves + 1 sweeps; the loop ends by a break
      for (int k = tid; k < n; k += T) s_leg[k] = we(s_order[k], s_order[k + 1]);
      __syncthreads();
      if (s == 0 && tid == 0) before = sum_legs();
      ++sweeps;
      double bd = 0.0;                          // only a delta < 0 is a move
      int bk = PF_TOUR_SEARCH_NONE;
      for (int k0 = tid; k0 < pairs; k0 += PF_TOUR_SEARCH_UNROLL * T) {
        double wac[PF_TOUR_SEARCH_UNROLL], wbe[PF_TOUR_SEARCH_UNROLL], old[PF_TOUR_SEARCH_UNROLL], d[PF_TOUR_SEARCH_UNROLL];
        int key[PF_TOUR_SEARCH_UNROLL];
        bool open_end[PF_TOUR_SEARCH_UNROLL];
#pragma unroll
        for (int u = 0; u < PF_TOUR_SEARCH_UNROLL; ++u) {             // every load is issued before the first is used: a slot past the end reads pair 0
          const int k = k0 + u * T;
          int i, j;
          tsearch_pair(k < pairs ? k : 0, hi, i, j);
          const int a = s_order[i - 1], bn = s_order[i], c = s_order[j], e = s_order[j + 1];
          open_end[u] = e < 0;                                        // w(b, none) = +0.0: some other node is read and dropped
          wac[u] = w2(a, c);
          wbe[u] = w2(bn, open_end[u] ? (bn ? 0 : 1) : e);
          old[u] = s_leg[i - 1] + s_leg[j];
          key[u] = k < pairs ? (i << 16) | j : PF_TOUR_SEARCH_NONE;
        }
#pragma unroll
        for (int u = 0; u < PF_TOUR_SEARCH_UNROLL; ++u) d[u] = (wac[u] + (open_end[u] ? 0.0 : wbe[u])) - old[u];
#pragma unroll
        for (int u = 0; u < PF_TOUR_SEARCH_UNROLL; ++u) {             // ascending pairs: a strict < keeps the first smallest
          if (key[u] != PF_TOUR_SEARCH_NONE && d[u] < bd) {
            bd = d[u];
            bk = key[u];
          }
        }
      }
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const double qv = __shfl_xor(bd, o);
        const int qk = __shfl_xor(bk, o);
        if (tsearch_before(qv, qk, bd, bk)) {
          bd = qv;
          bk = qk;
        }
      }
      if ((tid & 63) == 0) {
        s_rv[tid >> 6] = bd;
        s_rk[tid >> 6] = bk;
      }
      __syncthreads();
      double dv = s_rv[0];
      int dk = s_rk[0];
#pragma unroll
      for (int q = 1; q < W; ++q) {
        const double qv = s_rv[q];
        const int qk = s_rk[q];
        if (tsearch_before(qv, qk, dv, dk)) {
          dv = qv;
          dk = qk;
        }
      }
      if (dk == PF_TOUR_SEARCH_NONE) { st = 0; break; }               // a local optimum (the same in every thread)
      if (moves == max_moves) { st = 2; break; }                      // a move is there and the cap forbids it
      const int i = dk >> 16, j = dk & 0xFFFF;                        // 1 <= i < j <= hi: an evaluated pair
      for (int t = tid; t < (j - i + 1) / 2; t += T) {
        const int x = s_order[i + t];
        s_order[i + t] = s_order[j - t];
        s_order[j - t] = x;
      }
      ++moves;
      __syncthreads();                          // (also: every thread has read s_rv / s_rk before the next sweep writes them)
    }
    for (int p = tid; p < n; p += T) row[p] = s_order[p];             // (no move since the legs were filled: they are the result's)
    if (tid == 0) {
      value[(size_t)b * 2] = sum_legs();
      value[(size_t)b * 2 + 1] = before;
      status[b] = st;
      if (info) { info[(size_t)b * 4] = moves; info[(size_t)b * 4 + 1] = sweeps; info[(size_t)b * 4 + 2] = 0; info[(size_t)b * 4 + 3] = 0; }
    }
    __syncthreads();
  }
}

}  // namespace pf
