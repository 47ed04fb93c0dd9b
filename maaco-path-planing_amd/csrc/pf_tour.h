// pf_tour.h -- tours: the exact best order through up to 16 stops (pf_tour_matrix, pf_tour_solve).
//
// A problem is an n x n matrix d of doubles (d[i][j] the cost of going from node i to node j, >= 0 or +inf, the diagonal never
// read); node 0 is the start.  mode 0: the tour ends anywhere, 1: it returns to node 0, 2: it ends at node n - 1.  The middle
// nodes are 1..m (m = n - 1, or n - 2 in mode 2; m <= 16); bit k of a set S stands for node k + 1.  The Held-Karp table
//   f[S][j] = +inf                                          if need[j] & M is no subset of S \ {j}, or j needs the end node
//           = d[0][j]                                       if S == {j}
//           = min over i in S \ {j} of fl(f[S \ {j}][i] + d[i][j])      (i ascending, a strict <: the first minimum stays)
// is laid out as tab[S m + k] (k = j - 1).  All states of one set size are independent and read only rows of sets one element
// smaller, so the table is filled layer by layer, c = 1..m, A LANE PER STATE with the sets of size c found by filtering all
// 2^m masks on popcount.  Two forms, one rule:
//   k_tour_layers_in_lds_group_per_problem  (m <= PF_TOUR_LDS_M): one workgroup per problem, the table and the matrix in LDS,
//       the layer loop inside the kernel (one __syncthreads() per layer), the order read back by thread 0 of the workgroup.
//   k_tour_layer_lane_per_state + k_tour_trace_lane_per_problem  (larger m): the table in the handle's scratch in HBM, one
//       launch per layer over (problem, state) -- the stream orders the layers --, then one lane per problem reads the order.
// Whichever runs, totals, orders and info are the rule's: every f is one fp64 addition of two words that do not depend on the
// schedule, and the minimum keeps the first smallest candidate.  The finite states are counted with integer atomics.
#pragma once

namespace pf {

#ifndef PF_TOUR_LDS_M
#define PF_TOUR_LDS_M 9                         /* the table lies in LDS up to this m (2^9 * 9 * 8 = 36 KiB); 0: always in HBM */
#endif
#define PF_TOUR_M_MAX 16
#define PF_TOUR_THREADS 256
#define PF_TOUR_BLOCKED 0xFFFFFFFFu             /* a need word no set contains: the node needs the end */

static_assert(PF_TOUR_LDS_M >= 0 && PF_TOUR_LDS_M <= 9, "the LDS table is a static array of at most 36 KiB");

struct TourNeed { unsigned nm[PF_TOUR_M_MAX]; };  // need[k + 1] over the middle nodes, shifted to the table's bits; PF_TOUR_BLOCKED

__device__ __forceinline__ double tour_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ bool tour_same(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// d_mat[i n + j] = fields[i RC + stops[j]]: a plain gather, one lane per entry
__global__ __launch_bounds__(PF_TOUR_THREADS) void k_tour_matrix_gather(const double* __restrict__ fields, const int* __restrict__ stops, int RC, int n,
                                                                        double* __restrict__ mat) {
  const long long e = (long long)blockIdx.x * PF_TOUR_THREADS + threadIdx.x;
  if (e >= (long long)n * n) return;
  const int i = (int)(e / n), j = (int)(e - (long long)i * n);
  mat[e] = fields[(size_t)i * (size_t)RC + (size_t)stops[j]];
}

// Every off-diagonal entry is >= 0 or +inf: *bad takes the smallest flat index (b n n + i n + j) of one that is not.
__global__ __launch_bounds__(PF_TOUR_THREADS) void k_tour_validate_entries(const double* __restrict__ mat, int n, long long total, unsigned long long* __restrict__ bad) {
  const long long nn = (long long)n * n;
  for (long long e = (long long)blockIdx.x * PF_TOUR_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * PF_TOUR_THREADS) {
    const long long r = e % nn;
    if (r / n == r % n) continue;
    if (!(mat[e] >= 0.0)) atomicMin(bad, (unsigned long long)e);      // (NaN fails the comparison)
  }
}

// One state (S, k) of layer popcount(S): T = the table, D = the problem's matrix (both LDS or HBM).
template <typename TP, typename DP>
__device__ __forceinline__ double tour_state(TP T, DP D, int n, int m, unsigned S, int k, const TourNeed& need) {
  const unsigned rest = S & ~(1u << k);
  if ((need.nm[k] & ~rest) != 0u) return tour_inf();
  if (rest == 0u) return D[k + 1];                                    // d[0][k + 1]
  double best = tour_inf();
  for (unsigned q = rest; q; q &= q - 1u) {
    const int i = __ffs((int)q) - 1;
    const double v = T[(size_t)rest * (size_t)m + (size_t)i] + D[(i + 1) * n + (k + 1)];
    if (v < best) best = v;
  }
  return best;
}

// The order of one problem out of its finished table, by the fixed rule: the last middle node is the smallest j whose closing
// value equals total as a word; from (S, j) the predecessor is the smallest i of S \ {j} with fl(f[S \ {j}][i] + d[i][j]) ==
// f[S][j] as words.  At most m steps; every table index lies inside [0, 2^m m).  m == 0 is the host's.
template <typename TP, typename DP>
__device__ void tour_read_order(TP T, DP D, int mode, int n, int m, double* total_out, int* order, int* status, long long* info, unsigned long long finite) {
  const unsigned full = (1u << m) - 1u;
  const int end = mode == 1 ? 0 : n - 1;
  double total = tour_inf();
  int last = -1;
  for (int k = 0; k < m; ++k) {
    double v = T[(size_t)full * (size_t)m + (size_t)k];
    if (mode != 0) v = v + D[(k + 1) * n + end];
    if (v < total) { total = v; last = k; }
  }
  *total_out = total;
  const bool ok = last >= 0;                                          // (a finite minimum was found: total < +inf)
  *status = ok ? 0 : 1;
  if (info) { info[0] = (long long)finite; info[1] = ok ? last + 1 : -1; info[2] = 0; info[3] = 0; }
  if (!ok) {
    for (int p = 0; p < n; ++p) order[p] = -1;
    return;
  }
  order[0] = 0;
  if (mode == 2) order[n - 1] = n - 1;
  unsigned S = full;
  int k = last;
  for (int p = m; p >= 1; --p) {
    order[p] = k + 1;
    const unsigned rest = S & ~(1u << k);
    if (rest == 0u) break;
    const double want = T[(size_t)S * (size_t)m + (size_t)k];
    int prev = -1;
    for (unsigned q = rest; q; q &= q - 1u) {
      const int i = __ffs((int)q) - 1;
      if (tour_same(T[(size_t)rest * (size_t)m + (size_t)i] + D[(i + 1) * n + (k + 1)], want)) { prev = i; break; }
    }
    if (prev < 0) prev = __ffs((int)rest) - 1;                        // (cannot happen: want is one of the candidates)
    S = rest;
    k = prev;
  }
}

// The LDS form: 1 <= m <= PF_TOUR_LDS_M.  min(B, grid) workgroups loop over the problems.
__global__ __launch_bounds__(PF_TOUR_THREADS) void k_tour_layers_in_lds_group_per_problem(const double* __restrict__ mat, int mode, int n, int m, int B, TourNeed need,
                                                                                          double* __restrict__ total, int* __restrict__ order,
                                                                                          int* __restrict__ status, long long* __restrict__ info) {
  __shared__ double s_tab[(PF_TOUR_LDS_M ? (1 << PF_TOUR_LDS_M) * PF_TOUR_LDS_M : 1)];
  __shared__ double s_d[(PF_TOUR_LDS_M + 2) * (PF_TOUR_LDS_M + 2)];
  __shared__ unsigned s_finite;
  const int tid = (int)threadIdx.x, states = (1 << m) * m;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    for (int e = tid; e < n * n; e += PF_TOUR_THREADS) s_d[e] = mat[(size_t)b * (size_t)(n * n) + (size_t)e];
    if (tid == 0) s_finite = 0u;
    __syncthreads();
    unsigned mine = 0u;
    for (int c = 1; c <= m; ++c) {
      for (int s = tid; s < states; s += PF_TOUR_THREADS) {
        const unsigned S = (unsigned)(s / m);
        const int k = s - (int)S * m;
        if (__popc(S) != c || !((S >> k) & 1u)) continue;
        const double v = tour_state((const double*)s_tab, (const double*)s_d, n, m, S, k, need);
        s_tab[s] = v;
        mine += v < tour_inf() ? 1u : 0u;
      }
      __syncthreads();
    }
    if (mine) atomicAdd(&s_finite, mine);
    __syncthreads();
    if (tid == 0)
      tour_read_order((const double*)s_tab, (const double*)s_d, mode, n, m, total + b, order + (size_t)b * (size_t)n, status + b,
                      info ? info + (size_t)b * 4 : nullptr, (unsigned long long)s_finite);
    __syncthreads();
  }
}

// The HBM form, layer c: a lane per state of the 2^m m states, problems b0.. of the chunk on blockIdx.y; tab = [tables][2^m m].
__global__ __launch_bounds__(PF_TOUR_THREADS) void k_tour_layer_lane_per_state(const double* __restrict__ mat, int n, int m, int c, int nb, TourNeed need,
                                                                               double* tab, unsigned long long* __restrict__ finite) {
  const int states = (1 << m) * m;
  const int s = (int)(blockIdx.x * PF_TOUR_THREADS + threadIdx.x);
  if (s >= states) return;
  const unsigned S = (unsigned)(s / m);
  const int k = s - (int)S * m;
  if (__popc(S) != c || !((S >> k) & 1u)) return;
  for (int b = (int)blockIdx.y; b < nb; b += (int)gridDim.y) {
    double* const T = tab + (size_t)b * (size_t)states;
    const double v = tour_state((const double*)T, mat + (size_t)b * (size_t)(n * n), n, m, S, k, need);
    T[s] = v;
    if (v < tour_inf()) atomicAdd(finite + b, 1ull);
  }
}

__global__ __launch_bounds__(64) void k_tour_trace_lane_per_problem(const double* __restrict__ mat, int mode, int n, int m, int nb, const double* __restrict__ tab,
                                                                    const unsigned long long* __restrict__ finite, double* __restrict__ total,
                                                                    int* __restrict__ order, int* __restrict__ status, long long* __restrict__ info) {
  const int b = (int)(blockIdx.x * 64 + threadIdx.x);
  if (b >= nb) return;
  tour_read_order(tab + (size_t)b * (size_t)((1 << m) * m), mat + (size_t)b * (size_t)(n * n), mode, n, m, total + b, order + (size_t)b * (size_t)n, status + b,
                  info ? info + (size_t)b * 4 : nullptr, finite[b]);
}

// m == 0: n == 1 (modes 0 and 1: total 0, order [0]) or mode 2 with n == 2 (total d[0][1], order [0, 1]); a lane per problem
__global__ __launch_bounds__(64) void k_tour_no_middle_nodes(const double* __restrict__ mat, int mode, int n, int B, double* __restrict__ total, int* __restrict__ order,
                                                             int* __restrict__ status, long long* __restrict__ info) {
  const int b = (int)(blockIdx.x * 64 + threadIdx.x);
  if (b >= B) return;
  const double t = mode == 2 ? mat[(size_t)b * 4 + 1] : 0.0;
  const bool ok = t < tour_inf();
  total[b] = t;
  status[b] = ok ? 0 : 1;
  for (int p = 0; p < n; ++p) order[(size_t)b * (size_t)n + p] = ok ? p : -1;
  if (info) { info[(size_t)b * 4] = 0; info[(size_t)b * 4 + 1] = -1; info[(size_t)b * 4 + 2] = 0; info[(size_t)b * 4 + 3] = 0; }
}

}  // namespace pf
