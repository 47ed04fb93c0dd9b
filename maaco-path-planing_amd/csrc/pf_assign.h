// pf_assign.h -- assignments: the exact best robot-to-task matching (pf_assign_matrix, pf_assign_solve).
//
// A problem is an n x m matrix a of doubles, row-major, rows robots and columns tasks, 1 <= n <= m <= PF_ASSIGN_MAX; +inf = no
// way, every other entry finite with |x| <= 2^1000.  The rule (include/pathfit.h holds it word for word) inserts the rows in
// order, each by one shortest-augmenting-path tree over the columns:
//   mode 0 "sum":  potentials u, v; a tree step offers cur = fl(fl(x - u[i0]) - v[j]) to every unused column (a strict <), takes
//                  the smallest minv at the smallest j, moves the potentials by it and goes on from that column's row;
//   mode 1 "max":  the same tree without potentials (cur = x, t = max(t, delta)): t is the best possible largest entry;
//   mode 2:        mode 1, then mode 0 from fresh state with every entry above t read as +inf.
// Only additions, subtractions and comparisons occur, each one fp64 operation in the rule's order, and the argmin is over
// (value, column): whichever form runs, col, value, dual and info are the rule's words.  Two forms, switched on m:
//   k_assign_wave_per_problem   (m <= PF_ASSIGN_WAVE_M): a wavefront per problem, column j in lane j (v, minv, way, p, used) and
//       row r in lane r (u, its column, "in the tree"); row i0 arrives in one coalesced load, u[i0] and p[j1] by lane read, the
//       minimum by a butterfly of lane exchanges and a ballot.  No LDS, no barrier.
//   k_assign_group_per_problem  (larger m): a workgroup per problem, thread t holds columns t, t + T, ...; u and the master copy
//       of p lie in LDS; the argmin is a wave reduction over (value, column, p) and one exchange through LDS, double-buffered so
//       that a tree step costs one barrier; thread 0 walks the augmenting path.
// Every loop is bounded (a tree has at most m steps, a row is inserted once) and every index is a column < m or a row < n.
#pragma once

namespace pf {

#ifndef PF_ASSIGN_MAX
#define PF_ASSIGN_MAX 1024
#endif
#ifndef PF_ASSIGN_WAVE_M
#define PF_ASSIGN_WAVE_M 64                     /* the wave form runs up to this m; 0: the workgroup form at every m */
#endif
#ifndef PF_ASSIGN_THREADS
#define PF_ASSIGN_THREADS 256                   /* the workgroup form's threads: 256 (four columns a thread at m = 1024) or 1024 */
#endif
#define PF_ASSIGN_GATHER_THREADS 256
#define PF_ASSIGN_WAVES 4                       /* problems (wavefronts) per workgroup of the wave form */
#define PF_ASSIGN_NONE 0x7FFFFFFF               /* the column of an empty argmin */

static_assert(PF_ASSIGN_WAVE_M >= 0 && PF_ASSIGN_WAVE_M <= 64, "a lane per column");
static_assert(PF_ASSIGN_THREADS == 256 || PF_ASSIGN_THREADS == 1024, "the workgroup form is built for 256 or 1024 threads");

__device__ __forceinline__ double assign_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double assign_big() { return __longlong_as_double(0x7E70000000000000ll); }   // 2^1000

// d_mat[(row0 + i) ld + j] (or [j ld + row0 + i]) = fields[i RC + cols[j]]: a plain gather, one lane per entry
__global__ __launch_bounds__(PF_ASSIGN_GATHER_THREADS) void k_assign_matrix_gather(const double* __restrict__ fields, const int* __restrict__ cols, int RC, int n_rows,
                                                                                   int n_cols, int row0, int ld, int transpose, double* __restrict__ mat) {
  const long long e = (long long)blockIdx.x * PF_ASSIGN_GATHER_THREADS + threadIdx.x;
  if (e >= (long long)n_rows * n_cols) return;
  const int i = (int)(e / n_cols), j = (int)(e - (long long)i * n_cols);
  const double x = fields[(size_t)i * (size_t)RC + (size_t)cols[j]];
  mat[transpose ? (size_t)j * (size_t)ld + (size_t)(row0 + i) : (size_t)(row0 + i) * (size_t)ld + (size_t)j] = x;
}

// Every entry is +inf or finite with |x| <= 2^1000: *bad takes the smallest flat index of one that is not (NaN, -inf, beyond).
__global__ __launch_bounds__(PF_ASSIGN_GATHER_THREADS) void k_assign_validate_entries(const double* __restrict__ mat, long long total, unsigned long long* __restrict__ bad) {
  for (long long e = (long long)blockIdx.x * PF_ASSIGN_GATHER_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * PF_ASSIGN_GATHER_THREADS) {
    const double x = mat[e];
    if (!(x == assign_inf() || fabs(x) <= assign_big())) atomicMin(bad, (unsigned long long)e);
  }
}

// lane reads: `l` is wave-uniform and a lane < 64
__device__ __forceinline__ int assign_lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double assign_lane_d(double v, int l) {
  const long long w = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)w, l), hi = __builtin_amdgcn_readlane((int)(w >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}

// ---- the wave form ----------------------------------------------------------------------------------------------------------
// One phase over the wavefront's problem.  Lane j < m is column j (p, v), lane r < n is row r (u, mycol).  Returns the first row
// that could not be placed, or -1.
template <bool SUM>
__device__ __forceinline__ int assign_wave_phase(const double* __restrict__ a, int n, int m, int lane, double limit, int& p, int& mycol, double& u, double& v, double& t,
                                                 long long& steps) {
  const bool col = lane < m;
  p = -1;
  mycol = -1;
  u = 0.0;
  v = 0.0;
  t = -assign_inf();
  steps = 0;
  for (int i = 0; i < n; ++i) {
    double minv = assign_inf();
    int way = -1, i0 = i, j0 = -1;
    bool used = false, rowin = lane == i, ended = false;
    for (int s = 0; s < m; ++s) {
      ++steps;
      double x = col ? a[i0 * m + lane] : assign_inf();
      if (SUM) {
        if (x > limit) x = assign_inf();
        x = x - assign_lane_d(u, i0);
        x = x - v;
      }
      const bool open = col && !used;
      if (open && x < minv) {
        minv = x;
        way = j0;
      }
      const double key = open ? minv : assign_inf();
      double best = key;
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const double q = __shfl_xor(best, o);
        if (q < best) best = q;
      }
      const unsigned long long eq = __ballot(open && key == best);
      if (!(best < assign_inf()) || eq == 0ull) return i;             // no unused column, or delta == +inf
      const int j1 = __ffsll((long long)eq) - 1;                      // the smallest column that holds the minimum
      const double delta = assign_lane_d(key, j1);
      if (SUM) {
        if (rowin) u = u + delta;
        if (col) {
          if (used) v = v - delta;
          else minv = minv - delta;
        }
      } else if (delta > t) {
        t = delta;
      }
      j0 = j1;
      if (lane == j1) used = true;
      const int pj = assign_lane_i(p, j1);
      if (pj < 0) { ended = true; break; }
      i0 = pj;                                                        // a matched row: 0 <= pj < i
      if (lane == pj) rowin = true;
    }
    if (!ended) return i;                                             // (cannot happen: at most i < m columns are matched)
    int j = j0;
    for (int s = 0; s < m && j >= 0; ++s) {                           // augment: p[j] = p[way[j]], the first column takes row i
      const int jp = assign_lane_i(way, j);
      const int r = jp < 0 ? i : assign_lane_i(p, jp);
      if (lane == j) p = r;
      if (lane == r) mycol = j;
      j = jp;
    }
  }
  return -1;
}

__global__ __launch_bounds__(64 * PF_ASSIGN_WAVES) void k_assign_wave_per_problem(const double* __restrict__ mat, int mode, int n, int m, int B, int* __restrict__ col,
                                                                                  double* __restrict__ value, int* __restrict__ status, double* __restrict__ dual,
                                                                                  long long* __restrict__ info) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long b = (long long)blockIdx.x * PF_ASSIGN_WAVES + (long long)(threadIdx.x >> 6);
  if (b >= (long long)B) return;                                      // (the whole wavefront: there is no barrier in this kernel)
  const double* const a = mat + (size_t)b * (size_t)(n * m);
  int p = -1, mycol = -1, bad = -1;
  double u = 0.0, v = 0.0, t = -assign_inf(), limit = assign_inf();
  long long steps_sum = 0, steps_max = 0;
  if (mode != 0) {
    bad = assign_wave_phase<false>(a, n, m, lane, limit, p, mycol, u, v, t, steps_max);
    limit = t;
  }
  if (mode != 1 && bad < 0) {
    double t2;
    bad = assign_wave_phase<true>(a, n, m, lane, limit, p, mycol, u, v, t2, steps_sum);
  }
  const bool ok = bad < 0;
  if (lane < n) col[(size_t)b * (size_t)n + (size_t)lane] = ok ? mycol : -1;
  if (dual) {
    const bool keep = ok && mode != 1;
    if (lane < n) dual[(size_t)b * (size_t)(n + m) + (size_t)lane] = keep ? u : 0.0;
    if (lane < m) dual[(size_t)b * (size_t)(n + m) + (size_t)(n + lane)] = keep ? v : 0.0;
  }
  double sum = assign_inf(), mx = assign_inf();
  if (ok) {
    const double e = (lane < n && mycol >= 0 && mycol < m) ? a[lane * m + mycol] : 0.0;
    sum = assign_lane_d(e, 0);
    mx = sum;
    for (int i = 1; i < n; ++i) {                                     // the left-to-right sum of a[i][col[i]]
      const double x = assign_lane_d(e, i);
      sum = sum + x;
      if (x > mx) mx = x;
    }
  }
  if (lane == 0) {
    value[(size_t)b * 2] = sum;
    value[(size_t)b * 2 + 1] = mx;
    status[b] = ok ? 0 : 1;
    if (info) {
      info[(size_t)b * 4] = steps_sum;
      info[(size_t)b * 4 + 1] = steps_max;
      info[(size_t)b * 4 + 2] = bad;
      info[(size_t)b * 4 + 3] = 0;
    }
  }
}

// ---- the workgroup form -----------------------------------------------------------------------------------------------------
template <int T>
struct AssignShared {
  double u[PF_ASSIGN_MAX];                      // the row potentials
  double e[PF_ASSIGN_MAX];                      // a[i][col[i]], for the left-to-right sum
  int p[PF_ASSIGN_MAX];                         // the master copy of p (the owners hold theirs in registers)
  int way[PF_ASSIGN_MAX];                       // published at a tree's end for the walk back
  int col[PF_ASSIGN_MAX];
  double rv[2][T / 64];                         // the argmin exchange: (value, column, p of that column) per wavefront, two buffers
  int rj[2][T / 64], rp[2][T / 64];
};

__device__ __forceinline__ bool assign_before(double av, int aj, double bv, int bj) { return av < bv || (av == bv && aj < bj); }

// One phase over the workgroup's problem; thread tid owns columns tid + k T.  `par` is the exchange buffer of the next tree step.
// Returns the first row that could not be placed, or -1, the same in every thread.
template <int T, bool SUM>
__device__ __forceinline__ int assign_group_phase(const double* __restrict__ a, int n, int m, double limit, AssignShared<T>& sh, double (&v)[PF_ASSIGN_MAX / T],
                                                  int (&p)[PF_ASSIGN_MAX / T], double& t, long long& steps, int& par) {
  constexpr int CPT = PF_ASSIGN_MAX / T, W = T / 64;
  const int tid = (int)threadIdx.x;
  double minv[CPT];
  int way[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    v[k] = 0.0;
    p[k] = -1;
    const int j = tid + k * T;
    if (j < m) sh.p[j] = -1;
  }
  for (int r = tid; r < n; r += T) {
    sh.u[r] = 0.0;
    sh.col[r] = 0;
  }
  t = -assign_inf();
  steps = 0;
  __syncthreads();
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      minv[k] = assign_inf();
      way[k] = -1;
    }
    unsigned used = 0u;
    int i0 = i, j0 = -1;
    bool ended = false;
    for (int s = 0; s < m; ++s) {
      ++steps;
      const double ui0 = SUM ? sh.u[i0] : 0.0;
      const double* const row = a + (size_t)i0 * (size_t)m;
      double bv = assign_inf();
      int bj = PF_ASSIGN_NONE, bp = -1;
#pragma unroll
      for (int k = 0; k < CPT; ++k) {
        const int j = tid + k * T;
        if (j < m && !((used >> k) & 1u)) {
          double x = row[j];
          if (SUM) {
            if (x > limit) x = assign_inf();
            x = x - ui0;
            x = x - v[k];
          }
          if (x < minv[k]) {
            minv[k] = x;
            way[k] = j0;
          }
          if (minv[k] < bv) {                                         // (k ascending is j ascending: the smallest j stays)
            bv = minv[k];
            bj = j;
            bp = p[k];
          }
        }
      }
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const double qv = __shfl_xor(bv, o);
        const int qj = __shfl_xor(bj, o), qp = __shfl_xor(bp, o);
        if (assign_before(qv, qj, bv, bj)) {
          bv = qv;
          bj = qj;
          bp = qp;
        }
      }
      if ((tid & 63) == 0) {
        sh.rv[par][tid >> 6] = bv;
        sh.rj[par][tid >> 6] = bj;
        sh.rp[par][tid >> 6] = bp;
      }
      __syncthreads();
      double delta = sh.rv[par][0];
      int j1 = sh.rj[par][0], pj = sh.rp[par][0];
#pragma unroll
      for (int w = 1; w < W; ++w) {
        const double qv = sh.rv[par][w];
        const int qj = sh.rj[par][w];
        if (assign_before(qv, qj, delta, j1)) {
          delta = qv;
          j1 = qj;
          pj = sh.rp[par][w];
        }
      }
      par ^= 1;
      if (j1 == PF_ASSIGN_NONE) return i;                             // no unused column with a finite minv: delta == +inf
      if (SUM) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
          const int j = tid + k * T;
          if (j < m) {
            if ((used >> k) & 1u) {
              if (p[k] >= 0 && p[k] < n) sh.u[p[k]] = sh.u[p[k]] + delta;   // (a used column is matched: 0 <= p[k] < i, one column a row)
              v[k] = v[k] - delta;
            } else {
              minv[k] = minv[k] - delta;
            }
          }
        }
        if (tid == 0) sh.u[i] = sh.u[i] + delta;
      } else if (delta > t) {
        t = delta;
      }
      j0 = j1;
      if ((j1 & (T - 1)) == tid) used |= 1u << (j1 / T);
      if (pj < 0) { ended = true; break; }
      i0 = pj;
    }
    if (!ended) return i;                                             // (cannot happen: at most i < m columns are matched)
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int j = tid + k * T;
      if (j < m) sh.way[j] = way[k];
    }
    __syncthreads();
    if (tid == 0) {
      int j = j0;
      for (int s = 0; s < m && j >= 0; ++s) {                         // augment: p[j] = p[way[j]], the first column takes row i
        const int jp = sh.way[j];
        sh.p[j] = jp < 0 ? i : sh.p[jp];
        j = jp;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int j = tid + k * T;
      if (j < m) p[k] = sh.p[j];
    }
  }
  return -1;
}

template <int T>
__global__ __launch_bounds__(T) void k_assign_group_per_problem(const double* __restrict__ mat, int mode, int n, int m, int B, int* __restrict__ col,
                                                                double* __restrict__ value, int* __restrict__ status, double* __restrict__ dual,
                                                                long long* __restrict__ info) {
  constexpr int CPT = PF_ASSIGN_MAX / T;
  __shared__ AssignShared<T> sh;
  const int tid = (int)threadIdx.x;
  int par = 0;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const double* const a = mat + (size_t)b * (size_t)n * (size_t)m;
    double v[CPT];
    int p[CPT];
    int bad = -1;
    double t = -assign_inf(), limit = assign_inf();
    long long steps_sum = 0, steps_max = 0;
    if (mode != 0) {
      bad = assign_group_phase<T, false>(a, n, m, limit, sh, v, p, t, steps_max, par);
      limit = t;
      __syncthreads();
    }
    if (mode != 1 && bad < 0) {
      double t2;
      bad = assign_group_phase<T, true>(a, n, m, limit, sh, v, p, t2, steps_sum, par);
      __syncthreads();
    }
    const bool ok = bad < 0;
    if (ok) {
#pragma unroll
      for (int k = 0; k < CPT; ++k) {
        const int j = tid + k * T;
        if (j < m && p[k] >= 0 && p[k] < n) sh.col[p[k]] = j;
      }
    }
    __syncthreads();
    for (int r = tid; r < n; r += T) {
      const int c = sh.col[r];                                        // a column < m (0 until its row is matched)
      col[(size_t)b * (size_t)n + (size_t)r] = ok ? c : -1;
      sh.e[r] = ok ? a[(size_t)r * (size_t)m + (size_t)c] : 0.0;
      if (dual) dual[(size_t)b * (size_t)(n + m) + (size_t)r] = (ok && mode != 1) ? sh.u[r] : 0.0;
    }
    if (dual) {
#pragma unroll
      for (int k = 0; k < CPT; ++k) {
        const int j = tid + k * T;
        if (j < m) dual[(size_t)b * (size_t)(n + m) + (size_t)(n + j)] = (ok && mode != 1) ? v[k] : 0.0;
      }
    }
    __syncthreads();
    if (tid == 0) {
      double sum = assign_inf(), mx = assign_inf();
      if (ok) {
        sum = sh.e[0];
        mx = sum;
        for (int i = 1; i < n; ++i) {                                 // the left-to-right sum of a[i][col[i]]
          const double x = sh.e[i];
          sum = sum + x;
          if (x > mx) mx = x;
        }
      }
      value[(size_t)b * 2] = sum;
      value[(size_t)b * 2 + 1] = mx;
      status[b] = ok ? 0 : 1;
      if (info) {
        info[(size_t)b * 4] = steps_sum;
        info[(size_t)b * 4 + 1] = steps_max;
        info[(size_t)b * 4 + 2] = bad;
        info[(size_t)b * 4 + 3] = 0;
      }
    }
    __syncthreads();
  }
}

}  // namespace pf
