// pf_fleet.h -- fleet routes: best-improvement 2-opt and segment relocation over k robots and n tasks, k + n <= 1024
// (pf_fleet_improve).
//
// A problem is an N x N matrix d of doubles, N = k + n, nodes 0 .. k - 1 the robots' start cells, nodes k .. N - 1 the tasks; only
// the upper triangle is read, w(x, y) = d[min(x, y) N + max(x, y)], w(x, none) = w(x, x) = +0.0, and never a robot-robot entry.
// A start is a route row: a permutation of the nodes with route[0] = 0 and the robots in increasing order; the tasks behind robot
// r's marker are its route.  nxt(p) = route[p + 1] where that is a task, else END(rob(p)): "none" in mode 0, node rob(p) in mode 1.
// One sweep looks at two families of candidates (include/pathfit.h holds the rule word for word):
//   code 0, 2-opt:     1 <= i < j <= N - 1 with the positions i .. j all tasks; a = route[i-1], b = route[i], c = route[j], e = nxt(j),
//                      delta = fl(fl(w(a,c) + w(b,e)) - fl(w(a,b) + w(c,e)));  the positions i .. j are reversed
//   code L = 1, 2, 3:  the segment i .. i + L - 1 (all tasks) goes behind position j (j < i - 1 or j > i + L - 1, markers included),
//                      admissible iff rob(j) == rob(i) or cnt[rob(j)] + L <= cap[rob(j)];
//                      delta = fl(add - rem), rem = fl(fl(w(a,s1) + w(sL,b)) - w(a,b)), add = fl(fl(w(p,s1) + w(sL,q)) - w(p,q))
// and takes the smallest (delta, code, i, j); if its delta is < 0 and fewer than max_moves moves were applied, it is applied.
// k_fleet_group_per_start: a workgroup of 1024 threads per start, the move loop in the kernel.  LDS holds the route row, rob per
//   position, the markers' positions, cnt and cap per robot, nxt per position, leg[p] = w(route[p], nxt(p)) and rem[L][i].  The head of
//   a sweep fills them from the row as it stands: a marker writes its position, a position finds its robot by bisection over
//   the markers' positions, rem costs one gather per (L, i).  w(a,b), w(c,e) and w(p,q) are then legs, so a candidate costs two
//   gathers, read through the caches.  The 2-opt pairs are numbered row by row as the tour search's (tsearch_pair) and thread t takes
//   the pairs t, t + T, ...; the relocations of all three lengths are one row-major [3 N][N] grid of which thread t takes the cells
//   t, t + T, ..., its (L, i, j) carried along without a division.  A thread has the gathers of four candidates in flight.  It keeps
//   its best (delta, code << 20 | i << 10 | j) -- its candidates come in ascending key, so a strict < keeps the first smallest --;
//   the workgroup's is found by lane exchanges within a wavefront and one exchange through LDS across the wavefronts.  A move is
//   applied by all threads: a reversal is (j - i + 1) / 2 swaps, a relocation writes the shifted stretch into the nxt words (they are
//   filled again by the next sweep) and copies it back.  The lengths are one thread per robot, summing its legs in order.
// Every delta is a fixed chain of fp64 operations on words that do not depend on the schedule and the minimum is over
// (delta, code, i, j): routes, lengths, values, statuses and infos are the rule's words for every T, unroll and assignment of
// starts to workgroups.  The relocate delta is nested roundings: nothing says that an accepted move shortens the real-number
// total, so every loop is bounded by the cap: the move loop ends after at most max_moves + 1 sweeps.
// Every node read out of a route row was checked by k_fleet_validate_rows before this kernel is launched: it lies in [0, N), the
// row is a permutation, the markers stand in increasing order from position 0 on.  Every index into LDS is a position in [0, N),
// a robot in [0, k] (the markers' positions hold N at index k) or a (L - 1) N + i with i + L <= N.
#pragma once

#include "pf_tour_search.h"

namespace pf {

#ifndef PF_FLEET_MAX
#define PF_FLEET_MAX 1024
#endif
#ifndef PF_FLEET_GROUP
#define PF_FLEET_GROUP 1024                     /* the threads of a start's workgroup (a multiple of 64) */
#endif
#ifndef PF_FLEET_UNROLL
#define PF_FLEET_UNROLL 4                       /* the candidates a thread has in flight: their loads are issued together */
#endif
#define PF_FLEET_THREADS 256                    /* the validation kernels' */
#define PF_FLEET_NONE 0x7FFFFFFF                /* the key of an empty minimum */
#define PF_FLEET_NO_CAP 0x3FFFFFFF              /* cap[r] without capacities */

static_assert(PF_FLEET_MAX == 1024, "a candidate's key is code << 20 | i << 10 | j, the rows static arrays");
static_assert(PF_FLEET_GROUP % 64 == 0 && PF_FLEET_GROUP >= 64 && PF_FLEET_GROUP <= 1024, "whole wavefronts, one workgroup");

// Every readable entry (i < j, j a task) is >= 0 and (<= 2^1000 or +inf): *bad takes the smallest flat index (b N N + i N + j) of
// one that is not (NaN fails the comparisons); has_inf[b] becomes 1 for a matrix with a +inf entry there (zeroed by the host before).
__global__ __launch_bounds__(PF_FLEET_THREADS) void k_fleet_validate_entries(const double* __restrict__ mat, int k, int N, long long total,
                                                                             unsigned long long* __restrict__ bad, int* __restrict__ has_inf) {
  const long long nn = (long long)N * N;
  for (long long e = (long long)blockIdx.x * PF_FLEET_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * PF_FLEET_THREADS) {
    const long long r = e % nn;
    const int i = (int)(r / N), j = (int)(r % N);
    if (i >= j || j < k) continue;
    const double x = mat[e];
    if (!(x >= 0.0 && (x <= tsearch_big() || x == tsearch_inf()))) atomicMin(bad, (unsigned long long)e);
    else if (x == tsearch_inf()) has_inf[e / nn] = 1;                 // (every writer stores the same word)
  }
}

// Every start row is a permutation of 0 .. N - 1 with node 0 first and the robots in increasing order: *bad takes the smallest flat
// index (b N + p) of a position whose node lies outside [0, N), repeats the node of a smaller position, is not node 0 at position 0,
// or is a robot r >= 1 that robot r - 1 does not stand in front of.  A workgroup per row; first[v] = the smallest position of node v.
__global__ __launch_bounds__(PF_FLEET_THREADS) void k_fleet_validate_rows(const int* __restrict__ route, int k, int N, int B, unsigned long long* __restrict__ bad) {
  __shared__ int first[PF_FLEET_MAX];
  const int tid = (int)threadIdx.x;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const int* const row = route + (size_t)b * (size_t)N;
    for (int v = tid; v < N; v += PF_FLEET_THREADS) first[v] = PF_FLEET_NONE;
    __syncthreads();
    for (int p = tid; p < N; p += PF_FLEET_THREADS) {
      const int v = row[p];
      if (v >= 0 && v < N) atomicMin(&first[v], p);
    }
    __syncthreads();
    for (int p = tid; p < N; p += PF_FLEET_THREADS) {
      const int v = row[p];
      const bool ok = v >= 0 && v < N && first[v] == p && (p != 0 || v == 0) && (v < 1 || v >= k || first[v - 1] < p);
      if (!ok) atomicMin(bad, (unsigned long long)b * (unsigned long long)N + (unsigned long long)p);
    }
    __syncthreads();
  }
}

// Every robot of every (valid) row holds at most cap[r] tasks: *bad takes the smallest flat index (b k + r) of one that holds
// more.  A workgroup per row; at[r] = the position of robot r's marker, at[k] = N.
__global__ __launch_bounds__(PF_FLEET_THREADS) void k_fleet_validate_caps(const int* __restrict__ route, const int* __restrict__ cap, int k, int N, int B,
                                                                          unsigned long long* __restrict__ bad) {
  __shared__ int at[PF_FLEET_MAX + 1];
  const int tid = (int)threadIdx.x;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const int* const row = route + (size_t)b * (size_t)N;
    for (int p = tid; p < N; p += PF_FLEET_THREADS) {
      const int v = row[p];
      if (v >= 0 && v < k) at[v] = p;                                 // (a valid row: every robot once)
    }
    if (tid == 0) at[k] = N;
    __syncthreads();
    for (int r = tid; r < k; r += PF_FLEET_THREADS)
      if (at[r + 1] - at[r] - 1 > cap[r]) atomicMin(bad, (unsigned long long)b * (unsigned long long)k + (unsigned long long)r);
    __syncthreads();
  }
}

// What the two rules (the sum of the lengths here, the largest length in pf_fleet_balance.h) do differently is a policy P: its
// LDS words (P::Lds), a thread's best candidate, begin (the head of a sweep, by all threads), take (a thread looks at one admissible
// candidate -- delta, and for a relocation rem, add and the length of the segment's own legs --; its candidates come in ascending key), reduce (the workgroup's best into every thread), improves, commit (the applied
// candidate's bookkeeping) and the words of value and info.  fleet_group is everything else: the rows in LDS, the head of a sweep,
// the candidates' gathers, the move.
struct fleet_sum {
  static constexpr int W = PF_FLEET_GROUP / 64;
  struct Lds {
    double rv[W];
    int rk[W];
  };
  double bd;
  int bk;
  static __device__ __forceinline__ double* keep(Lds&) { return nullptr; }
  __device__ __forceinline__ void begin(Lds&, int, int) {}
  __device__ __forceinline__ void reset() {
    bd = 0.0;                                   // only a delta < 0 is a move
    bk = PF_FLEET_NONE;
  }
  __device__ __forceinline__ void take(const Lds&, double d, double, double, double, int, int, int key) {
    if (d < bd) {
      bd = d;
      bk = key;
    }
  }
  __device__ __forceinline__ void reduce(Lds& s, int tid) {
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
      s.rv[tid >> 6] = bd;
      s.rk[tid >> 6] = bk;
    }
    __syncthreads();
    bd = s.rv[0];
    bk = s.rk[0];
#pragma unroll
    for (int q = 1; q < W; ++q) {
      const double qv = s.rv[q];
      const int qk = s.rk[q];
      if (tsearch_before(qv, qk, bd, bk)) {
        bd = qv;
        bk = qk;
      }
    }
  }
  __device__ __forceinline__ bool improves() const { return bk != PF_FLEET_NONE; }   // no delta < 0 otherwise (the same in every thread)
  __device__ __forceinline__ int key() const { return bk; }
  __device__ __forceinline__ void commit(Lds&, int, int, int) {}
  static __device__ __forceinline__ void not_searched(double* value, long long* info, size_t b) {
    value[b * 3] = tsearch_inf();
    value[b * 3 + 1] = tsearch_inf();
    value[b * 3 + 2] = tsearch_inf();
    if (info) { info[b * 4] = 0; info[b * 4 + 1] = 0; info[b * 4 + 2] = 0; info[b * 4 + 3] = 0; }
  }
  __device__ __forceinline__ void write(double* value, long long* info, size_t b, double before, double, double after, double span, int moves, int sweeps,
                                        int two) const {
    value[b * 3] = after;
    value[b * 3 + 1] = before;
    value[b * 3 + 2] = span;
    if (info) { info[b * 4] = moves; info[b * 4 + 1] = sweeps; info[b * 4 + 2] = two; info[b * 4 + 3] = moves - two; }
  }
};

template <class P>
__device__ __forceinline__ void fleet_group(const double* __restrict__ mat, const int* __restrict__ has_inf, const int* __restrict__ cap, int mode, int k, int N, int B,
                                            int shared, int max_moves, int* route, double* __restrict__ len, double* __restrict__ value, int* __restrict__ status,
                                            long long* __restrict__ info) {
  constexpr int T = PF_FLEET_GROUP, U = PF_FLEET_UNROLL;
  __shared__ int s_route[PF_FLEET_MAX];
  __shared__ int s_rob[PF_FLEET_MAX];
  __shared__ int s_nxt[PF_FLEET_MAX];           // nxt(p), -1 for "none"; the scratch row of a relocation
  __shared__ int s_at[PF_FLEET_MAX + 1];        // the markers' positions, N at index k
  __shared__ int s_cnt[PF_FLEET_MAX];
  __shared__ int s_cap[PF_FLEET_MAX];
  __shared__ double s_leg[PF_FLEET_MAX];
  __shared__ double s_rem[3 * PF_FLEET_MAX];    // rem[(L - 1) N + i], NaN where the segment is none; the lengths before and after
  __shared__ typename P::Lds s_p;
  const int tid = (int)threadIdx.x;
  const int pairs = N >= 3 ? (N - 1) * (N - 2) / 2 : 0;               // the tour search's pairs with hi = N - 1
  const int cells = 3 * N * N;                                        // the relocations' grid
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    const int mi = shared ? 0 : b;
    const double* const m = mat + (size_t)mi * (size_t)N * (size_t)N;
    int* const row = route + (size_t)b * (size_t)N;
    if (has_inf[mi]) {                          // the rule needs finite weights: not searched
      for (int p = tid; p < N; p += T) row[p] = -1;
      for (int r = tid; r < k; r += T) len[(size_t)b * (size_t)k + r] = tsearch_inf();
      if (tid == 0) {
        P::not_searched(value, info, (size_t)b);
        status[b] = 1;
      }
      continue;
    }
    for (int p = tid; p < N; p += T) s_route[p] = row[p];
    for (int r = tid; r < k; r += T) s_cap[r] = cap ? cap[r] : PF_FLEET_NO_CAP;
    if (tid == 0) s_at[k] = N;
    __syncthreads();
    // w(x, y) for two different nodes; w(x, e) where e may be "none" (-1) or x itself (an empty route's leg home in mode 1)
    auto w2 = [&](int x, int y) -> double {
      return x < y ? m[(size_t)x * (size_t)N + (size_t)y] : m[(size_t)y * (size_t)N + (size_t)x];
    };
    auto we = [&](int x, int e) -> double { return (e < 0 || e == x) ? 0.0 : w2(x, e); };
    // len[r] into s_rem[r] (the legs are filled, rem is not in use) and into keep[r] where the policy holds the lengths: a thread per
    // robot sums its legs in order, thread 0 the lengths
    auto lengths = [&](double& total, double& span, double* keep) {
      for (int r = tid; r < k; r += T) {
        double t = s_leg[s_at[r]];
        for (int p = s_at[r] + 1; p < s_at[r + 1]; ++p) t = t + s_leg[p];
        s_rem[r] = t;
        if (keep) keep[r] = t;
      }
      __syncthreads();
      if (tid == 0) {
        total = s_rem[0];
        span = s_rem[0];
        for (int r = 1; r < k; ++r) {
          total = total + s_rem[r];
          span = s_rem[r] > span ? s_rem[r] : span;
        }
      }
      __syncthreads();                          // (s_rem is rem's again)
    };
    double before = 0.0, after = 0.0, span0 = 0.0, span = 0.0;
    int moves = 0, sweeps = 0, two = 0, st = 2;
    P rule;
    for (int s = 0; s <= max_moves; ++s) {      // at most max_moves moves: at most max_moves + 1 sweeps; the loop ends by a break
      // the head of a sweep: the markers' positions; then rob, nxt and the leg of every position, cnt of every robot; then rem
      for (int p = tid; p < N; p += T)
        if (s_route[p] < k) s_at[s_route[p]] = p;
      __syncthreads();
      for (int p = tid; p < N; p += T) {
        int lo = 0, hi = k - 1;                 // the largest r with at[r] <= p (at[0] = 0)
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s_at[mid] <= p) lo = mid; else hi = mid - 1;
        }
        s_rob[p] = lo;
        const int f = p + 1 < N ? s_route[p + 1] : -1;
        const int e = f >= k ? f : (mode == 1 ? lo : -1);
        s_nxt[p] = e;
        s_leg[p] = we(s_route[p], e);
      }
      for (int r = tid; r < k; r += T) s_cnt[r] = s_at[r + 1] - s_at[r] - 1;
      __syncthreads();
      if (s == 0) lengths(before, span0, P::keep(s_p));
      for (int x = tid; x < 3 * N; x += T) {
        const int L = x / N + 1, i = x - (L - 1) * N, z = i + L - 1;
        double rem = __longlong_as_double(0x7FF8000000000000ll);
        if (i >= 1 && z < N && s_route[i] >= k && s_route[z] >= k && s_rob[i] == s_rob[z])
          rem = (s_leg[i - 1] + s_leg[z]) - we(s_route[i - 1], s_nxt[z]);
        s_rem[x] = rem;
      }
      __syncthreads();
      ++sweeps;
      rule.begin(s_p, k, tid);
      rule.reset();
      // code 0: the 2-opt pairs
      for (int c0 = tid; c0 < pairs; c0 += U * T) {
        double wac[U], wbe[U], old[U];
        int key[U], ri[U];
        bool open_end[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {           // every load is issued before the first is used: a slot past the end reads pair 0
          const int c = c0 + u * T;
          int i, j;
          tsearch_pair(c < pairs ? c : 0, N - 1, i, j);
          const int a = s_route[i - 1], bn = s_route[i], cn = s_route[j], e = s_nxt[j];
          const bool ok = c < pairs && bn >= k && cn >= k && s_rob[i] == s_rob[j];
          open_end[u] = e < 0;                  // w(b, none) = +0.0: some other node is read and dropped
          wac[u] = w2(a, cn);
          wbe[u] = w2(bn, open_end[u] ? a : e);
          old[u] = s_leg[i - 1] + s_leg[j];
          ri[u] = s_rob[i];
          key[u] = ok ? (i << 10) | j : PF_FLEET_NONE;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {           // ascending keys: a strict < keeps the first smallest
          const double d = (wac[u] + (open_end[u] ? 0.0 : wbe[u])) - old[u];
          if (key[u] != PF_FLEET_NONE) rule.take(s_p, d, 0.0, 0.0, 0.0, ri[u], ri[u], key[u]);
        }
      }
      // codes 1 .. 3: the relocations, cell c of the [3 N][N] grid = (L, i, j) with x = (L - 1) N + i = c / N, j = c % N
      {
        int x = tid / N, j = tid - x * N;
        for (int c0 = tid; c0 < cells; c0 += U * T) {
          double wps[U], wsq[U], old[U], rem[U], inner[U];
          int key[U], ri[U], rd[U];
          bool open_end[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool in = c0 + u * T < cells;
            const int xx = in ? x : 0, jj = in ? j : 0;               // a slot past the end reads the cell (1, 0, 0) and drops it
            const int L = xx >= 2 * N ? 3 : (xx >= N ? 2 : 1), i = xx - (L - 1) * N;
            const double r = s_rem[xx];
            bool ok = in && r == r && (jj < i - 1 || jj > i + L - 1);
            const int iz = ok ? i : 1 % N, zz = ok ? i + L - 1 : 1 % N;   // (an empty slot reads nodes of the row and drops them)
            const int s1 = s_route[iz], sL = s_route[zz], p = s_route[jj], q = s_nxt[jj];
            const int rj = s_rob[jj];
            ok = ok && (rj == s_rob[iz] || s_cnt[rj] + L <= s_cap[rj]);
            open_end[u] = q < 0 || q == sL;
            wps[u] = we(p, s1);
            wsq[u] = w2(sL, open_end[u] ? (sL ? 0 : 1 % N) : q);
            old[u] = s_leg[jj];
            rem[u] = r;
            inner[u] = L == 1 ? 0.0 : (L == 2 ? s_leg[iz] : s_leg[iz] + s_leg[zz - 1]);   // the segment's own legs (zz - 1 >= 0: iz >= 1)
            ri[u] = s_rob[iz];
            rd[u] = rj;
            key[u] = ok ? (L << 20) | (i << 10) | jj : PF_FLEET_NONE;
            j += T;                             // the thread's next cell
            while (j >= N) {
              j -= N;
              ++x;
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const double add = (wps[u] + (open_end[u] ? 0.0 : wsq[u])) - old[u];
            const double d = add - rem[u];
            if (key[u] != PF_FLEET_NONE) rule.take(s_p, d, rem[u], add, inner[u], ri[u], rd[u], key[u]);
          }
        }
      }
      rule.reduce(s_p, tid);
      if (!rule.improves()) { st = 0; break; }                        // (the same in every thread)
      if (moves == max_moves) { st = 2; break; }                      // a move is there and the cap forbids it
      const int dk = rule.key();
      const int code = dk >> 20, i = (dk >> 10) & 1023, j = dk & 1023;   // an evaluated candidate: its positions lie in the row
      rule.commit(s_p, s_rob[i], s_rob[j], tid);
      if (code == 0) {
        for (int t = tid; t < (j - i + 1) / 2; t += T) {
          const int v = s_route[i + t];
          s_route[i + t] = s_route[j - t];
          s_route[j - t] = v;
        }
        ++two;
      } else {
        // the stretch lo .. hi that changes: the segment first and what stood between behind it (j < i), or the other way round
        const int L = code, lo = j < i ? j + 1 : i, hi = j < i ? i + L - 1 : j, gap = hi - lo + 1 - L;
        for (int t = tid; t <= hi - lo; t += T)
          s_nxt[lo + t] = j < i ? (t < L ? s_route[i + t] : s_route[lo + t - L]) : (t < gap ? s_route[lo + L + t] : s_route[i + t - gap]);
        __syncthreads();
        for (int t = tid; t <= hi - lo; t += T) s_route[lo + t] = s_nxt[lo + t];
      }
      ++moves;
      __syncthreads();                          // (also: every thread has read the policy's words before the next sweep writes them)
    }
    lengths(after, span, nullptr);              // (no move since the legs were filled: they are the result's)
    for (int p = tid; p < N; p += T) row[p] = s_route[p];
    for (int r = tid; r < k; r += T) len[(size_t)b * (size_t)k + r] = s_rem[r];
    if (tid == 0) {
      rule.write(value, info, (size_t)b, before, span0, after, span, moves, sweeps, two);
      status[b] = st;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PF_FLEET_GROUP) void k_fleet_group_per_start(const double* __restrict__ mat, const int* __restrict__ has_inf, const int* __restrict__ cap, int mode,
                                                                          int k, int N, int B, int shared, int max_moves, int* route, double* __restrict__ len,
                                                                          double* __restrict__ value, int* __restrict__ status, long long* __restrict__ info) {
  fleet_group<fleet_sum>(mat, has_inf, cap, mode, k, N, B, shared, max_moves, route, len, value, status, info);
}

}  // namespace pf
