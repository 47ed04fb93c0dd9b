// pf_fleet_balance.h -- fleet routes under the min-max objective: the candidates of pf_fleet.h priced by the largest length they
// leave (pf_fleet_balance; include/pathfit.h holds the rule word for word).
//
// Rows, weights, nxt, capacities, the two candidate families, delta / rem / add, the LDS rows, the head of a sweep, the gathers and
// the move are fleet_group's (pf_fleet.h); this file is the policy it runs under.  The rule carries len[0 .. k - 1]: the
// left-to-right lengths of the start row, then the applied candidates' new lengths.  A candidate inside route r has
// len'[r] = fl(len[r] + delta); one from route s to route d has len'[s] = fl(fl(len[s] - rem) - inner) and
// len'[d] = fl(fl(len[d] + add) + inner), inner the length of the segment's own L - 1 legs, which change routes with it; its price
// span' is the largest of its new lengths and of len over the robots it does not touch.  The move of a sweep is the smallest
// (span', delta, code, i, j); it is applied iff span' < span, or span' == span and delta < 0, with span = max len.
// LDS beside fleet_group's rows: len[k], the three largest lengths with their robots, and the reduction's words.  The head of a
// sweep finds the three largest in three workgroup reductions over (length, robot), the larger length first and the smaller robot
// on a tie; the largest length outside a candidate's one or two robots is then the first of the three whose robot is not among them
// (-inf where there is none: k <= 2).  Only the VALUE picked enters span', and equal lengths have equal values, so which robot a tie
// names does not matter.  A thread keeps its best (span', delta, key) with the candidate's one or two new lengths; the
// workgroup's is found by lane exchanges and one exchange through LDS; thread 0 writes the new lengths into len[] when the move is
// applied, so the lengths priced are the lengths carried.  span' of the applied candidate is max len afterwards: span never rises.
// Every line is one fp64 operation on words that do not depend on the schedule (no multiplication: nothing can contract).
// Every index into len[] is s_rob[] of a position of the row, a robot in [0, k).
#pragma once

#include "pf_fleet.h"

namespace pf {

struct fleet_span {
  static constexpr int W = PF_FLEET_GROUP / 64, T = PF_FLEET_GROUP;
  struct Lds {
    double len[PF_FLEET_MAX];
    double rs[W], rv[W], ra[W], rb[W];
    int rk[W];
  };
  double t0, t1, t2;                            // the three largest lengths, -inf where there are fewer robots
  int w0, w1, w2;                               // their robots, -1 where there is none
  double bs, bd, ba, bb;                        // the best candidate: span', delta, len' of rob(i) and of rob(j)
  int bk;
  int lowered = 0;
  static __device__ __forceinline__ double neg_inf() { return __longlong_as_double((long long)0xFFF0000000000000ull); }
  static __device__ __forceinline__ double larger(double x, double y) { return x > y ? x : y; }
  static __device__ __forceinline__ double* keep(Lds& s) { return s.len; }
  // (length, robot) x before y: the larger length, the smaller robot on a tie
  static __device__ __forceinline__ bool above(double xv, int xr, double yv, int yr) { return xv > yv || (xv == yv && xr < yr); }
  // the largest len[r] over the robots other than skip0 and skip1, with its robot (PF_FLEET_NONE with -inf where there is none)
  __device__ __forceinline__ void largest(Lds& s, int k, int tid, int skip0, int skip1, double& v, int& r) {
    v = neg_inf();
    r = PF_FLEET_NONE;
    for (int q = tid; q < k; q += T) {
      const double x = s.len[q];
      if (q != skip0 && q != skip1 && above(x, q, v, r)) {
        v = x;
        r = q;
      }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const double qv = __shfl_xor(v, o);
      const int qr = __shfl_xor(r, o);
      if (above(qv, qr, v, r)) {
        v = qv;
        r = qr;
      }
    }
    if ((tid & 63) == 0) {
      s.rv[tid >> 6] = v;
      s.rk[tid >> 6] = r;
    }
    __syncthreads();
    v = s.rv[0];
    r = s.rk[0];
#pragma unroll
    for (int q = 1; q < W; ++q) {
      const double qv = s.rv[q];
      const int qr = s.rk[q];
      if (above(qv, qr, v, r)) {
        v = qv;
        r = qr;
      }
    }
    __syncthreads();                            // (every thread has read the words before they are written again)
    if (r == PF_FLEET_NONE) r = -1;
  }
  __device__ __forceinline__ void begin(Lds& s, int k, int tid) {
    largest(s, k, tid, -1, -1, t0, w0);
    largest(s, k, tid, w0, -1, t1, w1);
    largest(s, k, tid, w0, w1, t2, w2);
  }
  __device__ __forceinline__ void reset() {
    bs = tsearch_inf();
    bd = tsearch_inf();
    ba = 0.0;
    bb = 0.0;
    bk = PF_FLEET_NONE;
  }
  // the largest length over the robots other than x and y: at most two of the three are skipped
  __device__ __forceinline__ double others(int x, int y) const {
    return (w0 != x && w0 != y) ? t0 : ((w1 != x && w1 != y) ? t1 : t2);
  }
  __device__ __forceinline__ void take(const Lds& s, double d, double rem, double add, double inner, int ri, int rj, int key) {
    double a, b;
    if (ri == rj) {
      a = s.len[ri] + d;
      b = a;
    } else {
      a = (s.len[ri] - rem) - inner;
      b = (s.len[rj] + add) + inner;
    }
    const double sp = larger(larger(a, b), others(ri, rj));
    if (sp < bs || (sp == bs && d < bd)) {      // ascending keys: a strict < keeps the first smallest
      bs = sp;
      bd = d;
      ba = a;
      bb = b;
      bk = key;
    }
  }
  static __device__ __forceinline__ bool before(double xs, double xd, int xk, double ys, double yd, int yk) {
    return xs < ys || (xs == ys && (xd < yd || (xd == yd && xk < yk)));
  }
  __device__ __forceinline__ void reduce(Lds& s, int tid) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const double qs = __shfl_xor(bs, o), qd = __shfl_xor(bd, o), qa = __shfl_xor(ba, o), qb = __shfl_xor(bb, o);
      const int qk = __shfl_xor(bk, o);
      if (before(qs, qd, qk, bs, bd, bk)) {
        bs = qs;
        bd = qd;
        ba = qa;
        bb = qb;
        bk = qk;
      }
    }
    if ((tid & 63) == 0) {
      const int q = tid >> 6;
      s.rs[q] = bs;
      s.rv[q] = bd;
      s.ra[q] = ba;
      s.rb[q] = bb;
      s.rk[q] = bk;
    }
    __syncthreads();
    int at = 0;
    bs = s.rs[0];
    bd = s.rv[0];
    bk = s.rk[0];
#pragma unroll
    for (int q = 1; q < W; ++q) {
      const double qs = s.rs[q], qd = s.rv[q];
      const int qk = s.rk[q];
      if (before(qs, qd, qk, bs, bd, bk)) {
        bs = qs;
        bd = qd;
        bk = qk;
        at = q;
      }
    }
    ba = s.ra[at];
    bb = s.rb[at];
  }
  // span = max len = t0 (the same in every thread)
  __device__ __forceinline__ bool improves() const { return bk != PF_FLEET_NONE && (bs < t0 || (bs == t0 && bd < 0.0)); }
  __device__ __forceinline__ int key() const { return bk; }
  __device__ __forceinline__ void commit(Lds& s, int ri, int rj, int tid) {
    if (tid == 0) {                             // (read again by the next sweep, behind its barriers)
      s.len[ri] = ba;
      if (rj != ri) s.len[rj] = bb;
    }
    lowered += bs < t0;
  }
  static __device__ __forceinline__ void not_searched(double* value, long long* info, size_t b) {
    for (int x = 0; x < 4; ++x) value[b * 4 + x] = tsearch_inf();
    if (info)
      for (int x = 0; x < 5; ++x) info[b * 5 + x] = 0;
  }
  __device__ __forceinline__ void write(double* value, long long* info, size_t b, double before, double span0, double after, double span, int moves, int sweeps,
                                        int two) const {
    value[b * 4] = span;
    value[b * 4 + 1] = after;
    value[b * 4 + 2] = span0;
    value[b * 4 + 3] = before;
    if (info) {
      info[b * 5] = moves;
      info[b * 5 + 1] = sweeps;
      info[b * 5 + 2] = two;
      info[b * 5 + 3] = moves - two;
      info[b * 5 + 4] = lowered;
    }
  }
};

__global__ __launch_bounds__(PF_FLEET_GROUP) void k_fleet_balance_group_per_start(const double* __restrict__ mat, const int* __restrict__ has_inf, const int* __restrict__ cap,
                                                                                  int mode, int k, int N, int B, int shared, int max_moves, int* route,
                                                                                  double* __restrict__ len, double* __restrict__ value, int* __restrict__ status,
                                                                                  long long* __restrict__ info) {
  fleet_group<fleet_span>(mat, has_inf, cap, mode, k, N, B, shared, max_moves, route, len, value, status, info);
}

}  // namespace pf
