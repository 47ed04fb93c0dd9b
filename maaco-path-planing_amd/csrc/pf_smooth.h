// pf_smooth.h -- any-angle smoothing: line-of-sight tests between cell centres and forward string pulling over path rows
// (pf_line_of_sight_batch, pf_smooth_batch).
//
// The rule, in integers.  a = (r0, c0), b = (r1, c1), dr = r1 - r0, dc = c1 - c0, s = |dr| + |dc|.  For a cell (r, c) of the
// bounding box, k = dr (c - c0) - dc (r - r0): the cell is CROSSED iff |2k| < s and TOUCHED (met in a corner point only) iff
// |2k| == s.  visible(a, b, strict) iff no crossed cell is an obstacle and, when strict, no touched one either; a == b is
// visible iff the cell is free.
//
// The mapping.  Major axis: columns if |dc| >= |dr|, else rows; B = the major extent, A = the minor one (A <= B).  At major
// offset t (0 .. B) and minor offset u (0 .. A), both counted from a towards b, |k| = |A t - B u|.  With q = floor(A t / B) and
// rem = A t - q B in [0, B):  u = q gives rem, u = q + 1 gives rem - B, u = q - 1 gives rem + B >= B >= s / 2 (a touch at best,
// and only on a pure diagonal), and any u further away gives |k| > B >= s / 2.  So a major index holds at most THREE cells that
// count, u in {q - 1, q, q + 1}, and a lane that owns one major index loads at most three occupancy bytes.  q comes from one
// float multiply with the reciprocal of B and one correction step: A t <= 4095^2 < 2^24 is exact in fp32, and the product is off by
// less than 4095 * 2^-22, so the truncated quotient is off by at most one.
//
// First blocker: the major index nearest a that holds a blocking cell is the lowest lane of the first pass whose ballot is not
// empty; among that index's blocking cells the smallest r C + c is taken inside the lane.
//
// k_line_of_sight_pairs_lanes_on_major: one wavefront per pair, lane i takes major offset 64 pass + i, stops at the first pass with a blocker.
// k_smooth_paths_one_wave_per_row: one wavefront (a workgroup of its own, so short paths retire early) per path.  The rule is sequential in the
// anchor only: while the anchor a stands, the tests p[j + 1], p[j + 2], ... are known in advance.  PF_SMOOTH_SPEC = 1 packs the
// (candidate, major offset) pairs of as many consecutive candidates as fit into the 64 lanes of one pass; the first failing
// candidate (the lowest blocked lane: lanes are ordered by candidate) decides and the later ones are discarded, which is the
// plain loop's answer by construction.  A candidate PF_SMOOTH_PACK_SPAN major indices away or more is tested alone, pass by pass.  PF_SMOOTH_SPEC = 0 is the
// plain form: one test at a time.  The input row is read from memory per test (L2); nothing is staged in LDS.
#pragma once

namespace pf {

#ifndef PF_SMOOTH_SPEC
#define PF_SMOOTH_SPEC 1
#endif
#ifndef PF_SMOOTH_PACK_SPAN
#define PF_SMOOTH_PACK_SPAN 32                  /* a candidate this many major indices away, or more, is tested alone: two such do not share 64 lanes */
#endif
#define PF_SM_NONE 0x7FFFFFFF
#define PF_SM_ST_OK 0
#define PF_SM_ST_BAD 1
#define PF_SM_ST_OVERFLOW 3

// The blocking cell of smallest id at major offset t of the segment (r0, c0) -> cell b, or PF_SM_NONE.  t <= B is the caller's.
__device__ __forceinline__ int sm_lane_blocker(const uint8_t* __restrict__ occ, int C, int r0, int c0, int b, int t, int strict) {
  const int r1 = b / C, c1 = b - r1 * C;
  const int dr = r1 - r0, dc = c1 - c0;
  const int adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
  const bool colmaj = adc >= adr;
  const int A = colmaj ? adr : adc, B = colmaj ? adc : adr, s = A + B;
  const int a = r0 * C + c0;
  if (B == 0) return occ[a] == 1 ? a : PF_SM_NONE;                   // a == b
  const int sr = dr < 0 ? -1 : 1, sc = dc < 0 ? -1 : 1;
  const int stepmaj = colmaj ? sc : sr * C, stepmin = colmaj ? sr * C : sc;
  const int n = A * t;
  int q = (int)((float)n * __builtin_amdgcn_rcpf((float)B));
  int rem = n - q * B;
  if (rem < 0) { q -= 1; rem += B; } else if (rem >= B) { q += 1; rem -= B; }
  const int base = a + t * stepmaj;
  int best = PF_SM_NONE;
#pragma unroll
  for (int d = -1; d <= 1; ++d) {
    const int u = q + d;
    int e2 = 2 * (rem - d * B);
    e2 = e2 < 0 ? -e2 : e2;
    if (u < 0 || u > A || !(e2 < s || (strict && e2 == s))) continue;
    const int cell = base + u * stepmin;
    if (occ[cell] == 1 && cell < best) best = cell;
  }
  return best;
}

// first_block of the pair (a, b), both inside the grid: wave-wide, every lane returns the same value; -1 = visible
__device__ __forceinline__ int sm_first_block(const uint8_t* __restrict__ occ, int C, int a, int b, int strict, int lane) {
  const int r0 = a / C, c0 = a - r0 * C, r1 = b / C, c1 = b - r1 * C;
  const int adr = r1 < r0 ? r0 - r1 : r1 - r0, adc = c1 < c0 ? c0 - c1 : c1 - c0;
  const int B = adc >= adr ? adc : adr;
  for (int t0 = 0; t0 <= B; t0 += 64) {
    const int t = t0 + lane;
    const int best = t <= B ? sm_lane_blocker(occ, C, r0, c0, b, t, strict) : PF_SM_NONE;
    const unsigned long long m = __ballot(best != PF_SM_NONE);
    if (m) return __shfl(best, __ffsll((long long)m) - 1);
  }
  return -1;
}

__global__ __launch_bounds__(64) void k_line_of_sight_pairs_lanes_on_major(const uint8_t* __restrict__ occ, int RC, int C, int strict, int n, const int* __restrict__ from,
                                                            const int* __restrict__ to, int* __restrict__ vis, int* __restrict__ fblock) {
  const int q = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (q >= n) return;
  const int a = from[q], b = to[q];
  int v = 0, f = -1;
  if ((unsigned)a < (unsigned)RC && (unsigned)b < (unsigned)RC) {
    f = sm_first_block(occ, C, a, b, strict, lane);
    v = f < 0;
  }
  if (lane == 0) {
    vis[q] = v;
    if (fblock) fblock[q] = f;
  }
}

// the waypoints of one path as they are found: the row, the count, the stats (the same values in every lane)
struct SmOut {
  int* way; int* idx; int cap; int cnt;
  int pr, pc, pdr, pdc;
  double length; int turns;
};

__device__ __forceinline__ void sm_emit(SmOut& o, int i, int cell, int C, int lane) {
  if (o.cnt < o.cap && lane == 0) {
    o.way[o.cnt] = cell;
    if (o.idx) o.idx[o.cnt] = i;
  }
  const int r = cell / C, c = cell - r * C;
  if (o.cnt > 0) {
    const int dr = r - o.pr, dc = c - o.pc;
    o.length = o.length + __builtin_sqrt((double)(dr * dr + dc * dc));
    if (o.cnt > 1 && (o.pdr * dc - o.pdc * dr != 0 || o.pdr * dr + o.pdc * dc < 0)) o.turns += 1;
    o.pdr = dr; o.pdc = dc;
  }
  o.pr = r; o.pc = c;
  o.cnt += 1;
}

__global__ __launch_bounds__(64) void k_smooth_paths_one_wave_per_row(const uint8_t* __restrict__ occ, int RC, int C, int strict, int n, int path_cap,
                                                     const int* __restrict__ cells, const int* __restrict__ len, int way_cap, int* __restrict__ way_cells,
                                                     int* __restrict__ way_idx, int* __restrict__ way_len, double* __restrict__ stats,
                                                     int* __restrict__ status) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (p >= n) return;
  const int L = len[p];
  const int* const row = cells + (size_t)p * (size_t)path_cap;
  bool bad = L < 1 || L > path_cap;
  if (!bad) {
    int off = 0;
    for (int i = lane; i < L; i += 64) off |= (unsigned)row[i] >= (unsigned)RC;
    bad = __ballot(off) != 0ull;
  }
  SmOut o;
  o.way = way_cells + (size_t)p * (size_t)way_cap;
  o.idx = way_idx ? way_idx + (size_t)p * (size_t)way_cap : nullptr;
  o.cap = way_cap; o.cnt = 0; o.pr = o.pc = o.pdr = o.pdc = 0; o.length = 0.0; o.turns = 0;
  int st = PF_SM_ST_BAD;
  if (!bad) {
    int ca = row[0];
    [[maybe_unused]] int ra = ca / C, cca = ca - ra * C;
    sm_emit(o, 0, ca, C, lane);
    int j = 1;
    while (j + 1 < L) {
      bool fail;
      const int nb = row[j + 1];
#if PF_SMOOTH_SPEC
      const int nr = nb / C, nc = nb - nr * C;
      const int ndr = nr < ra ? ra - nr : nr - ra, ndc = nc < cca ? cca - nc : nc - cca;
      if ((ndc >= ndr ? ndc : ndr) < PF_SMOOTH_PACK_SPAN) {           // the next candidate is near: it and its successors share a pass
        // candidates j + 1 + lane: spans, their running sum, the ones that fit into this pass (the first one does)
        const int ci = j + 1 + lane;
        const int cc = ci < L ? row[ci] : 0;
        int span = 65;
        if (ci < L) {
          const int r1 = cc / C, c1 = cc - r1 * C;
          const int adr = r1 < ra ? ra - r1 : r1 - ra, adc = c1 < cca ? cca - c1 : c1 - cca;
          span = (adc >= adr ? adc : adr) + 1;
        }
        int incl = span;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        const int nfit = __popcll(__ballot(incl <= 64));           // (the sums grow: the fitting candidates are a prefix)
        int cand = 0;
        for (int i = 0; i < nfit; ++i) cand += lane >= __builtin_amdgcn_readlane(incl, i);
        const int b = __shfl(cc, cand), t = lane - (__shfl(incl, cand) - __shfl(span, cand));
        const int best = cand < nfit ? sm_lane_blocker(occ, C, ra, cca, b, t, strict) : PF_SM_NONE;
        const unsigned long long m = __ballot(best != PF_SM_NONE);
        if (m) { j += __shfl(cand, __ffsll((long long)m) - 1); fail = true; }
        else { j += nfit; fail = false; }
      } else
#endif
      {
        fail = sm_first_block(occ, C, ca, nb, strict, lane) >= 0;
        if (!fail) j += 1;
      }
      if (fail) {                                                    // p[j + 1] is out of sight: p[j] is kept and becomes the anchor
        ca = row[j]; ra = ca / C; cca = ca - ra * C;
        sm_emit(o, j, ca, C, lane);
        j += 1;
      }
    }
    if (L > 1) sm_emit(o, L - 1, row[L - 1], C, lane);
    st = o.cnt > way_cap ? PF_SM_ST_OVERFLOW : PF_SM_ST_OK;
  }
  if (lane == 0) {
    const bool ok = st == PF_SM_ST_OK;
    way_len[p] = ok ? o.cnt : 0;
    status[p] = st;
    if (stats) { stats[2 * (size_t)p] = ok ? o.length : 0.0; stats[2 * (size_t)p + 1] = ok ? (double)o.turns : 0.0; }
  }
}

}  // namespace pf
