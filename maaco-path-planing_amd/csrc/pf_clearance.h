// pf_clearance.h -- clearance fields: the exact squared Euclidean distance from every cell to the nearest obstacle cell, the
// nearest obstacle itself, and the margins of path rows and straight segments read off that field
// (pf_clearance_field, pf_clearance_paths, pf_clearance_segments).  Everything is integer and exact.
//
// The rule.  d2[v] = min over the obstacle cells o (occupancy byte 1) of (rv - ro)^2 + (cv - co)^2, 0 on an obstacle,
// PF_CLEAR_NONE on a map without one; with `border` the cells just outside the grid count too, so min(r + 1, R - r, c + 1, C - c)^2
// takes part in the minimum.  near[v] = the obstacle cell inside the grid that attains the minimum WITHOUT the border, the
// smallest r C + c on a tie, -1 on a map without an obstacle: `border` changes d2 only, never near.
//
// The transform is separable.  Row pass: dcol[r][c] = the signed column offset from c to the nearest obstacle of row r (<= 0 to
// the left, PF_CLEAR_NONE in a row without one); an equal |offset| takes the left one.  Column pass: d2[r][c] = min over r' of
// (r' - r)^2 + dcol[r'][c]^2; an equal sum takes the lowest r'.  The tie rule: an obstacle of row r' at minimum distance from
// (r, c) is at the minimum |offset| of its row, where at most two obstacles stand and the left one has the smaller id; among the
// rows that attain the minimum the lowest one holds the smaller ids.  So the pair (lowest row, left obstacle) is the smallest id.
//
//   k_clear_rows_nearest_in_row     one wavefront per row, 64 cells per trip: the ballot of "is an obstacle" is one 64-bit word; the
//                                   nearest set bit at or below a lane is a leading-zero count of the word masked to the lane, the
//                                   nearest at or above it a trailing-zero count of the word shifted by the lane; the column of the
//                                   last obstacle of the words behind is the carry.  One sweep left to right (leaves the left
//                                   column in the lane's own output word), one right to left (reads it back, picks, writes dcol).
//   k_clear_cols_outward_scan       one thread per cell, the 64 lanes of a wavefront along a row (loads coalesce): rows r - k and
//                                   r + k for k = 1, 2, ... while k^2 <= the best sum so far, at most scan_rows steps.  A
//                                   cell the bound did not close within that many steps raises its column's flag.
//   k_clear_cols_lower_envelope     one thread per FLAGGED column, the lanes along a row: the lower envelope of the parabolas
//                                   (r - r')^2 + dcol[r'][c]^2 in exact integers (Felzenszwalb-Huttenlocher; the crossing point
//                                   of two parabolas is kept as the first integer row from which the later one is STRICTLY
//                                   smaller, a floor division), a stack of (row, first row) pairs per column in scratch, then one
//                                   walk down the column.  O(R) per column whatever the clearance.  It rewrites the whole column
//                                   with the same values the scan would have reached: both passes compute the minimum and the
//                                   same tie rule, so which one wrote a word cannot be seen.
//   k_clear_info_reduce / k_clear_write_info_block   the obstacle cells, and the largest d2 over the free cells with the smallest id
//                                   that attains it as one 64-bit atomic max of (d2 << 32) | ~id.
// -DPF_CLEAR_SCAN_ROWS=0 is the pure envelope form, a value >= R the pure scan; the shipped -1 takes clear_scan_rows(C): a dense
// map never starts an envelope thread and an open one never scans further than that many rows (DESIGN.md 4.16 has the probe table).
//
//   k_clear_paths_one_wave_per_row  one wavefront per path row: the lanes stride over the cells, gather d2, and one reduction
//                                   of the packed key (d2 << 32) | position gives the minimum and its first position.
//   k_clear_segments_lanes_on_major one wavefront per pair, lane i on major offset 64 pass + i: the rule and the three candidate
//                                   cells per major index are pf_smooth.h's (|2k| < s crossed, |2k| == s touched); the key is
//                                   (d2 << 32) | cell, so the smallest id wins a tie.  The quotient is an integer division here.
//
// No kernel reads a word another workgroup writes in the same launch (the column flags are written as the constant 1 and read
// in the next launch); kernel boundaries are the only synchronisation.
#pragma once

namespace pf {

#ifndef PF_CLEAR_SCAN_ROWS
#define PF_CLEAR_SCAN_ROWS -1                   /* rows the outward scan looks each way before it hands the column to the envelope pass; -1: clear_scan_rows(C) */
#endif
#define PF_CL_THREADS 256
#define PF_CL_AHEAD 8                           /* rows whose loads the envelope pass has in flight before it works on its stack */
#define PF_CL_CTL_WORDS 2                       /* control block (64-bit words): [0] the largest (d2, ~id) key, [1] obstacle cells */

// The scan's reach by measurement: one scan step over the whole map costs about 1.2 ns per cell, the envelope pass
// about 0.33 us per row whatever the width, so the scan has spent what an envelope pass costs after about 2^18 / C steps.
static inline int clear_scan_rows(int C) {
  if (PF_CLEAR_SCAN_ROWS >= 0) return PF_CLEAR_SCAN_ROWS;
  const int k = (1 << 18) / C;
  return k < 32 ? 32 : k;
}

__device__ __forceinline__ int clear_with_border(int d2, int r, int c, int R, int C, int border) {
  if (!border) return d2;
  int m = r + 1 < R - r ? r + 1 : R - r;
  const int mc = c + 1 < C - c ? c + 1 : C - c;
  m = m < mc ? m : mc;
  return m * m < d2 ? m * m : d2;
}

__global__ __launch_bounds__(PF_CL_THREADS) void k_clear_rows_nearest_in_row(const uint8_t* __restrict__ occ, int R, int C, int* dcol) {
  const int lane = (int)(threadIdx.x & 63u);
  const int r = (int)(blockIdx.x * (PF_CL_THREADS / 64) + (threadIdx.x >> 6));
  if (r >= R) return;                                                // (the whole wavefront)
  const uint8_t* const row = occ + (size_t)r * (size_t)C;
  int* const out = dcol + (size_t)r * (size_t)C;
  int carry = -1;                                                    // the column of the last obstacle in the words behind
  for (int base = 0; base < C; base += 64) {
    const int c = base + lane;
    const unsigned long long m = __ballot(c < C && row[c] == 1);
    const unsigned long long ml = m & (~0ull >> (63 - lane));
    if (c < C) out[c] = ml ? base + 63 - __clzll((long long)ml) : carry;
    if (m) carry = base + 63 - __clzll((long long)m);
  }
  carry = -1;                                                        // ... and of the first obstacle in the words ahead
  for (int base = ((C - 1) / 64) * 64; base >= 0; base -= 64) {
    const int c = base + lane;
    const unsigned long long m = __ballot(c < C && row[c] == 1);
    const unsigned long long mr = m >> lane;
    const int right = mr ? c + __ffsll((long long)mr) - 1 : carry;
    if (c < C) {
      const int left = out[c];                                       // this lane's own word of the first sweep
      int d = PF_CLEAR_NONE;
      if (left >= 0) d = left - c;
      if (right >= 0 && (left < 0 || right - c < c - left)) d = right - c;
      out[c] = d;
    }
    if (m) carry = base + __ffsll((long long)m) - 1;
  }
}

__global__ __launch_bounds__(PF_CL_THREADS) void k_clear_cols_outward_scan(const int* __restrict__ dcol, int R, int C, int border, int scan_rows, int* __restrict__ d2,
                                                                          int* __restrict__ near, int* __restrict__ colflag) {
  const int c = (int)(blockIdx.x * 64 + (threadIdx.x & 63u));
  const int r = (int)(blockIdx.y * (PF_CL_THREADS / 64) + (threadIdx.x >> 6));
  if (c >= C || r >= R) return;
  const int* const col = dcol + c;
  int best = PF_CLEAR_NONE, brow = -1, bd = 0;
  {
    const int d = col[(size_t)r * (size_t)C];
    if (d != PF_CLEAR_NONE) { best = d * d; brow = r; bd = d; }
  }
  int k = 1;
  for (; k <= scan_rows && k * k <= best && (r - k >= 0 || r + k < R); ++k) {
    if (r - k >= 0) {                                                // a row above holds smaller ids than every row seen so far: it wins a tie
      const int d = col[(size_t)(r - k) * (size_t)C];
      if (d != PF_CLEAR_NONE && k * k + d * d <= best) { best = k * k + d * d; brow = r - k; bd = d; }
    }
    if (r + k < R) {
      const int d = col[(size_t)(r + k) * (size_t)C];
      if (d != PF_CLEAR_NONE && k * k + d * d < best) { best = k * k + d * d; brow = r + k; bd = d; }
    }
  }
  if (k * k <= best && (r - k >= 0 || r + k < R)) colflag[c] = 1;    // not closed: the envelope pass takes the column
  const size_t v = (size_t)r * (size_t)C + (size_t)c;
  d2[v] = clear_with_border(best, r, c, R, C, border);
  if (near) near[v] = brow < 0 ? -1 : brow * C + c + bd;
}

__global__ __launch_bounds__(64) void k_clear_cols_lower_envelope(const int* __restrict__ dcol, int R, int C, int border, const int* __restrict__ colflag,
                                                                 int2* __restrict__ stack, int* __restrict__ d2, int* __restrict__ near) {
  const int c = (int)(blockIdx.x * 64 + threadIdx.x);
  if (c >= C || !colflag[c]) return;
  const int* const col = dcol + c;
  int2* const st = stack + c;                                        // entry k at st[k C]: {row, the first row it holds}
  constexpr int LOWEST = -0x7FFFFFFF - 1;
  int n = 0, tv = 0, tz = LOWEST, tf = 0;                            // the entries, and the top one: row, first row, dcol^2
  for (int q0 = 0; q0 < R; q0 += PF_CL_AHEAD) {
    int ahead[PF_CL_AHEAD];                                          // the loads of PF_CL_AHEAD rows are in flight together; the stack work follows
#pragma unroll
    for (int j = 0; j < PF_CL_AHEAD; ++j) ahead[j] = q0 + j < R ? col[(size_t)(q0 + j) * (size_t)C] : PF_CLEAR_NONE;
#pragma unroll
    for (int j = 0; j < PF_CL_AHEAD; ++j) {
      const int q = q0 + j, d = ahead[j];
      if (d == PF_CLEAR_NONE) continue;
      const int fq = d * d;
      int z = LOWEST;
      while (n > 0) {
        // the first row from which q's parabola is strictly below the top one's: floor(num / den) + 1  (den > 0, |num| <= R^2 + C^2)
        const int num = (fq + q * q) - (tf + tv * tv), den = 2 * (q - tv);
        int s = num / den;
        if (num < 0 && s * den != num) s -= 1;
        z = s + 1;
        if (z > tz) break;
        n -= 1;                                                      // the top entry holds no row any more
        z = LOWEST;
        if (n > 0) {
          const int2 e = st[(size_t)(n - 1) * (size_t)C];
          const int dd = col[(size_t)e.x * (size_t)C];
          tv = e.x; tz = e.y; tf = dd * dd;
        }
      }
      if (z >= R) continue;                                          // q would hold rows beyond the grid only
      st[(size_t)n * (size_t)C] = make_int2(q, z);
      n += 1; tv = q; tz = z; tf = fq;
    }
  }
  int k = 0, cv = 0, cd = 0, nz = R;                                 // the entry in use: its row, its dcol; the first row of the next one
  if (n > 0) {
    cv = st[0].x; cd = col[(size_t)cv * (size_t)C];
    if (n > 1) nz = st[(size_t)C].y;
  }
  for (int r = 0; r < R; ++r) {
    int best = PF_CLEAR_NONE, nr = -1;
    if (n > 0) {
      while (nz <= r) {
        k += 1;
        cv = st[(size_t)k * (size_t)C].x; cd = col[(size_t)cv * (size_t)C];
        nz = k + 1 < n ? st[(size_t)(k + 1) * (size_t)C].y : R;
      }
      best = (r - cv) * (r - cv) + cd * cd;
      nr = cv * C + c + cd;
    }
    const size_t v = (size_t)r * (size_t)C + (size_t)c;
    d2[v] = clear_with_border(best, r, c, R, C, border);
    if (near) near[v] = nr;
  }
}

__global__ __launch_bounds__(PF_CL_THREADS) void k_clear_info_reduce(const uint8_t* __restrict__ occ, const int* __restrict__ d2, int RC, unsigned long long* __restrict__ ctl) {
  unsigned long long best = 0ull;                                    // (a free cell's d2 is >= 1: its key is never 0)
  int obst = 0;
  for (int v = (int)(blockIdx.x * PF_CL_THREADS + threadIdx.x); v < RC; v += (int)(gridDim.x * PF_CL_THREADS)) {
    if (occ[v] == 1) { obst += 1; continue; }
    const unsigned long long key = ((unsigned long long)(unsigned)d2[v] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    best = o > best ? o : best;
    obst += __shfl_xor(obst, d);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (best) atomicMax(ctl, best);
    if (obst) atomicAdd(ctl + 1, (unsigned long long)obst);
  }
}

__global__ void k_clear_write_info_block(const unsigned long long* __restrict__ ctl, int RC, long long* __restrict__ info) {
  if (blockIdx.x || threadIdx.x) return;
  const long long obst = (long long)ctl[1];
  info[0] = obst;
  info[1] = (long long)RC - obst;
  info[2] = obst < RC ? (long long)(ctl[0] >> 32) : -1;
  info[3] = obst < RC ? (long long)(0xFFFFFFFFu - (unsigned)(ctl[0] & 0xFFFFFFFFull)) : -1;
}

__global__ __launch_bounds__(64) void k_clear_paths_one_wave_per_row(const int* __restrict__ d2, int RC, int n, int path_cap, const int* __restrict__ cells,
                                                                    const int* __restrict__ len, int margin_d2, int* __restrict__ out, int* __restrict__ profile,
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
  unsigned long long best = ~0ull;                                   // (d2 << 32) | position
  int below = 0, first = 0x7FFFFFFF;
  if (!bad) {
    int* const prof = profile ? profile + (size_t)p * (size_t)path_cap : nullptr;
    for (int i = lane; i < L; i += 64) {
      const int v = d2[row[i]];
      if (prof) prof[i] = v;
      const unsigned long long key = ((unsigned long long)(unsigned)v << 32) | (unsigned long long)(unsigned)i;
      best = key < best ? key : best;
      if (v < margin_d2) { below += 1; first = i < first ? i : first; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(best, d);
      best = o < best ? o : best;
      below += __shfl_xor(below, d);
      const int f = __shfl_xor(first, d);
      first = f < first ? f : first;
    }
  }
  if (lane == 0) {
    int* const o = out + 4 * (size_t)p;
    o[0] = bad ? PF_CLEAR_NONE : (int)(best >> 32);
    o[1] = bad ? -1 : (int)(best & 0xFFFFFFFFull);
    o[2] = bad ? 0 : below;
    o[3] = bad || !below ? -1 : first;
    status[p] = bad ? 1 : 0;
  }
}

__global__ __launch_bounds__(64) void k_clear_segments_lanes_on_major(const int* __restrict__ d2, int RC, int C, int touched, int n, const int* __restrict__ from,
                                                                     const int* __restrict__ to, int* __restrict__ dmin, int* __restrict__ dat) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (p >= n) return;
  const int a = from[p], b = to[p];
  unsigned long long best = ~0ull;                                   // (d2 << 32) | cell
  const bool inside = (unsigned)a < (unsigned)RC && (unsigned)b < (unsigned)RC;
  if (inside) {
    const int r0 = a / C, c0 = a - r0 * C, r1 = b / C, c1 = b - r1 * C;
    const int dr = r1 - r0, dc = c1 - c0;
    const int adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
    const bool colmaj = adc >= adr;
    const int A = colmaj ? adr : adc, B = colmaj ? adc : adr, s = A + B;
    if (B == 0) {
      best = ((unsigned long long)(unsigned)d2[a] << 32) | (unsigned long long)(unsigned)a;
    } else {
      const int sr = dr < 0 ? -1 : 1, sc = dc < 0 ? -1 : 1;
      const int stepmaj = colmaj ? sc : sr * C, stepmin = colmaj ? sr * C : sc;
      for (int t = lane; t <= B; t += 64) {
        const int nn = A * t, q = nn / B, rem = nn - q * B;           // minor offset q holds |k| = rem, q + 1 holds B - rem, q - 1 holds rem + B
#pragma unroll
        for (int d = -1; d <= 1; ++d) {
          const int u = q + d;
          int e2 = 2 * (rem - d * B);
          e2 = e2 < 0 ? -e2 : e2;
          if (u < 0 || u > A || !(e2 < s || (touched && e2 == s))) continue;
          const int cell = a + t * stepmaj + u * stepmin;
          const unsigned long long key = ((unsigned long long)(unsigned)d2[cell] << 32) | (unsigned long long)(unsigned)cell;
          best = key < best ? key : best;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d);
        best = o < best ? o : best;
      }
    }
  }
  if (lane == 0) {
    dmin[p] = inside ? (int)(best >> 32) : PF_CLEAR_NONE;
    if (dat) dat[p] = inside ? (int)(best & 0xFFFFFFFFull) : -1;
  }
}

}  // namespace pf
