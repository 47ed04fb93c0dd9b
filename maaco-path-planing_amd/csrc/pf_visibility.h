// pf_visibility.h -- visibility fields: what each viewpoint sees, exposure counts over a set of viewpoints and the exposure of
// path rows (pf_visibility_field, pf_visibility_count, pf_visibility_paths).
//
// The rule is pf_smooth.h's visible(a, b, strict), evaluated one-to-all: for the viewpoint a and a target b, the cells of the
// bounding box with |2k| < s are crossed and those with |2k| == s touched; b is seen iff no crossed cell is an obstacle and, when
// strict, no touched one either.  The endpoints are crossed, so an obstacle is never seen and a viewpoint on one sees nothing.
// A target further than max_range_sq (dr^2 + dc^2, integers) is not seen; max_range_sq < 0 means no limit.
//
// The mapping shipped (PF_VIS_WAVE_PER_TARGET = 0): ONE LANE PER TARGET, the 64 lanes of a wavefront on 64 consecutive cell ids.
// A lane walks its own sight line from the viewpoint, PF_VIS_TRIPS major indices a trip, and leaves at the first trip with a
// blocker; a target on an obstacle, outside the range disc or behind a viewpoint on an obstacle does no walk at all.  The
// remainder of pf_smooth.h's mapping is carried from index to index (rem += A, one conditional subtraction: no division, no
// multiply), and so is the cell id; an index tests at most three bytes: u = q (|2k| = 2 rem), u = q + 1 (2 (B - rem)) and, on a
// pure diagonal under the strict rule only, u = q - 1 (2 (rem + B) == s iff rem == 0 and A == B).  No load is conditional: a
// cell that does not count is replaced by the viewpoint's own cell, which is free, so all loads of a trip are in flight together
// and the lanes do not diverge inside a trip.  Neighbouring targets have neighbouring sight lines, so the lanes of a wavefront
// read the same few cache lines of the occupancy bytes.
// PF_VIS_WAVE_PER_TARGET = 1 is the form measured against it: one wavefront per target, the lanes on the major indices
// (sm_first_block, the pair kernel's walk).  At K = 64 it is slower on every map measured, most on the maps with obstacles,
// where a sight line ends after a few cells with 64 lanes lit; it wins only the 128 x 128 map at K = 1.
//
// k_visibility_count_lanes_on_targets: the same walk, a lane per target, each thread over a CHUNK of `per` consecutive viewpoints (blockIdx.y picks the
// chunk) and one integer atomicAdd of its partial sum into the zeroed counts: with per == 1 (shipped) one atomic per seen
// (viewpoint, cell), with per >= K a plain loop over the viewpoints per cell.  Integer sums: the same words whatever the order.
// The K masks are never written anywhere.
//
// The info words come from passes of their own over the finished masks / counts (a byte or a word per cell, against a walk per
// cell): packed 64-bit keys (value << 32) | ~id, reduced per wavefront and then with one atomicMax, give the largest value with
// the smallest cell id that attains it.
//
// k_visibility_paths_one_wave_per_row: one wavefront per path row, the lanes stride over the cells and gather the counts.
//
// Every occupancy byte read lies inside the bounding box of (viewpoint, target), both inside the grid (the host checks the
// viewpoints, the kernels their cell id against RC).
#pragma once

namespace pf {

#ifndef PF_VIS_WAVE_PER_TARGET
#define PF_VIS_WAVE_PER_TARGET 0                /* 1: the field kernel takes one wavefront per target (the form measured against the shipped one) */
#endif
#ifndef PF_VIS_COUNT_PER
#define PF_VIS_COUNT_PER 1                      /* viewpoints per thread of the count kernel; 0: split the viewpoints until about 2^20 threads exist */
#endif
#ifndef PF_VIS_TRIPS
#define PF_VIS_TRIPS 4                          /* major indices a lane examines per trip of its walk: their loads are in flight together */
#endif
#define PF_VIS_THREADS 256
#define PF_VIS_COUNT_THREADS_WANTED (1 << 20)   /* PF_VIS_COUNT_PER = 0: the count kernel splits the viewpoints until about this many threads exist */

// The viewpoints one thread of the count kernel walks.  Shipped: one (an atomic per seen pair), the fastest form on every map measured
// (DESIGN.md 4.24); 0 walks all K on a map that fills the device by its cells alone and fewer on a small one; a value >= K is a plain loop.
static inline int vis_count_per(int RC, int K) {
  if (PF_VIS_COUNT_PER > 0) return PF_VIS_COUNT_PER < K ? PF_VIS_COUNT_PER : K;
  long long chunks = (PF_VIS_COUNT_THREADS_WANTED + (long long)RC - 1) / RC;
  if (chunks > K) chunks = K;
  if (chunks > 65535) chunks = 65535;
  return (int)((K + chunks - 1) / chunks);
}

// Does the free cell a see the free cell a + (dr, dc), (dr, dc) != (0, 0)?  One lane, one sight line, out at the first blocker.
__device__ __forceinline__ bool vis_lane_sees(const uint8_t* __restrict__ occ, int C, int a, int dr, int dc, int strict) {
  const int adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
  const bool colmaj = adc >= adr;
  const int A = colmaj ? adr : adc, B = colmaj ? adc : adr, s = A + B;
  const int sr = dr < 0 ? -C : C, sc = dc < 0 ? -1 : 1;
  const int stepmaj = colmaj ? sc : sr, stepmin = colmaj ? sr : sc;
  const bool corner = strict && A == B;                              // a pure diagonal: the cells beside it are touched
  const bool corners = __ballot(corner) != 0ull;                     // (wave-uniform: the third load exists only where some lane needs it)
  // The two tests in loop-invariant form.  With lim = s (strict) or s - 1: 2 rem <= lim iff rem <= h, h = floor(lim / 2), and
  // 2 (B - rem) <= lim iff rem >= B - h.  q = floor(A t / B) < A iff t < B, and on a pure diagonal q = t: q itself is not kept.
  const int h = (strict ? s : s - 1) >> 1, lo = B - h;
  int rem = 0, cell = a;                                             // at major offset t: A t = q B + rem, cell = a + t stepmaj + q stepmin
  for (int t0 = 0; t0 <= B; t0 += PF_VIS_TRIPS) {
    // the addresses of PF_VIS_TRIPS major indices first, then all their loads in flight together, then one test: a cell that
    // does not count (or lies beyond b) is replaced by a itself, which is free, so no load is conditional
    unsigned i0[PF_VIS_TRIPS], i1[PF_VIS_TRIPS], i2[PF_VIS_TRIPS];
#pragma unroll
    for (int j = 0; j < PF_VIS_TRIPS; ++j) {
      const int t = t0 + j;
      i0[j] = (unsigned)(t <= B && rem <= h ? cell : a);
      i1[j] = (unsigned)(t < B && rem >= lo ? cell + stepmin : a);
      i2[j] = (unsigned)(corner && t >= 1 && t <= B ? cell - stepmin : a);   // (A == B: rem stays 0)
      rem += A; cell += stepmaj;
      if (rem >= B) { rem -= B; cell += stepmin; }
    }
    int hit = 0;
#pragma unroll
    for (int j = 0; j < PF_VIS_TRIPS; ++j) hit |= (occ[i0[j]] == 1) | (occ[i1[j]] == 1);
    if (corners) {
#pragma unroll
      for (int j = 0; j < PF_VIS_TRIPS; ++j) hit |= occ[i2[j]] == 1;
    }
    if (hit) return false;
  }
  return true;
}

// visible(a, v) within the range, for one lane: the free early answers, then the walk.  a and v lie inside the grid.
__device__ __forceinline__ bool vis_lane_target(const uint8_t* __restrict__ occ, int C, int a, int r0, int c0, int v, int r1, int c1, int strict, int range_sq) {
  if (occ[v] == 1) return false;
  const int dr = r1 - r0, dc = c1 - c0;
  if (range_sq >= 0 && dr * dr + dc * dc > range_sq) return false;
  if (v == a) return true;                                           // (the viewpoint is free: the caller's)
  return vis_lane_sees(occ, C, a, dr, dc, strict);
}

#if PF_VIS_WAVE_PER_TARGET
__global__ __launch_bounds__(PF_VIS_THREADS) void k_visibility_field_wave_per_target(const uint8_t* __restrict__ occ, int RC, int C, int strict, int range_sq, int K,
                                                                                      const int* __restrict__ view, uint8_t* __restrict__ seen) {
  const int lane = (int)(threadIdx.x & 63u);
  const int v = (int)(blockIdx.x * (PF_VIS_THREADS / 64) + (threadIdx.x >> 6));
  if (v >= RC) return;                                               // (the whole wavefront)
  const int r1 = v / C, c1 = v - r1 * C;
  for (int k = (int)blockIdx.y; k < K; k += (int)gridDim.y) {
    const int a = view[k];
    const int r0 = a / C, c0 = a - r0 * C;
    const int dr = r1 - r0, dc = c1 - c0;
    bool s = occ[a] != 1 && occ[v] != 1 && (range_sq < 0 || dr * dr + dc * dc <= range_sq);
    if (s) s = sm_first_block(occ, C, a, v, strict, lane) < 0;
    if (lane == 0) seen[(size_t)k * (size_t)RC + (size_t)v] = s ? 1 : 0;
  }
}
#else
__global__ __launch_bounds__(PF_VIS_THREADS) void k_visibility_field_lane_per_target(const uint8_t* __restrict__ occ, int RC, int C, int strict, int range_sq, int K,
                                                                                      const int* __restrict__ view, uint8_t* __restrict__ seen) {
  const int v = (int)(blockIdx.x * PF_VIS_THREADS + threadIdx.x);
  if (v >= RC) return;
  const int r1 = v / C, c1 = v - r1 * C;
  for (int k = (int)blockIdx.y; k < K; k += (int)gridDim.y) {
    const int a = view[k];                                           // (the same word in every lane)
    bool s = false;
    if (occ[a] != 1) {
      const int r0 = a / C, c0 = a - r0 * C;
      s = vis_lane_target(occ, C, a, r0, c0, v, r1, c1, strict, range_sq);
    }
    seen[(size_t)k * (size_t)RC + (size_t)v] = s ? 1 : 0;
  }
}
#endif

// keys [K][2]: {the largest (d2 << 32) | ~id over the seen cells, the seen cells}, zeroed by the host
__global__ __launch_bounds__(PF_VIS_THREADS) void k_visibility_field_info_reduce(const uint8_t* __restrict__ seen, int RC, int C, int K, const int* __restrict__ view,
                                                                                  unsigned long long* __restrict__ keys) {
  for (int k = (int)blockIdx.y; k < K; k += (int)gridDim.y) {
    const int a = view[k];
    const int r0 = a / C, c0 = a - r0 * C;
    const uint8_t* const row = seen + (size_t)k * (size_t)RC;
    unsigned long long best = 0;
    int cnt = 0;
    for (int v = (int)(blockIdx.x * PF_VIS_THREADS + threadIdx.x); v < RC; v += (int)(gridDim.x * PF_VIS_THREADS)) {
      if (!row[v]) continue;
      const int r1 = v / C, c1 = v - r1 * C;
      const int dr = r1 - r0, dc = c1 - c0;
      const unsigned long long key = ((unsigned long long)(unsigned)(dr * dr + dc * dc) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v);
      best = key > best ? key : best;
      cnt += 1;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(best, d);
      best = o > best ? o : best;
      cnt += __shfl_xor(cnt, d);
    }
    if ((threadIdx.x & 63u) == 0 && cnt) {
      atomicMax(keys + 2 * (size_t)k, best);
      atomicAdd(keys + 2 * (size_t)k + 1, (unsigned long long)cnt);
    }
  }
}

__global__ void k_visibility_field_write_info(int K, const unsigned long long* __restrict__ keys, long long* __restrict__ info) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= K) return;
  const unsigned long long key = keys[2 * (size_t)k], cnt = keys[2 * (size_t)k + 1];
  long long* const o = info + 4 * (size_t)k;
  o[0] = (long long)cnt;
  o[1] = cnt ? (long long)(key >> 32) : -1;
  o[2] = cnt ? (long long)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1;
  o[3] = 0;
}

// count [RC], zeroed by the host: += the viewpoints of this thread's chunk that see the cell
__global__ __launch_bounds__(PF_VIS_THREADS) void k_visibility_count_lanes_on_targets(const uint8_t* __restrict__ occ, int RC, int C, int strict, int range_sq, int K, int per,
                                                                                       const int* __restrict__ view, int* __restrict__ count) {
  const int v = (int)(blockIdx.x * PF_VIS_THREADS + threadIdx.x);
  if (v >= RC || occ[v] == 1) return;
  const int r1 = v / C, c1 = v - r1 * C;
  for (int chunk = (int)blockIdx.y; (long long)chunk * per < K; chunk += (int)gridDim.y) {
    const int k0 = chunk * per, k1 = k0 + per < K ? k0 + per : K;
    int n = 0;
    for (int k = k0; k < k1; ++k) {
      const int a = view[k];                                         // (the same word in every lane)
      if (occ[a] == 1) continue;
      const int r0 = a / C, c0 = a - r0 * C;
      n += vis_lane_target(occ, C, a, r0, c0, v, r1, c1, strict, range_sq) ? 1 : 0;
    }
    if (n) atomicAdd(count + v, n);
  }
}

// ctl [3]: {the largest (count << 32) | ~id over the free cells, free cells with count > 0, free cells}, zeroed by the host
__global__ __launch_bounds__(PF_VIS_THREADS) void k_visibility_count_info_reduce(const uint8_t* __restrict__ occ, const int* __restrict__ count, int RC,
                                                                                  unsigned long long* __restrict__ ctl) {
  unsigned long long best = 0;
  int nfree = 0, nseen = 0;
  for (int v = (int)(blockIdx.x * PF_VIS_THREADS + threadIdx.x); v < RC; v += (int)(gridDim.x * PF_VIS_THREADS)) {
    if (occ[v] == 1) continue;
    const int n = count[v];
    const unsigned long long key = ((unsigned long long)(unsigned)n << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v);
    best = key > best ? key : best;
    nfree += 1;
    nseen += n > 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    best = o > best ? o : best;
    nfree += __shfl_xor(nfree, d);
    nseen += __shfl_xor(nseen, d);
  }
  if ((threadIdx.x & 63u) == 0 && nfree) {
    atomicMax(ctl, best);
    if (nseen) atomicAdd(ctl + 1, (unsigned long long)nseen);
    atomicAdd(ctl + 2, (unsigned long long)nfree);
  }
}

__global__ void k_visibility_count_write_info(const unsigned long long* __restrict__ ctl, long long* __restrict__ info) {
  if (blockIdx.x || threadIdx.x) return;
  const bool any = ctl[2] != 0;
  info[0] = (long long)ctl[1];
  info[1] = (long long)ctl[2];
  info[2] = any ? (long long)(ctl[0] >> 32) : -1;
  info[3] = any ? (long long)(0xFFFFFFFFu - (unsigned)(ctl[0] & 0xFFFFFFFFull)) : -1;
}

__global__ __launch_bounds__(64) void k_visibility_paths_one_wave_per_row(const int* __restrict__ count, int RC, int n, int path_cap, const int* __restrict__ cells,
                                                                         const int* __restrict__ len, long long* __restrict__ out, int* __restrict__ profile,
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
  long long best = -0x7FFFFFFFFFFFFFFFll - 1, sum = 0;               // (count << 32) | ~position: the largest count, its first position
  int above = 0;
  if (!bad) {
    int* const prof = profile ? profile + (size_t)p * (size_t)path_cap : nullptr;
    for (int i = lane; i < L; i += 64) {
      const int v = count[row[i]];
      if (prof) prof[i] = v;
      const long long key = (long long)(((unsigned long long)(unsigned)v << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
      best = key > best ? key : best;
      sum += v;
      above += v > 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const long long o = __shfl_xor(best, d);
      best = o > best ? o : best;
      sum += __shfl_xor(sum, d);
      above += __shfl_xor(above, d);
    }
  }
  if (lane == 0) {
    long long* const o = out + 4 * (size_t)p;
    o[0] = bad ? 0 : sum;
    o[1] = bad ? -1 : (long long)(int)(best >> 32);
    o[2] = bad ? -1 : (long long)(0xFFFFFFFFu - (unsigned)((unsigned long long)best & 0xFFFFFFFFull));
    o[3] = bad ? 0 : above;
  }
  if (lane == 0) status[p] = bad ? 1 : 0;
}

}  // namespace pf
