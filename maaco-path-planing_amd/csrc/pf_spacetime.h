// pf_spacetime.h -- space-time fields: arrival ticks and routes among moving obstacles (pf_spacetime_stamp, pf_spacetime_field,
// pf_spacetime_paths, pf_spacetime_conflicts).
//
// Time runs in ticks 0..T; in a tick a robot waits or makes one move of the policy (allow_diag, restrict_corner).  S is the
// handle's static occupancy, D[t] the dynamic plane of tick t (uint64 [T + 1][R][Wc], Wc = ceil(C / 64), cell (r, c) = bit c & 63 of
// word r Wc + (c >> 6), bits at c >= C zero), A[t] = S | D[t].  A robot at u at tick t may be at v at tick t + 1 iff
//   1. v is inside the grid and A[t + 1][v] == 0                                                   (vertex)
//   2. v == u, or u -> v is a straight step, or a diagonal one when allow_diag                     (shape)
//   3. for a move, not both D[t][v] and D[t + 1][u]                                                (swap / pass-through, on the planes)
//   4. for a diagonal move under restrict_corner, (v.r, u.c) and (u.r, v.c) are clear in A[t] | A[t + 1]   (corner)
// reach[0] = the sources free in A[0]; reach[t + 1][v] = some u of reach[t] may be at v.  reach is NOT monotone in t.
//
// k_spacetime_field: ONE WORKGROUP PER SOURCE SET, the tick loop inside the kernel, min(B, CUs) workgroups looping over the sets.
// A thread owns the words w = tid, tid + threads, ...; per tick it builds word (r, k) of reach[t + 1] from the nine neighbouring
// words of reach[t] and of D[t + 1] (the swap rule's D[t + 1][u]), and, for the corner rule, the row's three words and the two
// words above and below of S | D[t] | D[t + 1].  A column neighbour is a shift with the carry of the adjacent word, a row
// neighbour the same bit of the word +- Wc.  Three planes are live per workgroup: reach[t], reach[t + 1] and `seen`, the OR of
// all reach planes so far, whose fresh bits are the cells whose arrival tick is t + 1 (written in the loop, one store per cell
// and call).  LDS = true: the three planes lie in LDS (3 R Wc 8 bytes <= PF_STF_LDS_BYTES); LDS = false: in a scratch slot of
// the workgroup in HBM.  Either way the hand-off from tick to tick stays inside one workgroup: the words a thread reads at tick
// t + 1 were written at tick t by threads of its own workgroup, one __syncthreads() per tick orders them, and no other workgroup
// ever writes them -- no agent-scope traffic, no flags.  The planes of D are read-only in the launch.
//
// The other three kernels are literal, cell by cell (st_may below is the rule as written above): the stamp and the conflict
// check take one wavefront per row with the lanes on the positions, the route walk one lane per query (a walk is a chain).
#pragma once

namespace pf {

#ifndef PF_STF_THREADS
#define PF_STF_THREADS 1024                     /* the largest workgroup of the field kernel; a map of fewer words takes fewer wavefronts */
#endif
#ifndef PF_STF_LDS_BYTES
#define PF_STF_LDS_BYTES (60 * 1024)            /* the three live planes lie in LDS up to this many bytes; 0: always in HBM */
#endif

typedef unsigned long long st_u64;

__device__ __forceinline__ int st_bit(const st_u64* P, int Wc, int r, int c) {
  return (int)((P[(size_t)r * (size_t)Wc + (size_t)(c >> 6)] >> (c & 63)) & 1ull);
}

// The static occupancy as a bit plane [R][Wc], one thread per word (the bits at c >= C stay zero).
__global__ __launch_bounds__(256) void k_spacetime_pack_static(const uint8_t* __restrict__ occ, int R, int C, int Wc, st_u64* __restrict__ S) {
  const int w = (int)(blockIdx.x * 256 + threadIdx.x);
  if (w >= R * Wc) return;
  const int r = w / Wc, c0 = (w - r * Wc) * 64;
  st_u64 x = 0;
  for (int i = 0; i < 64 && c0 + i < C; ++i) x |= (st_u64)(occ[(size_t)r * C + c0 + i] == 1) << i;
  S[w] = x;
}

struct StTri { st_u64 l, m, r; };                // a row's word seen from (r, k): bit c = the row's cell c - 1, c, c + 1

template <bool LDS>
__global__ __launch_bounds__(PF_STF_THREADS) void k_spacetime_field_group_per_set(const st_u64* __restrict__ S, const st_u64* __restrict__ D, int R, int C, int Wc, int T,
                                                                                   int diag, int restr, int B, const int* __restrict__ off, const int* __restrict__ src,
                                                                                   int* __restrict__ arrive, st_u64* __restrict__ reach_out, long long* __restrict__ info,
                                                                                   st_u64* scratch) {
  extern __shared__ st_u64 st_lds[];
  __shared__ st_u64 s_key;
  __shared__ unsigned s_cnt;
  const int W = R * Wc, RC = R * C, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  st_u64* p0;
  if constexpr (LDS) p0 = st_lds; else p0 = scratch + (size_t)blockIdx.x * 3 * (size_t)W;
  st_u64* p1 = p0 + W;
  st_u64* const seen = p0 + 2 * (size_t)W;       // (p0 and p1 swap; seen stays)
  const st_u64 lastmask = (C & 63) ? ((1ull << (C & 63)) - 1ull) : ~0ull;
  const bool corner = diag && restr;

  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    int* const arr = arrive + (size_t)b * (size_t)RC;
    st_u64* const ro = reach_out ? reach_out + (size_t)b * ((size_t)T + 1) * (size_t)W : nullptr;
    for (int i = tid; i < RC; i += nt) arr[i] = -1;
    for (int w = tid; w < W; w += nt) p0[w] = 0;
    if (tid == 0) { s_key = 0; s_cnt = 0; }
    __syncthreads();
    for (int i = off[b] + tid; i < off[b + 1]; i += nt) {             // the sources free in A[0] (the host checked the ids)
      const int v = src[i], r = v / C, c = v - r * C, w = r * Wc + (c >> 6);
      const st_u64 bit = 1ull << (c & 63);
      if (!((S[w] | D[w]) & bit)) atomicOr(p0 + w, bit);
    }
    __syncthreads();

    st_u64 key = 0;                                                   // (arrival tick << 32) | ~cell id: the largest tick, its smallest cell
    unsigned cnt = 0;
    auto emit = [&](st_u64 x, int w, int t) {                         // the cells of word w whose arrival tick is t
      const int r = w / Wc, base = r * C + (w - r * Wc) * 64;
      while (x) {
        const int v = base + __ffsll((long long)x) - 1;
        x &= x - 1;
        arr[v] = t;
        cnt += 1;
        const st_u64 kk = ((st_u64)(unsigned)t << 32) | (st_u64)(0xFFFFFFFFu - (unsigned)v);
        key = kk > key ? kk : key;
      }
    };
    for (int w = tid; w < W; w += nt) {
      const st_u64 x = p0[w];
      seen[w] = x;
      if (ro) ro[w] = x;
      emit(x, w, 0);
    }

    for (int t = 0; t < T; ++t) {
      const st_u64* const D0 = D + (size_t)t * (size_t)W;
      const st_u64* const D1 = D0 + W;
      for (int w = tid; w < W; w += nt) {
        const int r = w / Wc, k = w - r * Wc;
        const bool up = r > 0, dn = r + 1 < R, lf = k > 0, rt = k + 1 < Wc;
        auto tri = [&](const st_u64* P, int ww, bool row) -> StTri {  // the row of word ww = w - Wc, w or w + Wc; zero beside the grid
          if (!row) return StTri{0, 0, 0};
          const st_u64 a = lf ? P[ww - 1] : 0, m = P[ww], z = rt ? P[ww + 1] : 0;
          return StTri{(m << 1) | (a >> 63), m, (m >> 1) | (z << 63)};
        };
        // u = v - step: the row above serves the steps with dr = +1, .l the steps with dc = +1
        const StTri Pu = tri(p0, w - Wc, up), Pm = tri(p0, w, true), Pd = tri(p0, w + Wc, dn);
        const StTri Qu = tri(D1, w - Wc, up), Qm = tri(D1, w, true), Qd = tri(D1, w + Wc, dn);
        const st_u64 d0v = D0[w], sv = S[w];
        st_u64 nw = Pm.m                                              // wait
                    | (Pm.l & ~(d0v & Qm.l)) | (Pm.r & ~(d0v & Qm.r)) | (Pu.m & ~(d0v & Qu.m)) | (Pd.m & ~(d0v & Qd.m));
        if (diag) {
          st_u64 dul = Pu.l & ~(d0v & Qu.l), dur = Pu.r & ~(d0v & Qu.r), ddl = Pd.l & ~(d0v & Qd.l), ddr = Pd.r & ~(d0v & Qd.r);
          if (corner) {                                               // X = S | D[t] | D[t + 1] at (v.r, u.c) and (u.r, v.c)
            const st_u64 xa = lf ? (S[w - 1] | D0[w - 1] | D1[w - 1]) : 0, xm = sv | d0v | Qm.m, xz = rt ? (S[w + 1] | D0[w + 1] | D1[w + 1]) : 0;
            const st_u64 xl = (xm << 1) | (xa >> 63), xr = (xm >> 1) | (xz << 63);
            const st_u64 xu = up ? (S[w - Wc] | D0[w - Wc] | Qu.m) : 0, xd = dn ? (S[w + Wc] | D0[w + Wc] | Qd.m) : 0;
            dul &= ~(xl | xu); dur &= ~(xr | xu); ddl &= ~(xl | xd); ddr &= ~(xr | xd);
          }
          nw |= dul | dur | ddl | ddr;
        }
        nw &= ~(sv | Qm.m);                                           // vertex: A[t + 1][v]
        if (!rt) nw &= lastmask;
        p1[w] = nw;
        if (ro) ro[((size_t)t + 1) * (size_t)W + (size_t)w] = nw;
        const st_u64 old = seen[w], fresh = nw & ~old;
        if (fresh) { seen[w] = old | fresh; emit(fresh, w, t + 1); }
      }
      __syncthreads();                                                // reach[t + 1] is whole; nobody reads reach[t] any more
      st_u64* const s = p0; p0 = p1; p1 = s;
    }

#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const st_u64 o = __shfl_xor(key, d);
      key = o > key ? o : key;
      cnt += __shfl_xor(cnt, d);
    }
    if ((tid & 63) == 0 && cnt) { atomicMax(&s_key, key); atomicAdd(&s_cnt, cnt); }
    __syncthreads();
    if (tid == 0 && info) {
      long long* const o = info + 4 * (size_t)b;
      const st_u64 kk = s_key;
      const unsigned n = s_cnt;
      o[0] = (long long)n;
      o[1] = n ? (long long)(kk >> 32) : -1;
      o[2] = n ? (long long)(0xFFFFFFFFu - (unsigned)(kk & 0xFFFFFFFFull)) : -1;
      o[3] = 0;
    }
    __syncthreads();                                                  // (the next set wipes s_key and the planes)
  }
}

// ---- the rule, cell by cell ---------------------------------------------------------------------------------------------------
// May a robot at u = (ur, uc) at the tick of plane D0 be at v = (vr, vc) at the tick of plane D1 = D0 + W?  Both cells inside the grid.
__device__ __forceinline__ bool st_may(const uint8_t* __restrict__ occ, const st_u64* D0, const st_u64* D1, int C, int Wc, int ur, int uc, int vr, int vc, int diag,
                                       int restr) {
  if (occ[(size_t)vr * C + vc] == 1 || st_bit(D1, Wc, vr, vc)) return false;
  const int dr = vr - ur, dc = vc - uc;
  if (dr == 0 && dc == 0) return true;
  if (dr < -1 || dr > 1 || dc < -1 || dc > 1) return false;
  const bool dg = dr != 0 && dc != 0;
  if (dg && !diag) return false;
  if (st_bit(D0, Wc, vr, vc) && st_bit(D1, Wc, ur, uc)) return false;
  if (dg && restr) {
    if (occ[(size_t)vr * C + uc] == 1 || occ[(size_t)ur * C + vc] == 1) return false;
    if (st_bit(D0, Wc, vr, uc) || st_bit(D1, Wc, vr, uc) || st_bit(D0, Wc, ur, vc) || st_bit(D1, Wc, ur, vc)) return false;
  }
  return true;
}

// A path row as the stamp and the conflict check see it: bad = an empty row, a length beyond path_cap, a cell outside [0, RC) or a
// t0 outside [0, T].  One wavefront; every lane gets the verdict.
__device__ __forceinline__ bool st_row_bad(const int* __restrict__ row, int L, int path_cap, int RC, int t0, int T, int lane) {
  if (L < 1 || L > path_cap || t0 < 0 || t0 > T) return true;
  int off = 0;
  for (int j = lane; j < L; j += 64) off |= (unsigned)row[j] >= (unsigned)RC;
  return __ballot(off) != 0ull;
}

__device__ __forceinline__ void st_or(st_u64* D, int W, int Wc, int C, int T, int t, int r, int c) {
  if (t < 0 || t > T) return;
  atomicOr(D + (size_t)t * (size_t)W + (size_t)r * Wc + (size_t)(c >> 6), 1ull << (c & 63));
}

__global__ __launch_bounds__(64) void k_spacetime_stamp_one_wave_per_row(st_u64* D, int R, int C, int Wc, int T, int n, int path_cap, const int* __restrict__ cells,
                                                                        const int* __restrict__ len, const int* __restrict__ t0s, int after_end, int corners,
                                                                        int* __restrict__ status) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (p >= n) return;
  const int W = R * Wc, L = len[p], t0 = t0s ? t0s[p] : 0;
  const int* const row = cells + (size_t)p * (size_t)path_cap;
  const bool bad = st_row_bad(row, L, path_cap, R * C, t0, T, lane);
  if (lane == 0) status[p] = bad ? 1 : 0;
  if (bad) return;
  for (int j = lane; j < L && t0 + j <= T; j += 64) {
    const int v = row[j], vr = v / C, vc = v - vr * C;
    st_or(D, W, Wc, C, T, t0 + j, vr, vc);
    if (corners && j + 1 < L) {                                       // the swept footprint of a unit diagonal step over t0 + j -> t0 + j + 1
      const int x = row[j + 1], xr = x / C, xc = x - xr * C, dr = xr - vr, dc = xc - vc;
      if ((dr == 1 || dr == -1) && (dc == 1 || dc == -1)) {
        st_or(D, W, Wc, C, T, t0 + j, xr, vc);     st_or(D, W, Wc, C, T, t0 + j, vr, xc);
        st_or(D, W, Wc, C, T, t0 + j + 1, xr, vc); st_or(D, W, Wc, C, T, t0 + j + 1, vr, xc);
      }
    }
  }
  if (after_end) {
    const int v = row[L - 1], vr = v / C, vc = v - vr * C;
    for (long long t = (long long)t0 + L + lane; t <= T; t += 64) st_or(D, W, Wc, C, T, (int)t, vr, vc);
  }
}

// One lane per query: the tick (earliest, hold or given), then the walk back by the route rule -- the moves 0..7 in helper order
// first, the wait last -- twice: once to see that every tick has a predecessor, once to write the row, so that a row is either
// whole or untouched.  Every cell examined lies inside the grid whatever the reach words hold, and a walk makes `tick` steps.
__global__ __launch_bounds__(64) void k_spacetime_paths_lane_per_query(const uint8_t* __restrict__ occ, const st_u64* D, const st_u64* reach, int R, int C, int Wc, int T,
                                                                      int diag, int restr, int B, int n, const int* __restrict__ set_idx, const int* __restrict__ target,
                                                                      const int* __restrict__ tick, int path_cap, int* __restrict__ cells, int* __restrict__ len,
                                                                      int* __restrict__ status, int* __restrict__ tick_out) {
  const int q = (int)(blockIdx.x * 64 + threadIdx.x);
  if (q >= n) return;
  const int W = R * Wc, RC = R * C;
  const int b = set_idx[q], v = target[q];
  int tk = tick ? tick[q] : -1;
  int st = PF_ST_OK;
  if (b < 0 || b >= B || v < 0 || v >= RC || tk < -2 || tk > T) { st = PF_ST_INFEASIBLE; tk = -1; }
  const int vr0 = st ? 0 : v / C, vc0 = st ? 0 : v - vr0 * C;
  const st_u64* const Rb = reach + (size_t)(st ? 0 : b) * ((size_t)T + 1) * (size_t)W;
  if (!st) {
    int from = 0;
    if (tk == -2) {                                                   // the hold tick: the cell stays clear of D from there to T
      from = T + 1;
      for (int t = T; t >= 0 && !st_bit(D + (size_t)t * W, Wc, vr0, vc0); --t) from = t;
    }
    if (tk < 0) {
      tk = -1;
      for (int t = from; t <= T; ++t)
        if (st_bit(Rb + (size_t)t * W, Wc, vr0, vc0)) { tk = t; break; }
      if (tk < 0) st = PF_ST_INFEASIBLE;
    } else if (!st_bit(Rb + (size_t)tk * W, Wc, vr0, vc0)) {
      st = PF_ST_INFEASIBLE; tk = -1;
    }
  }
  if (!st && tk + 1 > path_cap) st = PF_ST_OVERFLOW;
  if (!st) {
    int* const row = cells + (size_t)q * (size_t)path_cap;
    const int nd = diag ? 8 : 4;
    for (int pass = 0; pass < 2 && !st; ++pass) {
      int vr = vr0, vc = vc0;
      for (int t = tk; t > 0; --t) {
        if (pass) row[t] = vr * C + vc;
        const st_u64* const P = Rb + (size_t)(t - 1) * W;
        const st_u64* const D0 = D + (size_t)(t - 1) * W;
        int ur = -1, uc = -1;
        for (int d = 0; d <= nd; ++d) {
          const int r = d < nd ? vr - HM_DR[d] : vr, c = d < nd ? vc - HM_DC[d] : vc;
          if ((unsigned)r >= (unsigned)R || (unsigned)c >= (unsigned)C) continue;
          if (!st_bit(P, Wc, r, c) || !st_may(occ, D0, D0 + W, C, Wc, r, c, vr, vc, diag, restr)) continue;
          ur = r; uc = c;
          break;
        }
        if (ur < 0) { st = PF_ST_OVERFLOW; break; }                   // (pass 0 only: planes that no field call made on this map)
        vr = ur; vc = uc;
      }
      if (pass) row[0] = vr * C + vc;
    }
  }
  len[q] = st ? 0 : tk + 1;
  status[q] = st;
  if (tick_out) tick_out[q] = tk;
}

// One step u -> v over the planes D0 -> D1, or the first cell (first: u is not looked at, D1 is the plane of its tick) -> the kind
// by precedence: 1 static, 2 vertex, 3 swap, 4 corner, 0 none.
__device__ __forceinline__ int st_kind(const uint8_t* __restrict__ occ, const st_u64* D0, const st_u64* D1, int C, int Wc, int u, int v, bool first, int diag, int restr) {
  const int vr = v / C, vc = v - vr * C;
  if (occ[v] == 1) return 1;
  if (first) return st_bit(D1, Wc, vr, vc) ? 2 : 0;
  const int ur = u / C, uc = u - ur * C, dr = vr - ur, dc = vc - uc;
  const bool wait = dr == 0 && dc == 0, dg = dr != 0 && dc != 0;
  if (!wait && (dr < -1 || dr > 1 || dc < -1 || dc > 1 || (dg && !diag))) return 1;
  const bool cr = dg && restr;
  if (cr && (occ[(size_t)vr * C + uc] == 1 || occ[(size_t)ur * C + vc] == 1)) return 1;
  if (st_bit(D1, Wc, vr, vc)) return 2;
  if (!wait && st_bit(D0, Wc, vr, vc) && st_bit(D1, Wc, ur, uc)) return 3;
  if (cr && (st_bit(D0, Wc, vr, uc) || st_bit(D1, Wc, vr, uc) || st_bit(D0, Wc, ur, vc) || st_bit(D1, Wc, ur, vc))) return 4;
  return 0;
}

__global__ __launch_bounds__(64) void k_spacetime_conflicts_one_wave_per_row(const uint8_t* __restrict__ occ, const st_u64* D, int R, int C, int Wc, int T, int diag, int restr,
                                                                            int n, int path_cap, const int* __restrict__ cells, const int* __restrict__ len,
                                                                            const int* __restrict__ t0s, int hold, int* __restrict__ out, int* __restrict__ status) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (p >= n) return;
  const int W = R * Wc, L = len[p], t0 = t0s ? t0s[p] : 0;
  const int* const row = cells + (size_t)p * (size_t)path_cap;
  int* const o = out + 4 * (size_t)p;
  if (st_row_bad(row, L, path_cap, R * C, t0, T, lane)) {
    if (lane == 0) { o[0] = -1; o[1] = 0; o[2] = -1; o[3] = 0; status[p] = 1; }
    return;
  }
  const bool past = (long long)t0 + L - 1 > T;
  const int last = past ? T - t0 : L - 1;                             // the last position inside the horizon
  st_u64 best = ~0ull;                                                // (tick << 40) | (kind << 32) | cell: the least
  int cnt = 0;
  for (int j = lane; j <= last; j += 64) {
    const st_u64* const D1 = D + (size_t)(t0 + j) * W;
    const int kind = st_kind(occ, j ? D1 - W : D1, D1, C, Wc, j ? row[j - 1] : 0, row[j], j == 0, diag, restr);
    if (kind) {
      const st_u64 key = ((st_u64)(unsigned)(t0 + j) << 40) | ((st_u64)kind << 32) | (st_u64)(unsigned)row[j];
      best = key < best ? key : best;
      cnt += 1;
    }
  }
  if (hold && !past) {                                                // the last cell as a vertex at every later tick
    const int v = row[L - 1], vr = v / C, vc = v - vr * C;
    for (long long t = (long long)t0 + L + lane; t <= T; t += 64)
      if (st_bit(D + (size_t)t * W, Wc, vr, vc)) {
        const st_u64 key = ((st_u64)t << 40) | (2ull << 32) | (st_u64)(unsigned)v;
        best = key < best ? key : best;
        cnt += 1;
      }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const st_u64 ob = __shfl_xor(best, d);
    best = ob < best ? ob : best;
    cnt += __shfl_xor(cnt, d);
  }
  if (lane == 0) {
    o[0] = cnt ? (int)(best >> 40) : -1;
    o[1] = cnt ? (int)((best >> 32) & 0xFFull) : 0;
    o[2] = cnt ? (int)(best & 0xFFFFFFFFull) : -1;
    o[3] = cnt;
    status[p] = past ? 2 : 0;
  }
}

}  // namespace pf
