// pf_sight.h -- the sight graph over a list of node cells and exact any-angle shortest paths in it (pf_sight_pack,
// pf_sight_field, pf_sight_paths).
//
// The graph.  M nodes, cell ids in increasing order; node i sees node j iff pf_smooth.h's visible(nodes[i], nodes[j], strict) holds
// and the pair lies within the range disc.  The adjacency is a bit matrix, 64 nodes a word: bit j & 63 of word j >> 6 of row i.
// k_sight_pack_lane_per_pair: ONE LANE PER ORDERED PAIR (i, j), the 64 lanes of a wavefront on 64 consecutive j, one __ballot a
// word (pf_cover.h's way of packing a predicate); the lane's walk is pf_visibility.h's vis_lane_sees.  Nodes are sorted by cell
// id, so the lanes of a wavefront sit on neighbouring cells and their sight lines read the same few cache lines.  All M^2 pairs
// are walked: the rule is symmetric, and so is the matrix, without a mirror pass.
//
// The field.  Edge weights w(i, j) = sqrt((double)(dr^2 + dc^2)).  A label is the least left-to-right fp64 sum over the walks
// from a usable source (one whose diagonal bit is set).  fp64 addition is monotone and w >= 1, so the labels are the unique
// fixed point of d[v] = min_u fl(d[u] + w(u, v)) with d = 0 at the sources: any label-correcting order ends on the same words.
// k_sight_field_group_per_set: one workgroup of 1 024 threads per source set, the round loop inside the kernel.  Thread t owns
// the nodes t, t + 1024, ...; a round relaxes every owned node v against adj[v][k] & changed[k], word by word; a word whose
// `changed` word is zero is skipped by the whole wavefront (the word lives in LDS: the branch is uniform); the set bits are taken
// with a count-trailing-zeros.  A label that fell marks its node in the next round's `changed` words; the loop ends on a round
// without a change.  Labels only fall, and every value ever stored is the sum of a real walk, so a label read while its owner
// lowers it is a valid (if stale) bound: its node is marked, and the reader meets the new value one round later.
// The labels of a set live in LDS while M <= PF_SIGHT_LDS_NODES (8 bytes a node: 128 KiB at M = 16 384, of the CU's 160) and are
// copied to the row at the end; above that they live in the output row itself (HBM, through the CU's L1).  The shipped value
// keeps every legal M in LDS; a smaller value is the form measured against it.
//
// The parents are a field-only rule of their own (k_sight_parents): the smallest u with the bit set, d[u] < d[v] and
// fl(d[u] + w(u, v)) == d[v]; such a u exists at every finite label that is no source, because the label is that sum for the
// walk's last edge.  k_sight_paths chases them, a thread a query, and ends every walk within M steps whatever the words hold.
//
// Bounds: every occupancy byte read lies inside the bounding box of two nodes, both inside the grid (the host checks the node
// list); a node index is used only after a check against M; rows of the matrix are read in words [0, ceil(M / 64)) only.
#pragma once

namespace pf {

#ifndef PF_SIGHT_LDS_NODES
#define PF_SIGHT_LDS_NODES 16384                /* labels of a set live in LDS up to this many nodes, in the output row above */
#endif
#define PF_SIGHT_GROUP 1024
#define PF_SIGHT_THREADS 256
#define PF_SIGHT_WORDS_MAX 256                  /* ceil(PF_SIGHT_NODES_MAX / 64) */
#define PF_SIGHT_ST_OK 0
#define PF_SIGHT_ST_RANGE 1
#define PF_SIGHT_ST_INFEASIBLE 2
#define PF_SIGHT_ST_OVERFLOW 3
#define PF_SIGHT_ST_PARENTS 4

// rc [M]: (r << 16) | c of every node (R, C < 2^16: the host's R^2 + C^2 < 2^31 - 1)
__global__ __launch_bounds__(PF_SIGHT_THREADS) void k_sight_node_coords(const int* __restrict__ nodes, int M, int C, int* __restrict__ rc) {
  const int i = (int)(blockIdx.x * PF_SIGHT_THREADS + threadIdx.x);
  if (i >= M) return;
  const int a = nodes[i], r = a / C;
  rc[i] = (r << 16) | (a - r * C);
}

__global__ __launch_bounds__(PF_SIGHT_THREADS) void k_sight_pack_lane_per_pair(const uint8_t* __restrict__ occ, int C, int strict, int range_sq, int M,
                                                                              const int* __restrict__ nodes, unsigned long long* __restrict__ adj, int ld) {
  const int W = (M + 63) >> 6;
  const int w = (int)(blockIdx.x * (PF_SIGHT_THREADS / 64) + (threadIdx.x >> 6));
  if (w >= W) return;                                                 // (the whole wavefront)
  const int lane = (int)(threadIdx.x & 63u), j = w * 64 + lane;
  const bool live = j < M;
  const int v = nodes[live ? j : M - 1];
  const int r1 = v / C, c1 = v - r1 * C;
  for (int i = (int)blockIdx.y; i < M; i += (int)gridDim.y) {
    const int a = nodes[i];                                           // (the same word in every lane)
    bool s = false;
    if (live && occ[a] != 1) {
      const int r0 = a / C, c0 = a - r0 * C;
      s = vis_lane_target(occ, C, a, r0, c0, v, r1, c1, strict, range_sq);
    }
    const unsigned long long word = __ballot(s);
    if (lane == 0) adj[(size_t)i * (size_t)ld + (size_t)w] = word;
  }
}

// ctl [4], zeroed by the host: {the largest (degree << 32) | ~i, set off-diagonal bits, nodes without their diagonal bit, -}
__global__ __launch_bounds__(PF_SIGHT_THREADS) void k_sight_pack_info_reduce(const unsigned long long* __restrict__ adj, int ld, int M, unsigned long long* __restrict__ ctl) {
  const int W = (M + 63) >> 6;
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = (int)(blockIdx.x * (PF_SIGHT_THREADS / 64) + (threadIdx.x >> 6)), waves = (int)(gridDim.x * (PF_SIGHT_THREADS / 64));
  unsigned long long best = 0, bits = 0, blocked = 0;
  for (int i = wave; i < M; i += waves) {                             // a wavefront a row, the lanes on its words
    const unsigned long long* const row = adj + (size_t)i * (size_t)ld;
    int deg = 0;
    for (int k = lane; k < W; k += 64) deg += __popcll(row[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) deg += __shfl_xor(deg, d);
    const int diag = (int)((row[i >> 6] >> (i & 63)) & 1ull);
    deg -= diag;
    const unsigned long long key = ((unsigned long long)(unsigned)deg << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    best = key > best ? key : best;
    bits += (unsigned long long)deg;
    blocked += (unsigned long long)(1 - diag);
  }
  if (lane == 0 && wave < M) {
    atomicMax(ctl, best);
    if (bits) atomicAdd(ctl + 1, bits);
    if (blocked) atomicAdd(ctl + 2, blocked);
  }
}

__global__ void k_sight_pack_write_info(const unsigned long long* __restrict__ ctl, long long* __restrict__ info) {
  if (blockIdx.x || threadIdx.x) return;
  info[0] = (long long)ctl[1];
  info[1] = (long long)(ctl[0] >> 32);
  info[2] = (long long)(0xFFFFFFFFu - (unsigned)(ctl[0] & 0xFFFFFFFFull));
  info[3] = (long long)ctl[2];
}

__device__ __forceinline__ double sight_weight(int rcu, int rcv) {
  const int dr = (rcu >> 16) - (rcv >> 16), dc = (rcu & 0xFFFF) - (rcv & 0xFFFF);
  return __builtin_sqrt((double)(dr * dr + dc * dc));
}

// One workgroup per source set.  work [4], zeroed by the host: {the most rounds of a set, rounds over all sets, candidate sums
// formed, labels lowered}.
template <bool LDS>
__global__ __launch_bounds__(PF_SIGHT_GROUP) void k_sight_field_group_per_set(const unsigned long long* __restrict__ adj, int ld, int M, const int* __restrict__ rc, int B,
                                                                             const int* __restrict__ set_off, const int* __restrict__ src, double* dist,
                                                                             long long* __restrict__ info, unsigned long long* __restrict__ work) {
  extern __shared__ double sight_lds[];
  __shared__ unsigned long long chg[2][PF_SIGHT_WORDS_MAX];
  __shared__ unsigned long long red[4];                               // finite labels, sources, the largest label's bits, the smallest index that holds it
  const int t = (int)threadIdx.x, W = (M + 63) >> 6;
  const double inf = __builtin_inf();
  unsigned long long formed = 0, lowered = 0;
  for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
    double* const row = dist + (size_t)b * (size_t)M;
    double* const lab = LDS ? sight_lds : row;
    for (int v = t; v < M; v += PF_SIGHT_GROUP) lab[v] = inf;
    for (int k = t; k < W; k += PF_SIGHT_GROUP) chg[0][k] = 0;
    if (t < 4) red[t] = t == 3 ? ~0ull : 0ull;
    __syncthreads();
    for (int j = set_off[b] + t; j < set_off[b + 1]; j += PF_SIGHT_GROUP) {
      const int s = src[j];                                           // (in [0, M): the host's check)
      if ((adj[(size_t)s * (size_t)ld + (size_t)(s >> 6)] >> (s & 63)) & 1ull) {
        lab[s] = 0.0;                                                 // (a source listed twice stores the same word twice)
        atomicOr(&chg[0][s >> 6], 1ull << (s & 63));
      }
    }
    __syncthreads();
    int cur = 0, rounds = 0;
    for (;;) {
      for (int k = t; k < W; k += PF_SIGHT_GROUP) chg[cur ^ 1][k] = 0;
      __syncthreads();
      int fell = 0;
      for (int v = t; v < M; v += PF_SIGHT_GROUP) {
        const unsigned long long* const arow = adj + (size_t)v * (size_t)ld;
        const int rcv = rc[v];
        const double dv = lab[v];
        double best = dv;
        for (int k = 0; k < W; ++k) {
          const unsigned long long cw = chg[cur][k];                  // (one LDS word for the whole wavefront: the skip is uniform)
          if (!cw) continue;
          unsigned long long m = arow[k] & cw;
          while (m) {
            const int u = (k << 6) + __builtin_ctzll(m);
            m &= m - 1;
            const double cand = lab[u] + sight_weight(rc[u], rcv);
            best = cand < best ? cand : best;
            formed += 1;
          }
        }
        if (best < dv) {
          lab[v] = best;
          atomicOr(&chg[cur ^ 1][v >> 6], 1ull << (v & 63));
          fell = 1;
          lowered += 1;
        }
      }
      rounds += 1;
      if (!__syncthreads_or(fell)) break;
      cur ^= 1;
    }
    // the row (where the labels sat in LDS) and the info words
    int finite = 0, zero = 0;
    unsigned long long top = 0;
    for (int v = t; v < M; v += PF_SIGHT_GROUP) {
      const double d = lab[v];
      if (LDS) row[v] = d;
      if (d < inf) {
        finite += 1;
        zero += d == 0.0;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(d);   // (d >= 0: the bits order as the values)
        top = bits > top ? bits : top;
      }
    }
    if (info) {
      if (finite) { atomicAdd(&red[0], (unsigned long long)finite); atomicMax(&red[2], top); }
      if (zero) atomicAdd(&red[1], (unsigned long long)zero);
      __syncthreads();
      const unsigned long long most = red[2];
      for (int v = t; v < M; v += PF_SIGHT_GROUP) {
        const double d = LDS ? lab[v] : row[v];
        if (d < inf && (unsigned long long)__double_as_longlong(d) == most) { atomicMin(&red[3], (unsigned long long)v); break; }
      }
      __syncthreads();
      if (t == 0) {
        long long* const o = info + 4 * (size_t)b;
        o[0] = (long long)red[0];
        o[1] = (long long)red[1];
        o[2] = red[0] ? (long long)red[3] : -1;
        o[3] = 0;
      }
    }
    if (t == 0) {
      atomicMax(work, (unsigned long long)rounds);
      atomicAdd(work + 1, (unsigned long long)rounds);
    }
    __syncthreads();                                                  // (red and lab are the next set's)
  }
  // the two sums of this workgroup: per wavefront, then one atomic each
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    formed += __shfl_xor(formed, d);
    lowered += __shfl_xor(lowered, d);
  }
  if ((t & 63) == 0) {
    if (formed) atomicAdd(work + 2, formed);
    if (lowered) atomicAdd(work + 3, lowered);
  }
}

// parent [B][M]: a thread per (set, node), the bits of the node's row in increasing order, out at the first match
__global__ __launch_bounds__(PF_SIGHT_THREADS) void k_sight_parents(const unsigned long long* __restrict__ adj, int ld, int M, const int* __restrict__ rc, int B,
                                                                   const double* __restrict__ dist, int* __restrict__ parent) {
  const int v = (int)(blockIdx.x * PF_SIGHT_THREADS + threadIdx.x);
  if (v >= M) return;
  const int W = (M + 63) >> 6;
  const unsigned long long* const arow = adj + (size_t)v * (size_t)ld;
  const int rcv = rc[v];
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const double* const lab = dist + (size_t)b * (size_t)M;
    const double dv = lab[v];
    int p = -1;
    if (dv < __builtin_inf() && dv > 0.0) {
      for (int k = 0; k < W && p < 0; ++k) {
        unsigned long long m = arow[k];
        while (m) {
          const int u = (k << 6) + __builtin_ctzll(m);
          m &= m - 1;
          const double du = lab[u];
          if (du < dv && du + sight_weight(rc[u], rcv) == dv) { p = u; break; }
        }
      }
    }
    parent[(size_t)b * (size_t)M + (size_t)v] = p;
  }
}

// A thread per query: the chain is counted first, then written, then the row is summed from the source's end.
__global__ __launch_bounds__(PF_SIGHT_THREADS) void k_sight_paths(int M, const int* __restrict__ nodes, int C, int B, const double* __restrict__ dist,
                                                                 const int* __restrict__ parent, int n, const int* __restrict__ set, const int* __restrict__ target,
                                                                 int reverse, int way_cap, int* __restrict__ way, int* __restrict__ way_len, double* __restrict__ stats,
                                                                 int* __restrict__ status) {
  const int q = (int)(blockIdx.x * PF_SIGHT_THREADS + threadIdx.x);
  if (q >= n) return;
  const int b = set ? set[q] : 0, tgt = target[q];
  int st = PF_SIGHT_ST_OK, L = 0;
  double length = 0.0;
  int turns = 0;
  if ((unsigned)b >= (unsigned)B || (unsigned)tgt >= (unsigned)M) st = PF_SIGHT_ST_RANGE;
  else {
    const double* const lab = dist + (size_t)b * (size_t)M;
    const int* const par = parent + (size_t)b * (size_t)M;
    if (!(lab[tgt] < __builtin_inf())) st = PF_SIGHT_ST_INFEASIBLE;
    else {
      int v = tgt;
      L = 1;
      for (;;) {
        const int p = par[v];
        if (p == -1) break;
        if ((unsigned)p >= (unsigned)M || L >= M) { st = PF_SIGHT_ST_PARENTS; break; }   // (M nodes at most: a longer chain repeats one)
        v = p;
        L += 1;
      }
      if (st == PF_SIGHT_ST_OK && lab[v] != 0.0) st = PF_SIGHT_ST_PARENTS;               // the chain ends at a node that is no source
      if (st == PF_SIGHT_ST_OK && L > way_cap) st = PF_SIGHT_ST_OVERFLOW;
      if (st == PF_SIGHT_ST_OK) {
        int* const out = way + (size_t)q * (size_t)way_cap;
        v = tgt;
        for (int i = 0; i < L; ++i) {                                 // position from the target's end
          out[reverse ? i : L - 1 - i] = nodes[v];
          if (i + 1 < L) v = par[v];
        }
        int pr = 0, pc = 0, pdr = 0, pdc = 0;
        for (int i = 0; i < L; ++i) {                                 // source -> target, whichever way the row runs
          const int cell = out[reverse ? L - 1 - i : i];
          const int r = cell / C, c = cell - r * C;
          if (i > 0) {
            const int dr = r - pr, dc = c - pc;
            length = length + __builtin_sqrt((double)(dr * dr + dc * dc));
            if (i > 1 && (pdr * dc - pdc * dr != 0 || pdr * dr + pdc * dc < 0)) turns += 1;
            pdr = dr; pdc = dc;
          }
          pr = r; pc = c;
        }
      }
    }
  }
  const bool ok = st == PF_SIGHT_ST_OK;
  way_len[q] = ok ? L : 0;
  status[q] = st;
  if (stats) { stats[2 * (size_t)q] = ok ? length : 0.0; stats[2 * (size_t)q + 1] = ok ? (double)turns : 0.0; }
}

}  // namespace pf
