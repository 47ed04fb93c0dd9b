// pf_pso_batch.h -- K independent PSO swarms in one batched sweep (pf_pso_*_batch), included at the end of pathfit.hip.
//
// Swarm k has its own seed, start and target; all swarms share the grid, N, W and the coefficients.  Every per-particle buffer
// holds the swarms back to back -- particle a of swarm k is row k N + a, a LOCAL (0 .. N - 1), the layout of pf_mpa_batch.h /
// pf_ga_batch.h -- and every per-swarm buffer (gbest [K][2W], gstats [K][5], gpath [K][cap + 1], gfit [K], seeds [K]) has row k.
//
// A round of the asynchronous sweep evaluates, for every swarm, its particles [cur[k], N): cur[k] is the first particle whose
// evaluation is not final yet (pso.py:222-229: a particle sees the gbest as the particles before it left it).  The round's ITEMS
// are these segments back to back; tab = int32 [2 K + 1] = { off[0 .. K] (off[k] = first item of swarm k, off[K] = n), cur[0 .. K) }
// is the one table the host uploads per round.  Item i of swarm k is particle a = cur[k] + i - off[k].
//
// Compact staging instead of update-in-place plus roll-back: k_pso_update_batch reads the particle's rows and writes the NEW
// position and velocity into staging row i, next to the item's start / target cell and its row k N + a; ONE k_decode_multi launch
// decodes the n staging rows; k_pso_scan_batch finds every swarm's improver; k_pso_commit_batch copies the staging rows of the
// FINAL items into the swarm's rows.  An item that is not final leaves no trace: the next round reads its unchanged rows and gbest
// row k, which has moved by then, and draws the same numbers (the stream is keyed by (seed, iteration, particle)).
//
// The kernels carry no PSO arithmetic of their own: they map their index to (swarm, particle), move the base pointers and call
// the item functions the solo kernels call (pso_update_item, pso_scan_item, pso_commit_item), so swarm k computes what a solo
// sweep computes by construction.  Templates on a dummy parameter for the reason given in pf_mpa_batch.h: they are emitted behind
// every kernel the code object had, so none of those moves.

struct PsoScanRec { int idx, ovf; double fit; };   // one per swarm and round: improver (index inside the segment, or -1), status-3 items, fitness

// the swarm of item i: the last k with off[k] <= i (empty segments share their offset with the next swarm and are stepped over)
PF_DEV int pso_item_swarm(const int* off, int K, int i) {
  int lo = 0, hi = K - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= i) lo = mid; else hi = mid - 1; }
  return lo;
}

// thread per (item, waypoint): pso.py:186-202 with gbest row k and seeds[k], stream (seeds[k], DOM_PSO, iter, a).  p.n = items,
// p.pos / p.vel / p.pbest / p.gbest = the swarms' rows (read only here), s_* = the staging rows.
template <int PF_LATE = 0>
__global__ void k_pso_update_batch(PsoArgs p, int K, int N, const unsigned long long* seeds, const int* tab, const int* starts, const int* targets,
                                   double* s_pos, double* s_vel, int* s_start, int* s_target, int* s_row) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.n * p.W) return;
  const int i = t / p.W, d = t - i * p.W;
  const int k = pso_item_swarm(tab, K, i);
  const int a = tab[K + 1 + k] + (i - tab[k]);
  pso_update_item(p, seeds[k], (unsigned long long)a, d, p.gbest + (size_t)k * p.W * 2, (((size_t)k * N + a) * p.W + d) * 2, s_pos, s_vel,
                  ((size_t)i * p.W + d) * 2);                     // (p.pos_keep is null: nothing is kept, nothing is rolled back)
  if (d == 0) { s_start[i] = starts[k]; s_target[i] = targets[k]; s_row[i] = k * N + a; }
}

// one block per swarm: k_pso_scan over the swarm's segment of the staging rows against its own pbest fitnesses and gfit[k]; a
// swarm without items gets (-1, 0, inf)
template <int PF_LATE = 0>
__global__ __launch_bounds__(256) void k_pso_scan_batch(int K, int N, int sync_mode, const int* tab, const double* s_stats, const int* s_len,
                                                        const int* s_status, const double* pbf, const double* gfit, PsoScanRec* rec) {
  const int k = blockIdx.x;
  if (k >= K) return;
  const int o = tab[k], n = tab[k + 1] - o;
  pso_scan_item(n, s_stats + (size_t)o * 5, s_len + o, s_status + o, pbf + (size_t)k * N + tab[K + 1 + k], gfit[k], sync_mode, &rec[k].idx, &rec[k].fit);
}

// block per item.  Asynchronous: the items at or before the swarm's improver are final (all of the segment if there is none);
// synchronous: every item is.  A final item's staging rows become the particle's current position / velocity / path / length /
// stats, then pso_commit_item: pso.py:216-220 against the OLD pbest, and for the improver pso.py:222-229 into gbest row k.
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_pso_commit_batch(int n, int K, int N, int W, int path_cap, int sync_mode, const int* tab, const PsoScanRec* rec,
                                                         const int* s_row, const double* s_pos, const double* s_vel, const double* s_stats,
                                                         const int* s_len, const int* s_cells, double* pos, double* vel, double* stats, int* len,
                                                         int* cells, double* pbest, double* pbest_fit, int* pb_cells, int* pb_len, double* gb,
                                                         double* gstats, int* gpath, double* gfit) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= n) return;
  const int row = s_row[i], k = row / N;
  const int li = i - tab[k], j = rec[k].idx;
  if (!sync_mode && j >= 0 && li > j) return;                     // evaluated on a gbest that has moved since: nothing is written
  const size_t w0 = (size_t)row * W * 2, s0 = (size_t)i * W * 2;
  const int L = s_len[i];
  const double fit = s_stats[(size_t)i * 5 + 4];
  for (int x = t; x < W * 2; x += 64) { pos[w0 + x] = s_pos[s0 + x]; vel[w0 + x] = s_vel[s0 + x]; }
  for (int x = t; x < L; x += 64) cells[(size_t)row * path_cap + x] = s_cells[(size_t)i * path_cap + x];
  if (t < 5) stats[(size_t)row * 5 + t] = s_stats[(size_t)i * 5 + t];
  if (t == 0) { len[row] = L; if (li == j) gfit[k] = fit; }
  pso_commit_item(t, W, li == j, L, fit, s_pos + s0, s_stats + (size_t)i * 5, s_cells + (size_t)i * path_cap, pbest + w0, pbest_fit + row,
                  pb_cells + (size_t)row * path_cap, pb_len + row, gb + (size_t)k * W * 2, gstats + (size_t)k * 5, gpath + (size_t)k * (path_cap + 1));
}
