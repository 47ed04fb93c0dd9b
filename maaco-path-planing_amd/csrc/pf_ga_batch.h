// pf_ga_batch.h -- K independent GA populations in one batched generation (pf_ga_*_batch), included at the end of pathfit.hip.
//
// Population k has its own seed, start and target; all populations share the grid, N, W and the rates.  Every buffer holds the
// populations back to back: individual i of population k is row k N + i, and the ids inside the order / parent arrays
// (d_gorder, d_psid) are LOCAL (0 .. N - 1), the layout of pf_mpa_batch.h.  The kernels here do no GA arithmetic of their own:
// they map their index to (population, item), move the base pointers to the population's rows and call the item functions the
// solo kernels call (ga_select_item, ga_breed_item, ga_assemble_item), so population k computes what a solo generation computes
// by construction.  The decode of all K N children is ONE k_decode_multi launch (csrc/pf_decode.h), the K sorts are the segmented
// rank sort and the K best rows come from k_mpa_best_rows (both pf_mpa_batch.h).
//
// Templates on a dummy parameter for the reason given in pf_mpa_batch.h: they are emitted behind every kernel the code object
// had, so none of those moves.

// K replays of the generation's selection stream (seeds[k], DOM_GA_SELECT, gen, 0) side by side: the replay is sequential by
// nature (k_ga_select), so a population gets a wavefront of its own rather than a lane -- 64 diverged replays in one wavefront
// would run one after another.  pool: K N ints.
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_ga_select_batch(const unsigned long long* seeds, int gen, int K, int N, int k_tour, const double* fit_all,
                                                        const int* gorder, int* pool, int* psid) {
  const int k = blockIdx.x;
  if (k >= K || threadIdx.x != 0) return;
  const size_t o = (size_t)k * N;
  ga_select_item(seeds[k], gen, N, k_tour, fit_all + o, gorder + o, pool + o, psid + o);
}
// one thread per (population, pair of children): stream (seeds[k], DOM_GA, gen, pair), parents from the population's own rows
template <int PF_LATE = 0>
__global__ void k_ga_breed_batch(const unsigned long long* seeds, int gen, int K, int N, int W, double cx_rate, double mut_rate,
                                 const uint8_t* occ, int R, int C, const int* chrom_all, const int* psid, int* out) {
  const int pairs = (N + 1) / 2;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= K * pairs) return;
  const int k = g / pairs, pair = g - k * pairs;
  const size_t o = (size_t)k * N;
  ga_breed_item(seeds[k], gen, N, W, cx_rate, mut_rate, occ, R, C, chrom_all + o * W, psid + o, 0, N, out + o * W, pair);
}
// one block per (population, child); a fallback parent is psid[k N + i], a row of the population's own old rows (one GPU: every
// row is present, old_lo = 0, old_hi = N)
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_ga_assemble_batch(int K, int N, int W, int cap, const int* kid_len, const int* kid_chrom,
                                                          const double* kid_stats, const int* kid_cells, const int* psid,
                                                          const int* chrom_old, const double* stats_old, const int* cells_old,
                                                          const int* len_old, int* chrom_new, double* stats_new, int* cells_new, int* len_new) {
  const int g = blockIdx.x;
  if (g >= K * N) return;
  const int k = g / N, i = g - k * N;
  const size_t o = (size_t)k * N;
  ga_assemble_item(i, threadIdx.x, W, cap, 0, kid_len + o, kid_chrom + o * W, kid_stats + o * 5, kid_cells + o * cap, psid + o,
                   chrom_old + o * W, stats_old + o * 5, cells_old + o * cap, len_old + o, 0, N, chrom_new + o * W, stats_new + o * 5,
                   cells_new + o * cap, len_new + o);
}
