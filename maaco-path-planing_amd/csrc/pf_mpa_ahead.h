// pf_mpa_ahead.h -- D consecutive MPA iterations of ONE population in one sweep (pf_mpa_iter_ahead), included at the end of
// pathfit.hip.
//
// An iteration that accepts no candidate leaves the population untouched: the stable sort at its end re-sorts unchanged keys, so
// the list order, the elite and every (seed, DOM, iter, position) stream input of the next iteration are what they were.  The
// jobs of iteration it + 1 are then computable before the sweep of iteration it has run, and the two sweeps can share one work
// queue.  A "level" is one such iteration: level d has its own (phase, CF, iter) and its own candidate rows; the population,
// the list (gidx / slot) and the elite are shared and read-only while the sweep runs.  Level 0 is applied with the sweep; a later
// level is applied only once every level before it is known to have accepted nothing (pf_mpa_ahead_take), and thrown away
// otherwise -- so a run computes what it computes one iteration at a time, exactly.
//
// The layout is that of pf_mpa_batch.h with "school" read as "level": level d's candidate rows are rows [d N, (d + 1) N) of the
// level buffers, the sweep's items are [0, D N) phase items and [D N, 2 D N) FADs items -- what k_mpa_search expects with
// n = D N -- and one longest-first queue orders all of them together.  The kernels do no MPA arithmetic of their own: they map
// their index to (level, predator), build the level's view of the launch arguments (level_view: the iteration's scalars and the
// level's candidate rows) and call the item functions the solo kernels call.
//
// Every kernel is a template on a dummy parameter for the reason given in pf_mpa_batch.h: it is emitted behind every kernel the
// code object had before, which therefore stay byte for byte what they were.
#define PF_AHEAD_MAX 16
struct MpaLevel { int phase, iter; double CF; };
struct MpaLevels { MpaLevel lv[PF_AHEAD_MAX]; int D, N; };

__host__ __device__ __forceinline__ void level_view(MpaPhaseArgs& p, const MpaLevels& ls, int d) {
  const size_t o = (size_t)d * (size_t)ls.N;
  p.phase = ls.lv[d].phase; p.iter = ls.lv[d].iter; p.CF = ls.lv[d].CF;
  p.out_cells += o * p.path_cap; p.out_len += o; p.out_stats += o * 5; p.status += o;
  p.prop += o;
}
__host__ __device__ __forceinline__ void level_view(MpaFadsArgs& f, const MpaLevels& ls, int d) {
  const size_t o = (size_t)d * (size_t)ls.N;
  f.iter = ls.lv[d].iter; f.CF = ls.lv[d].CF;
  f.status += o;
  f.cand_cells += o * f.path_cap; f.cand_len += o; f.cand_stats += o * 5;
}

// proposals of the D N phase items (k_mpa_propose; doubtful ones are listed under their index in the launch) and work estimates
// of the D N FADs items (k_plan_mpa_fads): thread g < D N proposes, thread D N + g estimates -- est[] is the queue's, item order
template <int PF_LATE = 0>
__global__ void k_mpa_estimates_ahead(MpaPhaseArgs p0, MpaFadsArgs f0, MpaLevels ls, float* est) {
  const int DN = ls.D * ls.N;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * DN) return;
  const bool isph = t < DN;
  const int g = isph ? t : t - DN;
  const int d = g / ls.N, a = g - d * ls.N;
  if (isph) {
    MpaPhaseArgs p = p0;
    level_view(p, ls, d);
    mpa_propose_item(p, a, g, est + (size_t)d * ls.N);
  } else {
    MpaFadsArgs f = f0;
    level_view(f, ls, d);
    mpa_fads_est_item(f, a, est + (size_t)DN + (size_t)d * ls.N);
  }
}
// one wave per item of the 2 D N (k_mpa_plan / k_mpa_finish)
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_mpa_plan_ahead(MpaSweepArgs q, MpaLevels ls, MpaJob* jobs, MpaRes* res) {
  const int DN = ls.D * ls.N;
  const int item = blockIdx.x;
  if (item >= 2 * DN) return;
  const bool isph = item < DN;
  const int g = isph ? item : item - DN;
  const int d = g / ls.N, a = g - d * ls.N;
  MpaPhaseArgs p = q.ph; MpaFadsArgs f = q.fd;
  level_view(p, ls, d); level_view(f, ls, d);
  mpa_plan_item(p, f, isph, a, item, jobs, res);
}
// ... and the items per level that overflowed (what k_mpa_search and k_mpa_finish add up in DevCounters::overflow for the whole
// sweep): a searched item whose result says so, or an unsearched one whose plan says so.  lvl_ovf: [D], zeroed by the host.
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_mpa_finish_ahead(MpaSweepArgs q, MpaLevels ls, const MpaJob* jobs, const MpaRes* res,
                                                         unsigned long long* lvl_ovf) {
  const int DN = ls.D * ls.N;
  const int item = blockIdx.x;
  if (item >= 2 * DN) return;
  const bool isph = item < DN;
  const int g = isph ? item : item - DN;
  const int d = g / ls.N, a = g - d * ls.N;
  MpaPhaseArgs p = q.ph; MpaFadsArgs f = q.fd;
  level_view(p, ls, d); level_view(f, ls, d);
  mpa_finish_item(p, f, isph, a, item, jobs, res);
  if (threadIdx.x == 0) {
    const MpaJob j = jobs[item];
    if (j.kind != 0 ? res[item].rc == 3 : j.aux == 3) atomicAdd(&lvl_ovf[d], 1ull);
  }
}
// k_mpa_apply that also counts the predators it changes (*accepted, zeroed by the host): the count of a level is what decides
// whether the next level's candidates are still the next iteration's.
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_mpa_apply_count(int n, int path_cap, const int* slots, const int* c1_cells, const int* c1_len,
                                                        const double* c1_stats, const int* c2_cells, const int* c2_len,
                                                        const double* c2_stats, int* pop_cells, int* pop_len, double* pop_stats,
                                                        unsigned long long* accepted) {
  const int a = blockIdx.x;
  if (a >= n) return;
  const int slot = slots[a];
  // mpa_apply_item takes a candidate exactly when one of the two is fitter than the predator as it stands
  const double fit = pop_stats[(size_t)slot * 5 + 4];
  const bool take = c1_stats[(size_t)a * 5 + 4] < fit || (c2_len[a] > 0 && c2_stats[(size_t)a * 5 + 4] < fit);
  __syncthreads();                                                  // (every lane has read the fitness before lane 4 rewrites it)
  if (!take) return;
  if (threadIdx.x == 0) atomicAdd(accepted, 1ull);
  mpa_apply_item(a, slot, path_cap, c1_cells, c1_len, c1_stats, c2_cells, c2_len, c2_stats, pop_cells, pop_len, pop_stats);
}
