// pf_mpa_batch.h -- K independent MPA schools in one batched sweep (pf_mpa_batch_*), included by pathfit.hip after the solo MPA
// kernels and the rank sort.
//
// A school is one MPA population: its own seed, start and target; all schools share the grid, N predators, the hyper-parameters
// and the score parameters.  Everything that differs between schools lives in one MpaSchool entry in HBM.  The buffers of a
// batch hold the schools back to back: predator a of school k is row k N + a of the population / candidate buffers, its
// position in the school's fitness-sorted list is entry k N + i of the order array (which holds LOCAL slots 0 .. N - 1), and the
// sweep's items are [0, K N) phase items, [K N, 2 K N) FADs items -- the layout k_mpa_search already expects with n = K N.
//
// The batched kernels do no MPA arithmetic of their own: they map their index to (school, predator), build the school's view
// of the launch arguments (school_view: base pointers moved to the school's rows, start / target / seed / bounds / elite /
// initial path from the table) and call the very item functions the solo kernels call (mpa_propose_item, mpa_plan_item,
// mpa_finish_item, mpa_fads_est_item, mpa_apply_item), so school k computes what a solo run computes by construction.
// k_mpa_search is launched as it is: a job carries everything a search needs.
//
// Every kernel here is a template (PF_LATE, always 0) for one reason: the compiler emits template instantiations after the
// plain functions, in the order of their first use, and these are first used after pf_mpa_iter_batch.  So they land BEHIND
// every kernel the code object had before, whose addresses -- and with them the PC-relative literals of k_mpa_search,
// k_astar_batch and k_decode_batch -- stay what they were: those kernels are byte for byte the parent's.
struct __attribute__((aligned(16))) MpaSchool {
  unsigned long long seed;
  int start, target;
  const double* ds; const double* dt;                    // bound tables (null: no pruning for this batch), shared by schools with the same cell
  const int* init_cells; const double* init_stats;       // memoised MPA._generate_initial_path() (MPA.py:154; FADs re-init :405)
  int init_len, pad_;                                    // 0: the target is unreachable
  int* elite_cells; int* elite_len; double* elite_stats; // the school's elite of the iteration (MPA.py:334)
};
struct MpaSchools { const MpaSchool* tab; int K, N, prune; };

__host__ __device__ __forceinline__ void school_view(MpaPhaseArgs& p, const MpaSchool& s, const MpaSchools& ms, int k) {
  const size_t o = (size_t)k * (size_t)ms.N;
  p.seed = s.seed; p.n = ms.N;
  p.m.start = s.start; p.m.target = s.target;
  p.m.ds = ms.prune ? s.ds : nullptr; p.m.dt = ms.prune ? s.dt : nullptr;
  p.pop_cells += o * p.path_cap; p.pop_len += o; p.pop_stats += o * 5;
  p.slot += o;                                           // (gidx is the same 0 .. N - 1 for every school)
  p.elite_cells = s.elite_cells; p.elite_len = -1; p.elite_len_dev = s.elite_len; p.elite_stats = s.elite_stats;
  p.out_cells += o * p.path_cap; p.out_len += o; p.out_stats += o * 5; p.status += o;
  p.prop += o;
}
__host__ __device__ __forceinline__ void school_view(MpaFadsArgs& f, const MpaSchool& s, const MpaSchools& ms, int k) {
  const size_t o = (size_t)k * (size_t)ms.N;
  f.seed = s.seed; f.n = ms.N;
  f.m.start = s.start; f.m.target = s.target;
  f.m.ds = ms.prune ? s.ds : nullptr; f.m.dt = ms.prune ? s.dt : nullptr;
  f.pop_cells += o * f.path_cap; f.pop_len += o; f.pop_stats += o * 5;
  f.slot += o; f.status += o;
  f.init_cells = s.init_cells; f.init_len = s.init_len; f.init_stats = s.init_stats;
  f.cand_cells += o * f.path_cap; f.cand_len += o; f.cand_stats += o * 5;
}

// proposals of all K N predators (k_mpa_propose): doubtful ones are listed under their index in the batch
template <int PF_LATE = 0>
__global__ void k_mpa_propose_batch(MpaPhaseArgs p0, MpaSchools ms, float* est) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ms.K * ms.N) return;
  const int k = g / ms.N, a = g - k * ms.N;
  MpaPhaseArgs p = p0;
  school_view(p, ms.tab[k], ms, k);
  mpa_propose_item(p, a, g, est + (size_t)k * ms.N);
}
template <int PF_LATE = 0>
__global__ void k_plan_mpa_fads_batch(MpaFadsArgs f0, MpaSchools ms, float* est) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ms.K * ms.N) return;
  const int k = g / ms.N, a = g - k * ms.N;
  MpaFadsArgs f = f0;
  school_view(f, ms.tab[k], ms, k);
  mpa_fads_est_item(f, a, est + (size_t)k * ms.N);
}
// one wave per item of the 2 K N (k_mpa_plan / k_mpa_finish)
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_mpa_plan_batch(MpaSweepArgs q, MpaSchools ms, MpaJob* jobs, MpaRes* res) {
  const int KN = ms.K * ms.N;
  const int item = blockIdx.x;
  if (item >= 2 * KN) return;
  const bool isph = item < KN;
  const int g = isph ? item : item - KN;
  const int k = g / ms.N, a = g - k * ms.N;
  MpaPhaseArgs p = q.ph; MpaFadsArgs f = q.fd;
  school_view(p, ms.tab[k], ms, k); school_view(f, ms.tab[k], ms, k);
  mpa_plan_item(p, f, isph, a, item, jobs, res);
}
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_mpa_finish_batch(MpaSweepArgs q, MpaSchools ms, const MpaJob* jobs, const MpaRes* res) {
  const int KN = ms.K * ms.N;
  const int item = blockIdx.x;
  if (item >= 2 * KN) return;
  const bool isph = item < KN;
  const int g = isph ? item : item - KN;
  const int k = g / ms.N, a = g - k * ms.N;
  MpaPhaseArgs p = q.ph; MpaFadsArgs f = q.fd;
  school_view(p, ms.tab[k], ms, k); school_view(f, ms.tab[k], ms, k);
  mpa_finish_item(p, f, isph, a, item, jobs, res);
}
// memory step + FADs acceptance (k_mpa_apply): predator g of the batch sits in row (its school's first row) + slots[g]
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_mpa_apply_batch(int KN, int N, int path_cap, const int* slots, const int* c1_cells, const int* c1_len,
                                                        const double* c1_stats, const int* c2_cells, const int* c2_len,
                                                        const double* c2_stats, int* pop_cells, int* pop_len, double* pop_stats) {
  const int g = blockIdx.x;
  if (g >= KN) return;
  mpa_apply_item(g, (g / N) * N + slots[g], path_cap, c1_cells, c1_len, c1_stats, c2_cells, c2_len, c2_stats, pop_cells, pop_len, pop_stats);
}

// ---- the segmented stable sort: K rank sorts of n keys in one launch sequence (K8, mode 0) ------------------------------
// Segment s sorts entries [s n, (s + 1) n) of the order array among themselves; ranks count only the segment's own keys, so
// the work is K n^2 / 64 wave-iterations, not (K n)^2 / 64, and no school's order ever sees another's keys.
template <int PF_LATE = 0>
__global__ void k_sort_prep_seg(int K, int n, const double* vals, int stride, int offset, const int* order,
                                unsigned long long* key, int* payload, unsigned* rank) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K * n) return;
  const int seg = i / n, id = order[i];
  key[i] = key_image_f64(vals[((size_t)seg * n + id) * stride + offset]); payload[i] = id;
  rank[i] = 0u;
}
template <int PF_LATE = 0>
__global__ __launch_bounds__(64) void k_rank_count_seg(int n, int per_seg, int jsplit, int jchunk, const unsigned long long* __restrict__ key,
                                                       unsigned* __restrict__ rank) {
  const unsigned seg = blockIdx.x / (unsigned)per_seg, blk = blockIdx.x - seg * (unsigned)per_seg;
  rank_count_block(blk, n, jsplit, jchunk, key + (size_t)seg * n, rank + (size_t)seg * n);
}
template <int PF_LATE = 0>
__global__ void k_rank_scatter_seg(int K, int n, const unsigned* rank, const int* payload, int* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K * n) return;
  out[(size_t)(i / n) * n + rank[i]] = payload[i];                  // rank < n: it counts keys of the segment other than i
}

// the elite of every school (k_mpa_pick_elite): one block per school, into the school's own elite buffers
template <int PF_LATE = 0>
__global__ __launch_bounds__(256) void k_mpa_pick_elite_batch(MpaSchools ms, int path_cap, const int* pop_cells, const int* pop_len,
                                                             const double* pop_stats, const int* order) {
  const int k = blockIdx.x;
  if (k >= ms.K) return;
  const MpaSchool s = ms.tab[k];
  const size_t row = (size_t)k * ms.N + order[(size_t)k * ms.N];
  const int L = pop_len[row];
  for (int i = threadIdx.x; i < L; i += 256) s.elite_cells[i] = pop_cells[row * path_cap + i];
  if (threadIdx.x < 5) s.elite_stats[threadIdx.x] = pop_stats[row * 5 + threadIdx.x];
  if (threadIdx.x == 0) *s.elite_len = L;
}
// population[0] of every school after the sort (MPA.py:413): out[6 k ...] = {slot, stats[5]}, one copy for the host
template <int PF_LATE = 0>
__global__ void k_mpa_best_rows(int K, int N, const double* pop_stats, const int* order, double* out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int slot = order[(size_t)k * N];
  out[6 * k] = (double)slot;
  for (int i = 0; i < 5; ++i) out[6 * k + 1 + i] = pop_stats[((size_t)k * N + slot) * 5 + i];
}
