/*
 * pathfit.h -- C-ABI of the MI355X population-fitness engine (libpathfit.so).
 *
 * The reference (dvnam1605/MAACO-path-planing) has NO plugin / operator / FFI
 * interface: its boundary is the Python method surface of the solver classes
 * (SURVEY.md section 8b).  Each entry point below therefore names the
 * reference *method* whose per-agent inner loop it replaces, batched over the
 * population.  The Python facades in maaco-path-planing_amd/pathfit/ keep the
 * reference's class / constructor / solve() surface and call these through
 * ctypes (binding shown in INTEGRATION.md).
 *
 * Conventions
 *   - plain C: pointers, sizes, scalars; no C++/torch types.
 *   - every function returns 0 on success, <0 on error (pf_last_error()).
 *     Per-agent infeasibility is DATA (status arrays), never an error.
 *   - pointers named d_* are DEVICE pointers (pf_dev_alloc or any HIP
 *     allocation on the handle's device, e.g. torch tensor .data_ptr());
 *     all others are host pointers.
 *   - a cell is r*C + c (int32).  Paths are "strided CSR": agent a's cells are
 *     d_cells[a*path_cap .. a*path_cap + d_len[a]); d_len[a]==0 is the
 *     reference's [] (infeasible).
 *   - calls are synchronous at the ABI (they return after the handle's stream
 *     has drained) unless the name ends in _async.
 *   - one host thread per handle.
 *   - status codes: PF_ST_OK 0, PF_ST_INFEASIBLE 1 (reference returned []),
 *     PF_ST_STEP_CAP 2 (reference's 3RC / 2RC pop cap hit, also []),
 *     PF_ST_OVERFLOW 3 (engine scratch or path_cap too small: result not
 *     produced; never silently truncated), PF_ST_KEPT 4 (MPA: reference fell
 *     back to the unmodified path).
 */
#ifndef PATHFIT_H
#define PATHFIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PF_ST_OK 0
#define PF_ST_INFEASIBLE 1
#define PF_ST_STEP_CAP 2
#define PF_ST_OVERFLOW 3
#define PF_ST_KEPT 4

#define PF_ASTAR_REF 0 /* AStarSolver.solve semantics, astar.py:33-101 */
#define PF_ASTAR_MPA 1 /* MPA._a_star semantics, MPA.py:106-151 */
#define PF_ASTAR_DIJKSTRA 2 /* DijkstraSolver.solve semantics, dijkstra.py:32-97 (variant 0's loop with h == 0) */

typedef struct pf_handle pf_handle;

/* scoring weights: helper.calculate_path_stats (helper.py:98-113) when
 * variant==0, MPA._calculate_path_stats (MPA.py:215-229, safety==0) when 1 */
typedef struct {
  int32_t variant;
  int32_t restrict_policy; /* restrict_diagonal_near_obstacle_policy */
  double w_turn, w_safe, min_safe, diag_pen;
} pf_score_params;

/* MAACO constructor scalars, MAACO.py:11-14 */
typedef struct {
  double alpha, beta, rho, Q, a_turn_coef, wh_max, wh_min, k_h_adaptive, q0_initial, C0_initial_pheromone;
  int32_t num_iterations;
  int32_t start, target; /* cells */
} pf_maaco_params;

/* MPA scalars, MPA.py:10-18 (+ sigma = the Mantegna constant of :251-253,
 * computed by the caller with math.gamma) */
typedef struct {
  double P_const, levy_beta, levy_sigma, FADs_rate;
  int32_t num_predators; /* global population size (for the i < N//2 split, MPA.py:351) */
  int32_t start, target;
  int32_t allow_diag, restrict_corner;
} pf_mpa_params;

/* per-launch counters (roofline numerators) */
typedef struct {
  int64_t pops, pushes, nbr_examined, path_cells, steps, candidates, decrease_keys, overflow_agents;
  /* candidates: MAACO candidate cells examined; for the A*-based calls, open-list entries that took the spill list */
  int64_t pruned_rebuilds; /* MPA rebuilds skipped because a length bound proved the candidate could not be accepted */
  int64_t settled_searches;    /* closed-set searches answered by the parallel label-settling engine (certified equal) */
  int64_t sequential_searches; /* closed-set searches it could not certify: run by the sequential pop loop */
} pf_counters;

/* ---- lifecycle ---------------------------------------------------- */
const char* pf_version(void);
int pf_device_count(void);
/* grid: R*C bytes with the reference's cell values (env.py:4-7: 1 = obstacle,
 * anything else free).  Replaces np.array(grid, dtype=int) + obstacle_nodes
 * (helper.py:121-125).  device: HIP ordinal. */
int pf_create(const uint8_t* grid, int32_t R, int32_t C, int32_t device, pf_handle** out);
void pf_destroy(pf_handle* h);
/* Dynamic maps: replace the occupancy of an existing handle (same R x C, same cell values as pf_create).  The grid
 * preparation runs again on the device; call pf_maaco_setup / pf_mpa_setup again before the next solver batch. */
int pf_update_grid(pf_handle* h, const uint8_t* grid);
const char* pf_last_error(pf_handle* h); /* h may be NULL for create errors */
/* the handle's HIP stream (hipStream_t) so callers can order their own work */
void* pf_stream(pf_handle* h);
int pf_sync(pf_handle* h);

/* ---- device memory plumbing --------------------------------------- */
int pf_dev_alloc(pf_handle* h, int64_t bytes, void** d_out);
int pf_dev_free(pf_handle* h, void* d_ptr);
int pf_h2d(pf_handle* h, void* d_dst, const void* src, int64_t bytes);
int pf_d2h(pf_handle* h, void* dst, const void* d_src, int64_t bytes);
int pf_d2d(pf_handle* h, void* d_dst, const void* d_src, int64_t bytes);
int pf_memset(pf_handle* h, void* d_dst, int32_t byte, int64_t bytes);
/* counters of the most recent batch call */
int pf_get_counters(pf_handle* h, pf_counters* out);
/* timing of the most recent batch call's dominant kernel, measured with HIP
 * events on the handle's stream (ms) */
float pf_last_kernel_ms(pf_handle* h);

/* ---- K2: A* connector batch ---------------------------------------- */
/* Replaces AStarSolver.solve(start, target, nodes_to_avoid) (astar.py:33) or
 * MPA._a_star(start, end, nodes_to_avoid) (MPA.py:106) for n independent
 * queries.  Avoid sets are CSR (d_avoid_off int64[n+1], d_avoid_cells int32)
 * or NULL.  d_counters: int64[n*4] {pops, pushes, max_open, nbr_examined} or NULL. */
int pf_astar_batch(pf_handle* h, int32_t variant, int32_t allow_diag, int32_t restrict_corner, int32_t n,
                   const int32_t* d_start, const int32_t* d_target, const int64_t* d_avoid_off,
                   const int32_t* d_avoid_cells, int32_t path_cap, int32_t* d_cells, int32_t* d_len,
                   int32_t* d_status, int64_t* d_counters);

/* ---- K1: path scoring batch ---------------------------------------- */
/* Replaces BasePathfinder._calculate_stats_for_path (helper.py:138) /
 * MPA._calculate_path_stats (MPA.py:215).  d_stats: double[n*5] =
 * {length, turns, safety, diag, fitness}; empty path -> {inf,0,0,0,inf}. */
int pf_score_batch(pf_handle* h, const pf_score_params* sp, int32_t n, int32_t path_cap,
                   const int32_t* d_cells, const int32_t* d_len, double* d_stats);

/* ---- K3: chained waypoint decode (+ score) ------------------------- */
/* Replaces GASolver._reconstruct_path_from_chromosome (ga_solver.py:58) when
 * d_wp_cells != NULL (int32[n*W]) or PSOSolver._reconstruct_path_from_position
 * (pso.py:56; round-half-even + clamp) when d_wp_pos != NULL (double[n*W*2]),
 * followed by _calculate_stats_for_path when sp != NULL. */
int pf_decode_batch(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t n, int32_t W,
                    const int32_t* d_wp_cells, const double* d_wp_pos, int32_t start, int32_t target,
                    int32_t path_cap, int32_t* d_cells, int32_t* d_len, int32_t* d_status,
                    const pf_score_params* sp, double* d_stats);
/* pf_decode_batch with a start and a target cell PER AGENT (d_start, d_target: int32[n] in HBM, the convention of
 * pf_astar_batch): agent a decodes start d_start[a] -> its W waypoints -> d_target[a] exactly as pf_decode_batch(start =
 * d_start[a], target = d_target[a]) decodes it -- ga_solver.py:58-93 / pso.py:56-94 with self.start_node / self.target_node
 * taken per agent -- so decodes of different start / target pairs (K GA populations, pathfit.GABatch) share one launch, one
 * longest-first queue and one tail policy.  A cell outside the grid in d_start / d_target is an argument error (-1) found by
 * the planner before the decode is launched (one 4-byte read); a start or target ON an obstacle is legal and gives status 1. */
int pf_decode_batch_multi(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t n, int32_t W,
                          const int32_t* d_wp_cells, const double* d_wp_pos, const int32_t* d_start, const int32_t* d_target,
                          int32_t path_cap, int32_t* d_cells, int32_t* d_len, int32_t* d_status,
                          const pf_score_params* sp, double* d_stats);

/* ---- K6: PSO velocity/position update ------------------------------ */
/* Replaces the inner loop pso.py:183-203 for particles agent0..agent0+n with
 * the sweep-start gbest (synchronous PSO).  In place on
 * d_pos/d_vel (double[n*W*2]).  Stream (seed, DOM_PSO=3, iter, agent). */
int pf_pso_update(pf_handle* h, int32_t n, int32_t W, double w, double c1, double c2, double max_vel,
                  double* d_pos, double* d_vel, const double* d_pbest, const double* d_gbest, uint64_t seed,
                  uint64_t iter, uint64_t agent0);
/* The same update, asynchronous (stream ordered), leaving the pre-update position / velocity of every particle in
 * d_pos_keep / d_vel_keep: the roll-back copy of the asynchronous sweep (pso.py:222-229: a particle evaluated on a gbest that
 * an earlier particle of the sweep has moved must be evaluated again from its old state). */
int pf_pso_update_keep(pf_handle* h, int32_t n, int32_t W, double w, double c1, double c2, double max_vel,
                       double* d_pos, double* d_vel, const double* d_pbest, const double* d_gbest, uint64_t seed,
                       uint64_t iter, uint64_t agent0, double* d_pos_keep, double* d_vel_keep);
/* One round of the asynchronous sweep committed in one launch, for the evaluated batch [0, m): particles [0, n_final) are
 * final -- pso.py:216-220 (pbest position, fitness AND path row) --, `improver` (< n_final, or -1) is the round's first gbest
 * improver -- pso.py:222-229: its position -> d_gbest[W*2], its five stats -> d_gbest_stats[5], its path -> d_gbest_path
 * ([0] = length, then the cells) --, particles [n_final, m) roll back to d_pos_keep / d_vel_keep.  Asynchronous. */
int pf_pso_commit(pf_handle* h, int32_t m, int32_t W, int32_t path_cap, int32_t n_final, int32_t improver, double* d_pos,
                  double* d_vel, const double* d_pos_keep, const double* d_vel_keep, const double* d_stats, const int32_t* d_len,
                  const int32_t* d_cells, double* d_pbest, double* d_pbest_fit, int32_t* d_pb_cells, int32_t* d_pb_len,
                  double* d_gbest, double* d_gbest_stats, int32_t* d_gbest_path);

/* ---- K4/K5: MAACO --------------------------------------------------- */
/* Replaces MAACO.__init__ state (pheromone_matrix :58-84, dist table :86-91)
 * plus the per-cell eta'^beta tables derived from :197-210 (host libm, so
 * bit-identical to the reference's math.exp / pow). */
int pf_maaco_setup(pf_handle* h, const pf_maaco_params* p);
/* Replaces MAACO._construct_ant_solution_maaco (MAACO.py:278) for ants
 * ant0..ant0+n of iteration iter.  d_plen double[n] (inf if failed),
 * d_turns int32[n] (-1 if failed).  Stream (seed, DOM_MAACO=1, iter, ant). */
int pf_maaco_walk_batch(pf_handle* h, int32_t iter, uint64_t seed, int32_t ant0, int32_t n, int32_t path_cap,
                        int32_t* d_cells, int32_t* d_len, double* d_plen, int32_t* d_turns, int32_t* d_status);
/* Replaces MAACO._update_pheromone_trails_maaco (MAACO.py:304) in three
 * ordered steps so that a population sharded over GPUs can fold its deposits
 * in global ant order: evaporate (:305), deposit (:306-311, sequential in ant
 * order per cell -- bit-exact, no float atomics), clip (:312-332). */
int pf_maaco_evaporate(pf_handle* h);
int pf_maaco_deposit(pf_handle* h, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len,
                     const double* d_plen);
int pf_maaco_clip(pf_handle* h, double best_len_overall);
/* The same update (MAACO.py:304-332) in ONE pass over tau for the paths of one batch on one GPU: per cell evaporate (:305),
 * the deposits in ant order (:306-311), clip (:312-332) -- the same fp64 operations in the same order as the three calls
 * above.  Successful ants mark their own deposits at the end of their walk (option "maaco_mark_in_walk", default 1), so
 * the update of the batch that was just walked needs no pass over the paths. */
int pf_maaco_update(pf_handle* h, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, const double* d_plen,
                    double best_len_overall);
/* One whole iteration of MAACO.solve_path_planning (MAACO.py:340-359) for the ants of one GPU, enqueued back to back: walks,
 * best-of-iteration scan (:343-349), take-over test against the caller's overall best (:351-358), one-pass pheromone update.
 * The overall best ant's path row stays in HBM (pf_maaco_best_path reads it on demand).
 * ONE 104-byte block comes back: out13 = {ib_len, ib_turns, ib_idx, took, best_len, best_turns, tmin, tmax, skipped, steps,
 * candidates, path_cells, overflow_agents}.  overflow_agents > 0: the pheromone was left untouched (skipped = 1); repeat
 * the call with longer path rows.  The call returns once the take-over test is known (the device mirrors out13 into pinned
 * host memory; no copy is enqueued); the pheromone update may still be running -- every later pf_ call on this handle is
 * ordered after it on the handle's stream, pf_sync waits for it. */
int pf_maaco_iterate(pf_handle* h, int32_t iter, uint64_t seed, int32_t ant0, int32_t n, int32_t path_cap,
                     int32_t* d_cells, int32_t* d_len, double* d_plen, int32_t* d_turns, int32_t* d_status,
                     double best_len, double best_turns, double* out13);
/* MAACO.best_path_overall (MAACO.py:351-358), kept in HBM by pf_maaco_iterate: whenever an iteration's best ant takes over, its
 * path row is copied on the device.  This call materialises it: *len_out cells into cells_out[cap] (0: no ant has arrived yet). */
int pf_maaco_best_path(pf_handle* h, int32_t* cells_out, int32_t cap, int32_t* len_out);
/* pheromone_matrix attribute round trip (double[R*C]) */
int pf_maaco_get_pheromone(pf_handle* h, double* tau);
int pf_maaco_set_pheromone(pf_handle* h, const double* tau);
void* pf_maaco_tau_dev(pf_handle* h); /* device pointer, for collectives */
/* sequential best-of-iteration scan MAACO.py:343-349 over host arrays;
 * inout: best_len/best_turns/best_idx (idx -1 = none yet) */
int pf_maaco_best_scan(int32_t n, const double* plen, const int32_t* turns, int32_t idx0, double* best_len,
                       double* best_turns, int32_t* best_idx);

/* ---- K4/K5 batched: K independent MAACO colonies in one iteration -------- */
/* K colonies share the handle's grid and one parameter set (p->start / p->target are ignored); colony c has its own start
 * starts[c], target targets[c], seed seeds[c] and n ants, and its own pheromone, eta table (shared between colonies with the
 * same start / target), deposit matrix and overall best path -- owned by the batch, so the handle's solo MAACO state
 * (pf_maaco_setup) is never touched, and several batches may live on one handle.  The tabu slot pool is the handle's.
 * Colony c computes exactly what a solo run (pf_maaco_setup with start / target = starts[c] / targets[c], pf_maaco_iterate
 * with seed seeds[c], ant0 0, n ants) computes: ant a of colony c draws the stream (seeds[c], DOM_MAACO, iter, a).
 * The device memory is checked at creation (tau, tau^alpha when alpha != 1, tep, ceil(n / 64) RC bit words, flags, deposits
 * and a best row per colony: ~1.3 MB at 128^2 x 256 ants): a batch that does not fit fails with a message.  pf_destroy
 * frees every batch of the handle; after pf_update_grid a batch only accepts pf_maaco_batch_destroy. */
typedef struct pf_maaco_batch pf_maaco_batch;
int pf_maaco_batch_create(pf_handle* h, const pf_maaco_params* p, int32_t K, int32_t n, const int32_t* starts, const int32_t* targets,
                          const uint64_t* seeds, pf_maaco_batch** out);
void pf_maaco_batch_destroy(pf_maaco_batch* b);
/* One iteration of every colony, as pf_maaco_iterate: one walk over the K n ants (colony c's ants are rows [c n, (c + 1) n) of
 * d_cells [K n][path_cap] and of the other columns), one best-of-iteration / take-over launch (a block per colony, against
 * best_len[c] / best_turns[c]), one pheromone pass, ONE wait.  out[13 c ...] = colony c's 13 doubles (pf_maaco_iterate's out13;
 * steps ... overflow_agents count the whole batch).  overflow_agents > 0 anywhere: no colony's pheromone moved; repeat the
 * call with longer rows. */
int pf_maaco_batch_iterate(pf_maaco_batch* b, int32_t iter, int32_t n, int32_t path_cap, int32_t* d_cells, int32_t* d_len,
                           double* d_plen, int32_t* d_turns, int32_t* d_status, const double* best_len, const double* best_turns,
                           double* out);
/* colony k's overall best path (pf_maaco_best_path), and its pheromone matrix round trip (double[R*C]) */
int pf_maaco_batch_best_path(pf_maaco_batch* b, int32_t k, int32_t* cells_out, int32_t cap, int32_t* len_out);
int pf_maaco_batch_get_pheromone(pf_maaco_batch* b, int32_t k, double* tau);
int pf_maaco_batch_set_pheromone(pf_maaco_batch* b, int32_t k, const double* tau);

/* ---- GA host operators (native, no device work) ------------------------ */
/* GASolver._selection, ga_solver.py:136-142: one generation of tournaments on the stream (seed, DOM_GA_SELECT, gen, 0):
 * random.sample(population, min(tournament_size, n)) then the first minimum of fitness.  parent_idx[n] = indices into
 * the (sorted) population. */
int pf_ga_select(uint64_t seed, int32_t gen, int32_t n, int32_t tournament_size, const double* fitness, int32_t* parent_idx);
/* GASolver._create_chromosome, ga_solver.py:55-56 (+48-53), for attempts attempt0 .. attempt0+n-1 of the population
 * initialisation (:95-133): attempt k draws W free cells from the stream (seed, DOM_INIT, 0, k).  cells[n][W]. */
int pf_ga_random_chromosomes(uint64_t seed, int32_t attempt0, int32_t n, int32_t W, const uint8_t* occ, int32_t R, int32_t C,
                             int32_t* cells);
/* GASolver._crossover + _mutate + _generate_random_waypoint for all children of a generation, ga_solver.py:144-160,
 * 186-194, 48-53: pair j (parents 2j, 2j+1 mod n of parent_cells[n][W], cells r*C+c) draws from (seed, DOM_GA, gen, j).
 * occ = host occupancy, 1 = obstacle.  child_cells[n][W]. */
int pf_ga_breed(uint64_t seed, int32_t gen, int32_t n, int32_t W, double crossover_rate, double mutation_rate,
                const uint8_t* occ, int32_t R, int32_t C, const int32_t* parent_cells, int32_t* child_cells);

/* ---- K7 + K2b + K1: MPA --------------------------------------------- */
int pf_mpa_setup(pf_handle* h, const pf_mpa_params* p, const pf_score_params* sp);
/* One phase sweep MPA.py:339-377 over n local predators.  d_gidx[a] = index
 * of predator a in the GLOBAL fitness-sorted population of this iteration (the
 * reference's loop index: it keys the stream (seed, DOM_MPA=2, iter, gidx) and
 * decides the phase-2 Levy/Brownian split, MPA.py:351); d_slot[a] = its
 * storage slot in the strided population d_pop_*.  The kernel draws the start
 * idx + gate, then runs MPA._reconstruct_path_segment (:284-318) or the
 * phase's no-move branch.  d_elite_cells/elite_len/d_elite_stats(double[5]) =
 * the sweep-start elite (may alias the population storage: candidates go to
 * separate buffers).  phase in {1,2,3}; CF per MPA.py:336.
 * Outputs candidate paths (strided, same cap) + stats double[n*5]. */
int pf_mpa_phase_batch(pf_handle* h, int32_t phase, double CF, int32_t iter, uint64_t seed, int32_t n,
                       int32_t path_cap, const int32_t* d_pop_cells, const int32_t* d_pop_len,
                       const double* d_pop_stats, const int32_t* d_gidx, const int32_t* d_slot,
                       const int32_t* d_elite_cells, int32_t elite_len, const double* d_elite_stats,
                       int32_t* d_out_cells, int32_t* d_out_len, double* d_out_stats, int32_t* d_status);
/* FADs sweep MPA.py:387-410 on the post-memory population (in place):
 * stream (seed, DOM_MPA_FADS=5, iter, gidx). */
int pf_mpa_fads_batch(pf_handle* h, double CF, int32_t iter, uint64_t seed, int32_t n, int32_t path_cap,
                      const int32_t* d_gidx, const int32_t* d_slot, int32_t* d_pop_cells, int32_t* d_pop_len,
                      double* d_pop_stats, int32_t* d_status);
/* One whole MPA iteration's device work in a single longest-first work queue: the phase sweep (as
 * pf_mpa_phase_batch, candidates -> d_c1_*) and the FADs candidates (MPA.py:387-410; they depend only on the
 * predator's stream and the grid, so they are produced concurrently -> d_c2_*, d_c2_len 0 = none), then the
 * memory step (:381-384) and the FADs acceptance (:402/:408) in place on the population.  Equivalent to
 * pf_mpa_phase_batch + pf_mpa_memory + pf_mpa_fads_batch, with one tail instead of two.  An agent whose
 * scratch overflowed is reported through pf_get_counters().overflow_agents and d_status (phase items). */
int pf_mpa_iter_batch(pf_handle* h, int32_t phase, double CF, int32_t iter, uint64_t seed, int32_t n, int32_t path_cap,
                      int32_t* d_pop_cells, int32_t* d_pop_len, double* d_pop_stats, const int32_t* d_gidx,
                      const int32_t* d_slot, const int32_t* d_elite_cells, int32_t elite_len, const double* d_elite_stats,
                      int32_t* d_c1_cells, int32_t* d_c1_len, double* d_c1_stats, int32_t* d_c2_cells, int32_t* d_c2_len,
                      double* d_c2_stats, int32_t* d_status);
/* Exact look-ahead for the fused sweep.  An iteration that accepts no candidate leaves the population, the
 * list order and the elite untouched, so the next iteration's sweep can run in the same work queue.
 * pf_mpa_iter_ahead: iterations iters[0 .. depth) (1 <= depth <= 16; phases[d], CFs[d] are level d's) of the population as
 *   ONE sweep of 2 * depth * n items.  depth == 1 is pf_mpa_iter_batch whose apply also counts.  With depth > 1 the candidate
 *   rows of all levels live in buffers the handle owns (allocated on first use, freed by pf_destroy; the d_c1 / d_c2 / d_status
 *   arguments are then not written); level 0 is applied, the others wait.  *accepted = predators level 0 changed.
 *   pf_get_counters() after a merged sweep: the search counters of the whole sweep, overflow_agents of level 0 alone.
 * pf_mpa_ahead_take: the device work of iteration `iter` from the waiting levels, if the level is still that iteration's (all
 *   levels before it accepted nothing, none overflowed, same buffers, no other MPA call or pf_update_grid since): its
 *   candidates are applied -- no search runs -- and *accepted = predators changed; pf_get_counters() then reads zero.
 *   Otherwise *accepted = -1, the waiting levels are dropped, and the caller sweeps the iteration itself.
 * pf_mpa_ahead_level_bufs: where the candidate rows of the level applied last are: out7 = {c1 cells, c1 len, c1 stats,
 *   c2 cells, c2 len, c2 stats, status}, all null after a single-level sweep (the caller's own rows).
 * pf_mpa_ahead_drop: forget the waiting levels (the caller changes the population by other means).
 * pf_mpa_ahead_stats: out6 = {option "mpa_lookahead", option "mpa_lookahead_always", merged sweeps, levels swept ahead,
 *   iterations served from a level, times a waiting level was found stale}. */
int pf_mpa_iter_ahead(pf_handle* h, int32_t depth, const int32_t* phases, const double* CFs, const int32_t* iters, uint64_t seed, int32_t n,
                      int32_t path_cap, int32_t* d_pop_cells, int32_t* d_pop_len, double* d_pop_stats, const int32_t* d_gidx,
                      const int32_t* d_slot, const int32_t* d_elite_cells, int32_t elite_len, const double* d_elite_stats,
                      int32_t* d_c1_cells, int32_t* d_c1_len, double* d_c1_stats, int32_t* d_c2_cells, int32_t* d_c2_len,
                      double* d_c2_stats, int32_t* d_status, int32_t* accepted);
int pf_mpa_ahead_take(pf_handle* h, int32_t iter, const int32_t* d_slot, int32_t* d_pop_cells, int32_t* d_pop_len, double* d_pop_stats,
                      int32_t* accepted);
int pf_mpa_ahead_level_bufs(pf_handle* h, void** out7);
int pf_mpa_ahead_drop(pf_handle* h);
int pf_mpa_ahead_stats(pf_handle* h, int64_t* out6);
/* MPA._reconstruct_path_segment (MPA.py:284-318) called directly: predator a
 * modifies population path a against the given elite path with explicit
 * idx / is_levy / scale and stream (seed, DOM_MPA, iter, d_agent[a]). */
int pf_mpa_rebuild_batch(pf_handle* h, int32_t iter, uint64_t seed, int32_t n, int32_t path_cap,
                         const int32_t* d_pop_cells, const int32_t* d_pop_len, const double* d_pop_stats,
                         const int32_t* d_elite_cells, int32_t elite_len, const int32_t* d_idx,
                         const int32_t* d_is_levy, const double* d_scale, const int32_t* d_agent,
                         int32_t* d_out_cells, int32_t* d_out_len, double* d_out_stats, int32_t* d_status);
/* memory step MPA.py:381-384: pop[d_slot[a]] <- cand[a] where cand fitness < pop fitness */
int pf_mpa_memory(pf_handle* h, int32_t n, int32_t path_cap, const int32_t* d_slot, const int32_t* d_cand_cells,
                  const int32_t* d_cand_len, const double* d_cand_stats, int32_t* d_pop_cells, int32_t* d_pop_len,
                  double* d_pop_stats);

/* ---- K7 batched: K independent MPA schools in one sweep ------------------- */
/* A school is one MPA population with its own seed seeds[k], start starts[k] and target targets[k]; the K schools share the
 * handle's grid, p->num_predators (N), the hyper-parameters and the score parameters (p->start / p->target are ignored).
 * School k computes exactly what a solo run computes (pf_mpa_setup with start / target = starts[k] / targets[k], then
 * pf_sort_order_by_key / pf_mpa_pick_elite / pf_mpa_iter_batch with seed seeds[k]): predator i of its fitness-sorted list
 * draws the streams (seeds[k], DOM_MPA=2, iter, i) and (seeds[k], DOM_MPA_FADS=5, iter, i), and the phase-2 split
 * (MPA.py:351) is i < N / 2 within the school.
 * Layout of every buffer the calls below take: school k's predators are rows [k N, (k + 1) N); d_order [K N] holds, per
 * school, the list (position -> LOCAL slot 0 .. N - 1).
 * pf_mpa_batch_create replaces K times MPA.__init__'s device work: the K MPA._generate_initial_path() searches
 * (_a_star(start, target), MPA.py:154; memoised for the FADs re-init branch :405) run as ONE pf_astar_batch of K and are
 * scored by one pf_score_batch; the pruning bound tables (one host Dijkstra per DISTINCT start or target cell) are built as
 * pf_mpa_setup builds them.  A school whose target is unreachable has initial length 0 (the caller seeds the reference's
 * fallback population [start, target], MPA.py:235-236; the re-init branch then never fires, as in the solo run).
 * The batch owns its school table, bound tables, initial paths, elites and sort scratch: the handle's solo MPA state
 * (pf_mpa_setup, pf_mpa_elite_buf) is never touched and several batches may live on one handle; the search slots, the work
 * queue and the per-call job / proposal scratch are the handle's.  Device memory (~8 RC bytes per school + 8 RC per distinct
 * cell) is checked at creation.  pf_destroy frees every batch of the handle; after pf_update_grid a batch only accepts
 * pf_mpa_batch_destroy (every other call fails with a message). */
typedef struct pf_mpa_batch pf_mpa_batch;
int pf_mpa_batch_create(pf_handle* h, const pf_mpa_params* p, const pf_score_params* sp, int32_t K, const int32_t* starts,
                        const int32_t* targets, const uint64_t* seeds, pf_mpa_batch** out);
void pf_mpa_batch_destroy(pf_mpa_batch* b);
/* school k's memoised initial path (host copy; *len_out = 0: unreachable) and its 5 stats (may be null) */
int pf_mpa_batch_init_path(pf_mpa_batch* b, int32_t k, int32_t* cells_out, int32_t cap, int32_t* len_out, double* stats5);
/* what pf_mpa_batch_create spent, in ms of host wall time: {initial searches + scores, bound tables, whole call} */
int pf_mpa_batch_create_ms(pf_mpa_batch* b, double* out3);
/* list.sort(key=fitness) of every school (MPA.py:321,333,412): K stable rank sorts of N keys (d_pop_stats[row * 5 + 4]) in one
 * launch sequence, each inside its own segment of d_order */
int pf_mpa_batch_sort(pf_mpa_batch* b, const double* d_pop_stats, int32_t* d_order);
/* elite = population[0].copy() of every school (MPA.py:334) into the batch's elite buffers: one block per school */
int pf_mpa_batch_pick_elite(pf_mpa_batch* b, int32_t path_cap, const int32_t* d_pop_cells, const int32_t* d_pop_len,
                            const double* d_pop_stats, const int32_t* d_order);
/* MPA.py:339-410 for all K schools, as pf_mpa_iter_batch does it for one: the phase items and the FADs candidates of the
 * K N predators share ONE longest-first work queue of 2 K N items, searched by the same kernel as the solo sweep; memory
 * step and FADs acceptance follow.  Doubtful proposals are confirmed on the host against their own school's elite and seed.
 * An item whose path does not fit path_cap is counted (pf_mpa_batch_counters: overflow_agents) and never truncated. */
int pf_mpa_batch_iterate(pf_mpa_batch* b, int32_t phase, double CF, int32_t iter, int32_t path_cap, int32_t* d_pop_cells,
                         int32_t* d_pop_len, double* d_pop_stats, const int32_t* d_order, int32_t* d_c1_cells, int32_t* d_c1_len,
                         double* d_c1_stats, int32_t* d_c2_cells, int32_t* d_c2_len, double* d_c2_stats, int32_t* d_status);
/* population[0] of every school after the sort (MPA.py:413) in one copy: out[6 k ...] = {local slot, length, turns, safety,
 * diag, fitness}; the 4-level tie-break MPA.py:415-437 stays with the caller */
int pf_mpa_batch_best_rows(pf_mpa_batch* b, const double* d_pop_stats, const int32_t* d_order, double* out);
/* the path in local slot `slot` of school k (the caller reads it when that school's best improves, MPA.py:417) */
int pf_mpa_batch_read_path(pf_mpa_batch* b, int32_t k, int32_t slot, int32_t path_cap, const int32_t* d_pop_cells,
                           const int32_t* d_pop_len, int32_t* cells_out, int32_t cap, int32_t* len_out);
/* counters of the batch's last sweep, and over its lifetime: items that overflowed, proposals the host's libm resolved */
int pf_mpa_batch_counters(pf_mpa_batch* b, pf_counters* out, int64_t* overflow_total, int64_t* doubts_resolved);

/* ---- distance fields: exact one-to-all path lengths from K sources (pathfit.DistanceField) ----------------------------
 * Exact shortest-path lengths from K source cells to every cell (one-to-all Dijkstra, dijkstra.py's relaxation with no target):
 * d_out[k*RC + v] = the least fixed point of D[src[k]] = 0, D[v] = min over legal moves u -> v of fl(D[u] + w) (w = 1 for the
 * four straight moves, sqrt(2) for the diagonals, the call's move policy) -- bit for bit what a heap Dijkstra leaves; +inf for
 * obstacles and unreachable cells; a source ON an obstacle gives an all-inf row (legal); a source outside the grid, K < 1 or a
 * null pointer is an argument error (-1) found on the host before anything is launched.  src is a HOST array.  d_info: int64[K*4]
 * {levels that held at least one live cell, cells with a finite label, relaxations offered, list appends} or NULL.
 * One workgroup per source, min(K, CUs) of them; their level lists (12 RC bytes per workgroup) are the
 * handle's, allocated on first use.  Time grows with the number of levels, floor(largest length) + 1: a corridor map with
 * paths of ~RC / 2 steps serialises.  Synchronous, ordered on the handle's stream; pf_last_kernel_ms reports the kernel. */
int pf_dist_field_batch(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t K, const int32_t* src,
                        double* d_out, int64_t* d_info);

/* ---- routing trees: DijkstraSolver's paths to many targets from one field (pathfit.DistanceField.paths) ----------------
 * pf_dist_field_parents: d_parents[k*RC + v] (uint8) = the last step of DijkstraSolver.solve()'s path from source k into v, from
 * the K fields d_fields [K][RC] that pf_dist_field_batch left under the SAME move policy: 0..7 the move index (helper.py:30-36
 * order) with v = parent + move, 8 at the source (D == 0), 255 for an obstacle or a cell out of reach (D == +inf).  The parent is
 * the u with the smallest (D[u], u) among the cells with a legal move u -> v and fl(D[u] + w) == D[v]: dijkstra.py:59-96 pops
 * in (g, (r, c)) order, every weight is >= 1, so that is its pop order, and came_from (:84) keeps the earliest-popped cell that
 * offers the final label -- the traced paths are the reference's cell for cell, not merely as short.  Fields that
 * are no fixed point of the handle's grid under the policy (a finite non-source cell without such a u) fail the call with a message;
 * every byte is written all the same.  K < 1 or a null pointer is an argument error (-1) found before anything is launched.
 * pf_dist_field_paths: n queries (d_field_idx[q], d_target[q]) -> row q of d_cells [n][path_cap], d_len, d_status, laid out as
 * pf_astar_batch's rows (pf_score_batch scores them unchanged): the path source -> target (reverse = 0, solve()'s order) or
 * target -> source (reverse != 0, the order an agent walks to the goal); target == source is the one-cell path (dijkstra.py:40-41).
 * PF_ST_INFEASIBLE, length 0: the target's code is 255, the target id lies outside [0, RC) or the field index outside [0, K)
 * (nothing is read or written out of range).  PF_ST_OVERFLOW, length 0, row untouched: more than path_cap cells -- or a map that
 * is no tree (a code other than 0..8 on the way, a step off the grid, more than RC cells): the walk is bounded whatever the
 * bytes hold.  d_field_idx NULL: each query takes the field with the smallest d_fields[k][target], the lowest k on a tie (the
 * nearest source; d_fields is needed only then); d_chosen (or NULL) takes the field each query used, -1 where the target id or
 * the field index was out of range.  K < 1, n < 0, path_cap < 1 or a missing pointer is an argument error (-1) found before any
 * launch; n == 0 returns 0 and launches nothing.  One lane per query, a step is one dependent byte load.
 * Both calls are synchronous and ordered on the handle's stream; pf_last_kernel_ms reports the kernel. */
int pf_dist_field_parents(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t K, const double* d_fields,
                          uint8_t* d_parents);
int pf_dist_field_paths(pf_handle* h, int32_t K, const uint8_t* d_parents, const double* d_fields, int32_t n,
                        const int32_t* d_field_idx, const int32_t* d_target, int32_t reverse, int32_t path_cap, int32_t* d_cells,
                        int32_t* d_len, int32_t* d_status, int32_t* d_chosen);

/* ---- nearest-source fields: one field per source SET, and the source that owns each cell (pathfit.NearestSourceField) ------
 * B sets in CSR form, both HOST arrays: set b is src[set_off[b] .. set_off[b + 1]), flat cell ids.
 * pf_dist_field_merged: d_out[b*RC + v] = the length of the shortest path into v from the NEAREST source of set b: the least
 * fixed point of D[s] = 0 for every free s of the set, D[v] = min fl(D[u] + w) otherwise -- bit for bit the elementwise minimum
 * of pf_dist_field_batch's rows for the set's sources, in 8 RC bytes whatever the size of the set and in
 * floor(largest distance to the nearest source) + 1 levels.  A source on an obstacle is skipped, a source listed twice counts
 * once, a set whose sources all lie on obstacles gives an all-inf row.  d_info as pf_dist_field_batch's (the seeds count as cells
 * reached and as appends) or NULL.  One workgroup per set, min(B, CUs) of them, on the same list slots.
 * pf_dist_field_owners: d_owner[b*RC + v] = the index WITHIN set b of the source at the root of v's chain through d_parents,
 * the parent maps pf_dist_field_parents computed from the merged rows (several cells of code 8 each); the lowest index where a
 * cell is listed more than once; -1 where the code is 255.  This is the tree a dijkstra.py-shaped search seeded with the whole
 * set leaves (the smallest (D[u], u) parent at every step), NOT the lowest index among the sources at the same distance;
 * pf_dist_field_paths with field index b traces the same chain.  d_count (or NULL): int64[set_off[B]], the cells each source
 * owns (integer atomics: exact).  The roots are found by pointer doubling, one launch per round, ceil(log2(n)) rounds, n the
 * bound on the cells of a chain: RC, or the largest "levels that held a live cell" of d_info, the [B][4] block the field call
 * wrote (or NULL).  A code outside 0..8 and 255, a step off the grid, a root that is no source of its set or a chain longer than
 * the bound fails the call with a message; every word of d_owner is written all the same, nothing is accessed out of range.
 * Both: B < 1, offsets that do not start at 0 or that decrease, an empty set, an id outside [0, RC) or a null pointer is an
 * argument error (-1) whose message names the set and the index, found on the host before anything is launched.  Synchronous,
 * ordered on the handle's stream; pf_last_kernel_ms reports the kernel(s). */
int pf_dist_field_merged(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t B, const int32_t* set_off,
                         const int32_t* src, double* d_out, int64_t* d_info);
int pf_dist_field_owners(pf_handle* h, int32_t B, const uint8_t* d_parents, const int32_t* set_off, const int32_t* src,
                         const int64_t* d_info, int32_t* d_owner, int64_t* d_count);

/* ---- any-angle smoothing: line of sight between cell centres, forward string pulling (pathfit.PathSmoother) ------------
 * The rule is exact integer geometry.  For a = (r0, c0), b = (r1, c1), dr = r1 - r0, dc = c1 - c0,
 * s = |dr| + |dc| and a cell (r, c) of the bounding box, k = dr (c - c0) - dc (r - r0): the segment between the centres CROSSES
 * the cell's open square iff |2k| < s and TOUCHES it in a corner point only iff |2k| == s.  a sees b iff no crossed cell is an
 * obstacle and, with restrict_corner != 0, no touched one either (on a single diagonal step: the corner-cut rule of the move
 * policies); a == b is visible iff the cell is free.  Both calls read the handle's occupancy at call time.
 * pf_line_of_sight_batch: n pairs of cell ids -> d_visible[i] = 0 / 1 and, when d_first_block != NULL, the blocking cell of the
 * major index (columns if |dc| >= |dr|, else rows) nearest d_from[i], the smallest r C + c among that index's blocking cells;
 * -1 when visible.  An endpoint outside the grid gives visible = 0, first_block = -1.  One wavefront per pair.
 * pf_smooth_batch: n path rows laid out as pf_astar_batch's (d_cells[i * path_cap ..], d_len[i]) -> the waypoints the forward
 * rule keeps: out = [0]; a = 0; j = 1; while j + 1 < L: visible(p[a], p[j + 1]) ? j += 1 : (out += [j], a = j, j = a + 1);
 * out += [L - 1].  Consecutive input cells are never tested; the input need not be a legal path.  d_way_cells [n * way_cap] the
 * cells, d_way_idx (or NULL) their positions in the input row, d_way_len their number, d_stats (or NULL) [n * 2] = {the sum of
 * the segments' Euclidean lengths left to right, the interior waypoints whose two segments are not parallel and equally
 * directed}, both 0 unless the status is 0.  d_status: 0 ok; 1 = an empty row, a length beyond path_cap or a cell outside [0, R C): length 0, the waypoint row
 * untouched; 3 = more waypoints than way_cap: length 0, the row's contents unspecified.  One wavefront per path.
 * Both: n < 0, a cap < 1 or a missing required pointer is an argument error (-1) found before any launch; n == 0 returns 0 and
 * launches nothing.  Synchronous, ordered on the handle's stream; pf_last_kernel_ms reports the kernel. */
int pf_line_of_sight_batch(pf_handle* h, int32_t restrict_corner, int32_t n, const int32_t* d_from, const int32_t* d_to,
                           int32_t* d_visible, int32_t* d_first_block);
int pf_smooth_batch(pf_handle* h, int32_t restrict_corner, int32_t n, int32_t path_cap, const int32_t* d_cells,
                    const int32_t* d_len, int32_t way_cap, int32_t* d_way_cells, int32_t* d_way_idx, int32_t* d_way_len,
                    double* d_stats, int32_t* d_status);

/* ---- connected components: labels, sizes, reachability queries (pathfit.Components) ----------------------------------------
 * Cells are r C + c.  A cell is free iff its grid value is not 1; two free cells are adjacent iff the handle's move mask of the
 * call's policy allows the move (the byte pf_astar_batch and pf_dist_field_batch use; symmetric under all four policies).  The
 * masks are read at call time: after pf_update_grid the next call labels the new map.
 * pf_components: d_labels[v] = -1 on an obstacle, else the rank of v's component when the components are ordered by their
 * smallest cell id (the numbering the searches' own labels use).  d_info (or NULL): {count, free cells, the size of the largest
 * component, its label}, the lowest label on a tie, -1 for the last field when count == 0.  Union-find rooted at the smallest
 * cell id, linked with agent-scope atomics, then flattened, ranked by an exclusive scan of the root flags in cell order and
 * counted with integer atomics: work and launches do not grow with a component's diameter and the result does not depend on the
 * order the links land in.  The handle keeps about three int32 words per cell of scratch from the first call on.
 * pf_component_sizes: d_sizes[l] (or NULL) = the cells labelled l and d_first[l] (or NULL) = the smallest of them (strictly
 * increasing in l for pf_components' labels; -1 for a label no cell carries), for l in [0, count); labels outside [0, count) are
 * ignored.  pf_components_same: d_same[i] = 1 iff d_a[i] and d_b[i] both lie in [0, RC), both labels are >= 0 and they are equal
 * (a free cell is connected to itself), else 0; nothing is read out of range.
 * A null handle (-2), a missing required pointer, n < 0 or count < 0 (-1, with a message) is an argument error found before any
 * launch; n == 0 or count == 0 returns 0 and launches nothing.  All three are synchronous and ordered on the handle's stream;
 * pf_last_kernel_ms reports the kernels.  pf_components_phase_ms: the HIP-event spans of the last pf_components call made under
 * pf_set_option "components_phases" = 1 -- {init + link, flatten, rank, labels, sizes + info} ms; zeros otherwise. */
int pf_components(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t* d_labels, int64_t* d_info);
int pf_component_sizes(pf_handle* h, const int32_t* d_labels, int32_t count, int64_t* d_sizes, int32_t* d_first);
int pf_components_same(pf_handle* h, const int32_t* d_labels, int32_t n, const int32_t* d_a, const int32_t* d_b,
                       int32_t* d_same);
int pf_components_phase_ms(pf_handle* h, float* ms);

/* ---- clearance fields: exact obstacle distances, the margins of path rows and segments (pathfit.Clearance) -----------------
 * Cells are r C + c; an obstacle is a cell of grid value 1.  Everything is integer and exact.  The occupancy is
 * read at call time: after pf_update_grid the next pf_clearance_field sees the new map.
 * pf_clearance_field: d_d2[v] = the squared Euclidean distance between cell centres from v to the nearest obstacle cell, 0 on an
 * obstacle.  border != 0: the cells just outside the grid count as obstacles too, so min(r + 1, R - r, c + 1, C - c)^2 takes part
 * in the minimum; border == 0 (the reference's rule, helper.py:67-80) on a map without an obstacle: every word is PF_CLEAR_NONE.
 * d_near (or NULL): the nearest obstacle cell INSIDE the grid, the smallest r C + c among the nearest ones, an obstacle's own id
 * on an obstacle, -1 everywhere on a map without an obstacle.  d_near ignores `border`: the border changes d_d2 only.
 * d_info (or NULL): {obstacle cells, free cells, the largest d2 over the free cells, the smallest cell id that attains it}, the
 * last two -1 when no cell is free.  A separable transform: a row pass over wave-wide obstacle masks, then a column pass that
 * scans outwards while the row distance can still win and hands the columns it could not close within about 2^18 / C rows to
 * an exact integer lower-envelope pass, so the work does not grow with the clearance.  The handle keeps about three int32 words per cell
 * of scratch from the first call on (freed by pf_destroy).  R^2 + C^2 >= 2^31 - 1 is an argument error.
 * pf_clearance_paths: n path rows laid out as pf_astar_batch's against a field in HBM -> d_out[i * 4 ..] = {the smallest d2 over
 * the row's cells, the position of the first cell that attains it, the number of cells with d2 < margin_d2, the position of the
 * first such cell or -1}; d_profile (or NULL) [n * path_cap]: d2 per cell, words beyond d_len[i] untouched.  d_status: 0 ok;
 * 1 = an empty row, a length beyond path_cap or a cell outside [0, R C): d_out = {PF_CLEAR_NONE, -1, 0, -1}, the profile row
 * untouched, nothing read out of range.  One wavefront per row.
 * pf_clearance_segments: n pairs of cell ids -> d_min[i] = the smallest d2 over the cells the straight segment between the two
 * centres crosses (the rule of the smoothing section: |2k| < s), with touched != 0 also over the cells it only touches in a
 * corner (|2k| == s); d_at (or NULL): the cell of smallest id that attains it.  An endpoint outside the grid gives
 * PF_CLEAR_NONE and -1; a == b gives that cell's own d2.  One wavefront per pair.
 * A null handle (-2); a missing required pointer, n < 0, path_cap < 1 or margin_d2 < 0 (-1, with a message) is an argument error
 * found before any launch; n == 0 returns 0 and launches nothing.  All three are synchronous and ordered on the handle's stream;
 * pf_last_kernel_ms reports the kernels. */
#define PF_CLEAR_NONE 0x7FFFFFFF
int pf_clearance_field(pf_handle* h, int32_t border, int32_t* d_d2, int32_t* d_near, int64_t* d_info);
int pf_clearance_paths(pf_handle* h, const int32_t* d_d2, int32_t n, int32_t path_cap, const int32_t* d_cells,
                       const int32_t* d_len, int32_t margin_d2, int32_t* d_out, int32_t* d_profile, int32_t* d_status);
int pf_clearance_segments(pf_handle* h, const int32_t* d_d2, int32_t touched, int32_t n, const int32_t* d_from,
                          const int32_t* d_to, int32_t* d_min, int32_t* d_at);

/* ---- widest-path fields over a clearance field: the largest robot that fits, and where (pathfit.Clearance.widest) ------------
 * d_d2: an int32 [R C] field in HBM, what pf_clearance_field left there (either `border`); any non-negative array is defined,
 * the caller vouches that it belongs to the map.  The call reads d_d2 only, never the handle's occupancy.  The B source sets
 * are pf_dist_field_merged's host CSR arrays: set b = src[set_off[b] .. set_off[b + 1]).
 * The capacity of a move u -> v is min(d2[u], d2[v]); a diagonal under restrict_corner != 0 also takes the two side cells' d2
 * into the minimum, and does not exist with allow_diag == 0.  d_out[b * R C + v] = w[b][v] = the largest, over all walks from
 * a source of set b to v, of the smallest capacity on the walk; d2[s] on a source s with d2[s] >= 1; 0 where no source reaches
 * with capacity >= 1 (every cell with d2 == 0).  Equivalently, for every t >= 1: w[b][v] >= t iff v and a source of set b lie
 * in one component, under the same policy, of the map whose obstacles are the cells with d2 < t.  A source with d2 == 0 is
 * skipped, one listed twice counts once, a set without a usable source gives an all-zero row.
 * d_info (or NULL) int64 [B][4]: {the sources that counted, the cells with w >= 1, the smallest w >= 1, the smallest cell id
 * that attains it}, the last two -1 when nothing is reached.
 * Tiles of 64 x 16 cells are relaxed to their own fixed point in LDS, one launch per round over the queued tiles of all B sets;
 * the rounds grow with the tiles a widest route crosses (at most 1 + its tile-border crossings), not with its cells, and the
 * host reads one 4-byte queue length per round.  The result is the least fixed point, identical run to run.
 * The handle keeps four int32 words per (set, tile) plus the sets as scratch from the first call on (grown on demand, freed by
 * pf_destroy).  A null handle (-2); B < 1, offsets that do not start at 0 or fall, an empty set, an id outside the grid or a
 * null pointer (-1, with a message that names the set and the index) is an argument error found before any launch.
 * Synchronous and ordered on the handle's stream; pf_last_kernel_ms reports the span of the kernels.
 * pf_clearance_widest_work (host side): out4 = {launches of the tile kernel, tile visits, words raised, 0} of the last call.
 * These depend on the schedule (which halo words a tile happened to see): figures for a probe, never part of the result. */
int pf_clearance_widest(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const int32_t* d_d2, int32_t B,
                        const int32_t* set_off, const int32_t* src, int32_t* d_out, int64_t* d_info);
int pf_clearance_widest_work(pf_handle* h, int64_t* out4);

/* ---- cost fields: exact weighted shortest paths over a per-cell cost map (pathfit.CostField) ----------------------------------
 * d_cost: a double [R C] cost map c in HBM.  Every FREE cell (grid value not 1) needs a finite c with 1 <= c <= 2^20; the words
 * on obstacle cells are ignored and never validated.  Legality of a move comes from the handle's mask byte of the policy, the
 * one pf_dist_field_merged uses; occupancy and masks are read at call time (pf_update_grid keeps working).
 * The weight of a legal move u -> v by move k:  w = m for k < 4,  w = fl(PF_SQRT2 m) for k >= 4,  m = fl(0.5 fl(c[u] + c[v])):
 * symmetric, exactly 1 / sqrt(2) when c == 1; w is rounded to a double before it is added (no fused operation anywhere).
 * pf_cost_field: B source sets in pf_dist_field_merged's host CSR form -> d_out[b * R C + v] = D[b][v], the least fixed point
 * of  D[s] = 0 on the free sources of set b,  D[v] = min over legal moves u -> v of fl(D[u] + w(u, v))  elsewhere; +inf on
 * obstacles and out of reach.  Every label is the left-to-right rounded cost of a real walk, what a heap Dijkstra leaves bit for
 * bit; with c == 1 the rows are pf_dist_field_merged's.  A source on an obstacle is skipped, one listed twice counts once, a
 * set without a usable source gives an all-inf row.  d_info (or NULL) int64 [B][4]: {the sources that counted, the cells with a
 * finite label, the cell with the largest finite label (the smallest id on a tie; -1 when nothing is reached), 0}.
 * A cost outside [1, 2^20] on a free cell, NaN and inf included, is an argument error (-1, the message names the cell) found by
 * a validation kernel BEFORE any output is touched.  Like pf_clearance_widest, tiles of 64 x 16 cells are relaxed to their own
 * fixed point in LDS, one launch per round over the queued (set, tile) pairs of all B sets; the rounds grow with the tiles an
 * optimal walk crosses, not with its cells or its cost, and the host reads one 4-byte queue length per round.  The result is
 * the least fixed point whatever the timing: identical run to run.  Scratch: pf_clearance_widest's block.
 * pf_cost_field_work (host side): out4 = {launches of the tile kernel, tile visits, words lowered, 0} of the last call: figures
 * for a probe that depend on the schedule, never part of a result.
 * pf_cost_field_parents: pf_dist_field_parents under these weights: d_parents[k * R C + v] = 0..7 the move of the last step
 * into v, 8 on a source, 255 without a route; the parent is the u with the smallest (D[u], u) among the cells with a legal move
 * u -> v and fl(D[u] + w(u, v)) == D[v] -- what a heap Dijkstra with keys (g, cell id), strict-improvement came_from and all
 * sources of the set seeded at 0 leaves.  pf_dist_field_paths and pf_dist_field_owners work on these maps unchanged.
 * pf_cost_paths: n path rows laid out as pf_astar_batch's -> d_total[q] = the left-to-right double sum of w over the row's
 * consecutive cells (0 for a one-cell row), d_bad[q] = -1; for a row with a step that is no king move between cells inside the
 * grid d_bad[q] = the index of the first such step and d_total[q] = NaN; a row with d_len <= 0 or > path_cap, or a lone cell
 * outside the grid, gives d_bad = 0 and NaN.  Occupancy is not consulted.  One wavefront per row.
 * All: a null handle (-2); B < 1, bad offsets, an empty set, an id outside the grid, K < 1, n < 0, path_cap < 1 or a missing
 * pointer (-1, with a message) is an argument error found before any launch; n == 0 returns 0.  Synchronous and ordered on the
 * handle's stream; pf_last_kernel_ms reports the span of the kernels. */
int pf_cost_field(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, int32_t B,
                  const int32_t* set_off, const int32_t* src, double* d_out, int64_t* d_info);
int pf_cost_field_work(pf_handle* h, int64_t* out4);
/* pf_cost_field_repair: the exact update of cost fields after a few cells changed.  d_rows [B][R C] holds what
 * pf_cost_field (or an earlier repair) left for the same sets and policy, computed on an occupancy and a cost map that differ
 * from the handle's present occupancy (after pf_update_grid) and from d_cost at most on the n_changed cells of `changed`, a HOST
 * array of flat cell ids; duplicates are fine, and so are cells that in fact did not change.  On return the rows, and d_info (or
 * NULL), are bit for bit what pf_cost_field would write now.  Two phases on the tile-queue engine: labels that lost their support
 * -- no legal move u -> v of the new mask with fl(D[u] + w_new(u, v)) == D[v], and every finite label on an obstacle -- are
 * raised to +inf, tile by tile from the 3 x 3 blocks about the listed cells, until nothing changes; every free source takes 0;
 * then pf_cost_field's relax kernel lowers from the tiles that had a word raised, that meet such a block or that hold a new
 * seed.  The work follows the tiles the invalid region crosses, not the map (the validation of d_cost and d_info still read the
 * map once); a change next to a source may cost as much as a fresh field or more, two phases crossing the same tiles.  The result
 * does not depend on the timing.  If the caller breaks the contract the result is unspecified, but the call ends within the
 * round bounds (R C + 1 launches a phase) and accesses nothing out of range.
 * n_changed == 0: the rows stay untouched and no tile kernel is launched; d_info is still written when given.  n_changed < 0, a
 * null `changed` with n_changed > 0, an id outside [0, R C) (the message names its index) and every argument error of
 * pf_cost_field: -1 with a message, found on the host before any launch; a bad cost on a free cell: -1, found by the validation
 * kernel BEFORE anything is written; a null handle: -2.  Afterwards pf_cost_field_work reports {tile launches of both phases,
 * tile visits of both, words lowered, words raised}: the labels that were finite before and +inf after the raise phase, a figure
 * that does not depend on the schedule (after pf_cost_field the fourth word stays 0).  pf_last_kernel_ms spans both phases.
 * Scratch: pf_clearance_widest's block, grown by one word per (set, tile) and by the device copy of the list. */
int pf_cost_field_repair(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, int32_t n_changed,
                         const int32_t* changed, int32_t B, const int32_t* set_off, const int32_t* src, double* d_rows,
                         int64_t* d_info);
int pf_cost_field_parents(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, int32_t K,
                          const double* d_fields, uint8_t* d_parents);
int pf_cost_paths(pf_handle* h, const double* d_cost, int32_t n, int32_t path_cap, const int32_t* d_cells,
                  const int32_t* d_len, double* d_total, int32_t* d_bad);

/* ---- turn fields: the exact optimum of length plus a turn penalty, over (cell, heading) states (pathfit.TurnField) ----------
 * Moves, legality and the move weight w(u, v, k) are the cost fields'; d_cost NULL means c == 1 everywhere (no buffer is read,
 * the same bits as a map of ones).  turn_weight is a finite double in [0, 2^20].  T[b][d][v] is the cheapest cost of a walk from
 * a source of set b that ENTERS v by move d:  T[d][s] = 0 for all eight d on every free source (the first move of a path is no
 * turn, as helper.py's count_turns has it);  elsewhere, with u = v - step(d) and the move u -> v legal,
 *     T[d][v] = min over d' of fl(T[d'][u] + e),   e = w for d' == d,  e = fl(w + turn_weight) otherwise;
 * +inf where the move is illegal, on obstacles and out of reach.  Every label is the left-to-right rounded cost of a real walk
 * (which may pass a cell twice), and the least fixed point is what a heap Dijkstra over the states leaves, bit for bit.
 * pf_turn_field: B source sets in pf_dist_field_merged's host CSR form -> d_states [B][8][R C] (plane-major) and d_best [B][R C],
 * best[v] = min over d of T[d][v]: the least, over all paths from a source to v, of the path's length plus turn_weight per
 * turn under the cost map; at turn_weight == 0 pf_cost_field's rows bit for bit.  d_info (or NULL) int64 [B][4] as
 * pf_cost_field's, counted on best.  Sources on obstacles, duplicates and sets without a usable source as pf_cost_field.  A bad
 * cost on a free cell (pf_cost_field's validation kernel) or a turn_weight outside [0, 2^20], NaN included, is an argument
 * error (-1) found BEFORE any output is touched.  Tiles of 32 x 16 cells with nine doubles a cell in LDS are relaxed to their own
 * fixed point, one launch per round over the queued (set, tile) pairs; one 4-byte queue length is read per round; at most
 * 8 R C + 2 rounds, and a tile's sweeps are bounded by its states + 2: beyond either the call fails with a message (DESIGN.md
 * 4.20).  Identical run to run.  Scratch: pf_clearance_widest's block.
 * pf_turn_field_work (host side): out4 = {launches of the tile kernel, tile visits, state words lowered, 0} of the last call:
 * figures for a probe that depend on the schedule, never part of a result.
 * pf_turn_field_paths: n queries (d_set_idx[q], d_target[q]) -> rows laid out as pf_dist_field_paths', from the states alone (no
 * parent map): start at the target with the heading of the smallest (T[d][t], d); at (v, d) step to u = v - step(d); stop when
 * best[u] == 0 (a source); otherwise take the d' with the smallest (T[d'][u], d') among those with fl(T[d'][u] + e) == T[d][v]
 * bit for bit.  The route's cost under pf_turn_paths equals best[target] bit for bit.  PF_ST_INFEASIBLE, length 0: no finite
 * state at the target, a target id outside [0, R C) or a set index outside [0, B).  PF_ST_OVERFLOW, length 0, row untouched:
 * more than path_cap cells -- or words that are no fixed point (no state offers the label, a step off the grid, more than R C
 * cells): the walk is bounded whatever the words hold.  One lane per query.
 * pf_turn_paths: n path rows laid out as pf_astar_batch's -> d_total[q] = the rule's cost summed left to right: a step weighs w,
 * or fl(w + turn_weight) when its move differs from the move of the step before; d_turns[q] = the steps that turned
 * (count_turns); d_bad[q] = -1.  Bad rows as pf_cost_paths: NaN, 0 turns and the first bad step.  One wavefront per row.
 * All: a null handle (-2); B < 1, bad offsets, an empty set, an id outside the grid, n < 0, path_cap < 1, a bad turn_weight or a
 * missing pointer (-1, with a message) is an argument error found before any launch; n == 0 returns 0.  Synchronous and ordered
 * on the handle's stream; pf_last_kernel_ms reports the span of the kernels. */
int pf_turn_field(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, double turn_weight, int32_t B,
                  const int32_t* set_off, const int32_t* src, double* d_states, double* d_best, int64_t* d_info);
int pf_turn_field_work(pf_handle* h, int64_t* out4);
/* pf_turn_field_repair: the exact update of a turn field after a few cells changed.  d_states [B][8][R C] and
 * d_best [B][R C] hold what pf_turn_field (or an earlier repair) left for the same sets, policy and turn_weight, computed on an
 * occupancy and a cost map that differ from the handle's present occupancy (after pf_update_grid) and from d_cost (NULL: ones) at
 * most on the n_changed cells of `changed`, a HOST array of flat cell ids; duplicates are fine, and so are cells that in fact did
 * not change.  On return the states, best and d_info (or NULL) are bit for bit what pf_turn_field would write now.  Two phases on
 * the tile-queue engine over the turn tile: the finite states that lost their support -- no d' with
 * fl(T[d'][u] + e(d', d)) == T[d][v] over a legal move u -> v of the new mask, u = v - step(d), and every finite state on an
 * obstacle -- are raised to +inf, tile by tile from the 3 x 3 blocks about the listed cells, until nothing changes, and best is
 * rewritten as the minimum of what survives (it may rise to a finite value); every free source takes 0 in its nine words; then
 * pf_turn_field's relax kernel lowers from the tiles that had a state raised, that meet such a block or that hold a new seed.
 * The work follows the tiles the invalid region crosses, not the map; a change next to a source may cost as much as a fresh field
 * or more.  The result does not depend on the timing.  If the caller breaks the contract the result is unspecified, but the call
 * ends within the round bounds (8 R C + 1 launches a phase) and the sweep bound, and accesses nothing out of range.
 * n_changed == 0: the rows stay untouched and no tile kernel is launched; d_info is still written when given.  n_changed < 0, a
 * null `changed` with n_changed > 0, an id outside [0, R C) (the message names its index) and every argument error of
 * pf_turn_field: -1 with a message, found on the host before any launch; a bad cost on a free cell: -1, found by the validation
 * kernel BEFORE anything is written; a null handle: -2.  Afterwards pf_turn_field_work reports {tile launches of both phases,
 * tile visits of both, state words lowered, state words raised}: the states that were finite before and +inf after the raise
 * phase, a figure that does not depend on the schedule (after pf_turn_field the fourth word stays 0).  pf_last_kernel_ms spans
 * everything.  Scratch: pf_clearance_widest's block, grown by one word per (set, tile), six words and the device copy of the list. */
int pf_turn_field_repair(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, double turn_weight,
                         int32_t n_changed, const int32_t* changed, int32_t B, const int32_t* set_off, const int32_t* src,
                         double* d_states, double* d_best, int64_t* d_info);
int pf_turn_field_paths(pf_handle* h, const double* d_cost, double turn_weight, int32_t B, const double* d_states, int32_t n,
                        const int32_t* d_set_idx, const int32_t* d_target, int32_t reverse, int32_t path_cap, int32_t* d_cells,
                        int32_t* d_len, int32_t* d_status);
int pf_turn_paths(pf_handle* h, const double* d_cost, double turn_weight, int32_t n, int32_t path_cap, const int32_t* d_cells,
                  const int32_t* d_len, double* d_total, int32_t* d_turns, int32_t* d_bad);

/* ---- visibility fields: what each viewpoint sees, exposure counts, the exposure of path rows (pathfit.Visibility) -----------
 * The rule is the smoothing section's visible(a, b, restrict_corner), evaluated from one cell to all: the cells
 * of the bounding box with |2k| < s are crossed, those with |2k| == s touched; b is seen from a iff no crossed cell is an
 * obstacle and, with restrict_corner != 0, no touched one either; a == b is seen iff the cell is free; the endpoints are
 * crossed.  So a viewpoint on an obstacle sees nothing, an obstacle is never seen, and the relation is symmetric.  With
 * max_range_sq >= 0 a cell counts only if dr^2 + dc^2 <= max_range_sq (integers); -1 means no limit.  `view` is a HOST array of
 * K cell ids (as pf_dist_field_batch's sources); the occupancy is read at call time (pf_update_grid keeps working).
 * pf_visibility_field: d_seen[k * R C + v] = 1 where view[k] sees v within the range, else 0; every byte of the K rows is
 * written.  d_info (or NULL) int64 [K][4]: {cells seen, the largest dr^2 + dc^2 among them, the smallest cell id that attains
 * it, 0}; {0, -1, -1, 0} when nothing is seen.  One lane per target, 64 consecutive cells per wavefront: a lane walks its own
 * sight line and leaves at the first blocker.
 * pf_visibility_count: d_count[v] = the number of k with view[k] seeing v (a viewpoint listed twice counts twice); the K masks
 * are never materialised.  d_info (or NULL) int64 [4]: {free cells with count > 0, free cells, the largest count over the free
 * cells, the smallest free cell id that attains it}; the last two -1 on a map without a free cell.  Integer sums (a lane per (viewpoint,
 * cell) pair and one integer atomic per seen pair): identical run to run.
 * pf_visibility_paths: n path rows laid out as pf_astar_batch's against counts in HBM (int32 [R C]) -> d_out[i * 4 ..] = {the
 * sum of the counts over the row's cells, the largest count, the position of the first cell that attains it, the cells with
 * count > 0}; d_profile (or NULL) [n * path_cap]: the count per cell, words beyond d_len[i] untouched.  d_status: 0 ok; 1 = an
 * empty row, a length beyond path_cap or a cell outside [0, R C): d_out = {0, -1, -1, 0}, the profile row untouched, nothing read
 * out of range.  One wavefront per row.
 * A null handle (-2); K < 1, max_range_sq < -1, a viewpoint outside [0, R C) (the message names its index), R^2 + C^2 >= 2^31 - 1,
 * a missing required pointer, n < 0 or path_cap < 1 (-1, with a message) is an argument error found before any launch; n == 0
 * returns 0 and launches nothing.  All three are synchronous and ordered on the handle's stream; pf_last_kernel_ms reports the
 * kernels.  Scratch: the distance fields' control block (the viewpoints and a few 64-bit words). */
int pf_visibility_field(pf_handle* h, int32_t restrict_corner, int32_t max_range_sq, int32_t K, const int32_t* view,
                        uint8_t* d_seen, int64_t* d_info);
int pf_visibility_count(pf_handle* h, int32_t restrict_corner, int32_t max_range_sq, int32_t K, const int32_t* view,
                        int32_t* d_count, int64_t* d_info);
int pf_visibility_paths(pf_handle* h, const int32_t* d_count, int32_t n, int32_t path_cap, const int32_t* d_cells,
                        const int32_t* d_len, int64_t* d_out, int32_t* d_profile, int32_t* d_status);

/* ---- space-time fields: arrival ticks and routes among moving obstacles (pathfit.SpaceTime) ---------------------------------
 * Time runs in ticks 0..T (the horizon, 0 <= T <= 2^20).  In a tick a robot waits or makes one move of the policy (allow_diag,
 * restrict_corner, as pf_dist_field_batch's); every move takes one tick.  S is the handle's static occupancy at call time
 * (pf_update_grid keeps working), D[t] the dynamic plane of tick t, A[t] = S | D[t].  The planes are the device buffer d_occ,
 * uint64 [T + 1][R][Wc] with Wc = ceil(C / 64): cell (r, c) is bit c & 63 of word r Wc + (c >> 6); the bits at c >= C are 0.
 * A robot at u at tick t may be at v at tick t + 1 iff
 *   1. v is inside the grid and A[t + 1][v] == 0 (vertex);
 *   2. v == u (wait), or u -> v is a straight step, or a diagonal step when allow_diag;
 *   3. for a move, not both D[t][v] and D[t + 1][u] are set (swap / pass-through; the test is on the planes, so two different
 *      obstacles that set the two bits forbid the move too);
 *   4. for a diagonal move under restrict_corner, neither (v.r, u.c) nor (u.r, v.c) is set in A[t] | A[t + 1].
 * With every D[t] zero, rules 1, 2 and 4 are the handle's move-mask byte of the policy.  reach[0] = the sources free in A[0];
 * reach[t + 1][v] = some u of reach[t] may be at v at tick t + 1.  reach is not monotone in t.  arrive[v] = the least t <= T with
 * reach[t][v], -1 if none; the hold tick of v = the least t with reach[t][v] and D[t'][v] == 0 for every t <= t' <= T.
 * pf_spacetime_stamp: ORs n path rows laid out as pf_astar_batch's into d_occ: the cell at position j of row i at tick
 * d_t0[i] + j (d_t0 NULL: 0).  after_end != 0: the last cell stays occupied to tick T, else the obstacle vanishes.  corners != 0:
 * a unit diagonal step over t -> t + 1 also stamps its two orthogonal corner cells at ticks t and t + 1 (the swept footprint);
 * other steps stamp none.  clear != 0 zeroes the planes first.  Ticks beyond T are dropped; consecutive cells need not be
 * adjacent.  d_status: 0 ok; 1 = an empty row, a length beyond path_cap, a cell outside [0, R C) or a t0 outside [0, T]: nothing
 * of the row is stamped, nothing is read out of range.  64-bit atomic ORs: rows may overlap.
 * pf_spacetime_field: B source sets in pf_dist_field_merged's host CSR form (an empty set is legal) -> d_arrive int32 [B][R C],
 * every word written; d_reach (or NULL) uint64 [B][T + 1][R Wc], every word written; d_info (or NULL) int64 [B][4] = {cells
 * reached, the largest arrival tick, the smallest cell id that attains it, 0}, {0, -1, -1, 0} when nothing is reached.  A source
 * on a cell occupied at tick 0 is skipped, one listed twice counts once, a set without a usable source reaches nothing.  One
 * workgroup per set, min(B, CUs) of them, the tick loop inside the kernel, 64 cells to a word; the three live planes of a
 * workgroup lie in LDS where 3 R Wc 8 bytes fit 60 KiB, else in the handle's scratch in HBM.
 * pf_spacetime_paths: n queries (d_set_idx[q], d_target[q], d_tick[q]) through d_reach (B sets) and d_occ -> rows d_cells
 * [n][path_cap], d_len, d_status and d_tick_out (or NULL), the tick used (-1 where none).  d_tick[q] == -1: the earliest arrival;
 * -2: the hold tick; >= 0: that tick; d_tick NULL: all -1.  A row holds tick + 1 cells, cell j the position at tick j.  From (tick,
 * target) the walk goes back: at (t, v), t > 0, the first u with reach[t - 1][u] and u -> v allowed over t - 1 -> t among
 * u = v - step(d), d = 0..7 in pf_dist_field_parents' move order, then u = v (the wait last).  PF_ST_INFEASIBLE, length 0: the
 * reach bit is not set, the tick lies beyond T or below -2, no hold tick exists, or the target or the set index is out of range.
 * PF_ST_OVERFLOW, length 0, row untouched: tick + 1 > path_cap, or some tick has no predecessor (planes that pf_spacetime_field
 * did not produce on this map).  A walk makes at most `tick` steps and reads inside the planes whatever the words hold.
 * pf_spacetime_conflicts: n rows of the same layout, starting at d_t0[i] (NULL: 0), against S, d_occ and the policy -> d_out
 * int32 [n][4] = {the first conflicting tick or -1, its kind (0: none), the cell the robot would enter or -1, the number of
 * conflicting steps}.  Kinds, by precedence at one step: 1 static (the cell is a static obstacle, or the step is neither a wait
 * nor a move of the policy on the static map), 2 vertex, 3 swap, 4 corner.  The row's first cell is checked as a vertex at t0 (on a
 * static obstacle: kind 1); a step t -> t + 1 reports tick t + 1.  hold != 0 also checks the last cell as a vertex at every later
 * tick up to T, each such tick one conflicting step.  d_status: 0 ok; 1 a bad row as the stamp's (d_out = {-1, 0, -1, 0}); 2 the row
 * runs past the horizon: checked up to T, the steps beyond not counted, no hold check.
 * A null handle (-2); T outside [0, 2^20], B < 1, offsets that do not start at 0 or that decrease, a source outside [0, R C) (the
 * message names its index), n < 0, path_cap < 1 or a missing required pointer (-1, with a message) is an argument error found
 * before any launch: no output is touched; n == 0 returns 0 and launches nothing.  All four are synchronous and ordered on the
 * handle's stream; pf_last_kernel_ms reports the kernels. */
int pf_spacetime_stamp(pf_handle* h, int32_t T, uint64_t* d_occ, int32_t n, int32_t path_cap, const int32_t* d_cells,
                       const int32_t* d_len, const int32_t* d_t0, int32_t after_end, int32_t corners, int32_t clear,
                       int32_t* d_status);
int pf_spacetime_field(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t T, const uint64_t* d_occ, int32_t B,
                       const int32_t* set_off, const int32_t* src, int32_t* d_arrive, uint64_t* d_reach, int64_t* d_info);
int pf_spacetime_paths(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t T, const uint64_t* d_occ, int32_t B,
                       const uint64_t* d_reach, int32_t n, const int32_t* d_set_idx, const int32_t* d_target,
                       const int32_t* d_tick, int32_t path_cap, int32_t* d_cells, int32_t* d_len, int32_t* d_status,
                       int32_t* d_tick_out);
int pf_spacetime_conflicts(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t T, const uint64_t* d_occ, int32_t n,
                           int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, const int32_t* d_t0, int32_t hold,
                           int32_t* d_out, int32_t* d_status);

/* ---- tours: the exact best order through up to 16 stops (pathfit.Tour) -------------------------------------------------------
 * A problem is an n x n matrix d of doubles, d[i n + j] the cost of going from node i to node j: not necessarily symmetric,
 * +inf = no way, the diagonal never read.  Node 0 is the start.  mode 0 (open): the tour may end anywhere; 1 (return): it comes
 * back to node 0; 2 (last): it ends at node n - 1.  The middle nodes M are the others: m = n - 1, or n - 2 in mode 2; 0 <= m <= 16.
 * need[j] (HOST uint32 [n], or NULL: none) is the set of nodes that must come before j; bit 0 is always satisfied, the end's own
 * needs are always met, and in mode 2 a middle node that needs node n - 1 can never be placed.  For S a subset of M and j in S
 * 
 *   f[S][j] = +inf if need[j] & M is no subset of S \ {j}, or if a middle j needs the end; else d[0][j] if S == {j}; else the
 *             minimum over i in S \ {j} of fl(f[S \ {j}][i] + d[i][j]), one fp64 addition per candidate;
 *   total   = min_j f[M][j] (mode 0), min_j fl(f[M][j] + d[j][0]) (mode 1), min_j fl(f[M][j] + d[j][n - 1]) (mode 2).
 * The order is read back by one rule: the last middle node is the smallest j whose closing value equals total as a 64-bit word;
 * from (S, j) the predecessor is the smallest i in S \ {j} with fl(f[S \ {j}][i] + d[i][j]) == f[S][j] as words.  fp64 addition
 * is monotone, so total is bit for bit the minimum over all admissible permutations of the legs' left-to-right sum, and the
 * returned order's left-to-right sum is total.  m == 0: total 0 and order [0] (n == 1), or total d[0][1] and order [0, 1] (mode 2).
 * pf_tour_matrix: d_mat[i n + j] = d_fields[i R C + stops[j]] for n HOST cell ids `stops` and n field rows in HBM (row i the field
 * from stop i, as pf_dist_field_batch or pf_cost_field leave them): a plain gather, neither symmetrised nor cleaned.
 * pf_tour_solve: B problems d_mat [B][n][n] that share n, mode and need -> d_total [B]; d_order int32 [B][n], the nodes in
 * visiting order (it begins with 0, does not repeat 0 in mode 1, ends with n - 1 in mode 2); d_status [B], 0 or 1 = infeasible
 * (total == +inf: a stop out of reach, cyclic needs; the order row is all -1); d_info (or NULL) int64 [B][4] = {the number of
 * finite f[S][j], the last middle node or -1, 0, 0}.  One layer per set size with a lane per state; for m <= 9 a workgroup per
 * problem keeps the table in LDS with the layer loop in the kernel, above that the tables lie in the handle's scratch (2^m m 8
 * bytes each) with one launch per layer, at most "tour_tables" problems in flight (pf_set_option; 0 = as many as fit 256 MiB),
 * the batch running in chunks.  Results never depend on the form, the chunks or the timing.
 * Every off-diagonal entry must be >= 0 or +inf: a NaN or a negative entry is -1 with a message naming (b, i, j), found by a
 * validation kernel BEFORE anything is written.  A null handle (-2); n < 1, mode 2 with n < 2, m > 16, a mode outside 0..2,
 * B < 1, need[0] != 0, a node needing itself, a need bit >= n, a stop outside [0, R C) (the message names its index) or a missing
 * required pointer (-1, with a message) is an argument error found on the host before any launch: no output is touched.  Both
 * are synchronous and ordered on the handle's stream; pf_last_kernel_ms reports the kernels (the validation included). */
int pf_tour_matrix(pf_handle* h, int32_t n, const int32_t* stops, const double* d_fields, double* d_mat);
int pf_tour_solve(pf_handle* h, int32_t mode, int32_t n, const uint32_t* need, int32_t B, const double* d_mat, double* d_total,
                  int32_t* d_order, int32_t* d_status, int64_t* d_info);

/* ---- assignments: the exact best robot-to-task matching (pathfit.Assignment) --------------------------------------------------
 * A problem is an n x m matrix a of doubles, row-major.  Rows are robots and columns are tasks, with 1 <= n <= m <= 1024
 * (PF_ASSIGN_MAX).  +inf means no way.  Every other entry is finite with |x| <= 2^1000.  Negative entries are allowed.  NaN and
 * -inf are errors.  There are three modes.
 * Mode 0, "sum".  Rows are inserted in order i = 0 .. n-1.  The state is: potentials u[n] and v[m], all 0 at the start; p[m], the
 * row matched to each column, -1 at the start.  Per inserted row, set minv[j] = +inf, way[j] = -1, used[j] = false, i0 = i,
 * j0 = -1.  Then repeat tree steps.  One tree step is:
 *   1. For every unused j in ascending order: cur = fl(fl(x - u[i0]) - v[j]), where x = a[i0][j], or +inf if x > limit.  If
 *      cur < minv[j], set minv[j] = cur and way[j] = j0.  The comparison is strict.
 *   2. delta is the smallest minv[j] over the unused j, and j1 is the smallest such j.  If there is none, or delta == +inf, the
 *      row cannot be placed and the problem is infeasible.
 *   3. u[i] += delta.  For every used j: u[p[j]] += delta and v[j] -= delta.  For every unused j: minv[j] -= delta.
 *   4. j0 = j1, used[j0] = true.  If p[j0] < 0, the tree ends.  Otherwise i0 = p[j0].
 * After the tree ends, augment along way from j0 back to -1: p[j0] = p[way[j0]], and the first column receives row i.  Each line
 * is one fp64 operation in the order written.  No multiplication occurs, so nothing can contract.  limit is +inf in mode 0.
 * Mode 1, "max" (bottleneck, the makespan).  The loop is the same without potentials: cur = a[i0][j], there is no step 3, and
 * t = max(t, delta) with t = -inf at the start.  Only comparisons occur.  t is exactly the smallest possible largest entry over
 * all assignments.
 * Mode 2, "max_sum".  Run mode 1.  Then run mode 0 from fresh state with limit = t.  The result is the cheapest assignment among
 * those with the best makespan.
 * Results.  col[i] is the column of row i.  value = {sum, max}: sum is the left-to-right fp64 sum of a[i][col[i]] for
 * i = 0 .. n-1, max is the largest of those entries.  dual holds u then v; it is all zeros in mode 1.  info = {tree steps of the
 * sum phase, tree steps of the max phase, the first row that could not be placed or -1, 0}; a step that finds no column counts.
 * An infeasible problem has status 1, col all -1, value = {+inf, +inf}, and dual all zeros.
 * The device's col, value, dual and info equal the rule's as 64-bit words, on every run and in every kernel form.  Mode 1's t is
 * exact on any input.  Mode 0's sum is the exact minimum over all assignments wherever every operation is exact (integer-valued
 * and dyadic matrices of moderate size); on other matrices it is the left-to-right sum of some assignment, never below the
 * brute-force minimum of left-to-right sums, and the reduced costs a - u - v can fall below zero by rounding.
 * pf_assign_matrix: d_mat[(row0 + i) ld + j] = d_fields[i R C + cols[j]] for i < n_rows field rows in HBM (a chunk: i counts
 * within it) and n_cols HOST cell ids `cols`; with `transpose` the value goes to d_mat[j ld + row0 + i].  A plain gather.
 * pf_assign_solve: B problems d_mat [B][n][m] that share n, m and mode -> d_col int32 [B][n], d_value [B][2], d_status [B],
 * d_dual [B][n + m] (or NULL), d_info int64 [B][4] (or NULL).  Up to 64 columns a wavefront solves a problem, column j in lane j;
 * above that a workgroup does, a thread holding its columns in registers.  One launch per call, whatever B.
 * A null handle (-2); n < 1, m < n, m > 1024, a mode outside 0..2, B < 1, a missing required pointer; for pf_assign_matrix a
 * count outside [1, 32768], row0 < 0, ld shorter than a row of the matrix or a cell outside [0, R C) (-1, with a message) is an
 * argument error found on the host before any launch.  A bad entry is -1 with a message naming the first (b, i, j), found by a
 * validation kernel BEFORE anything is written.  Both are synchronous and ordered on the handle's stream; pf_last_kernel_ms
 * reports the kernels (the validation included). */
#define PF_ASSIGN_MAX 1024
int pf_assign_matrix(pf_handle* h, int32_t n_rows, int32_t n_cols, const int32_t* cols, const double* d_fields, int32_t row0,
                     int32_t ld, int32_t transpose, double* d_mat);
int pf_assign_solve(pf_handle* h, int32_t mode, int32_t n, int32_t m, int32_t B, const double* d_mat, int32_t* d_col,
                    double* d_value, int32_t* d_status, double* d_dual, int64_t* d_info);

/* ---- tour search: 2-opt local search for tours of up to 1 024 stops (pathfit.TourSearch) --------------------------------------
 * A problem is an n x n matrix d of doubles, 1 <= n <= 1024 (PF_TOUR_SEARCH_MAX).  Node 0 is the start.  
 * Weights.  The rule reads the upper triangle only: w(x, y) = d[min(x, y) n + max(x, y)] for x != y.  The lower triangle and the
 * diagonal are never read, so the weights are symmetric as 64-bit words.  w(x, none) = +0.0, and w(x, x) = +0.0 (the closing leg
 * of n == 1 in mode 1, the only place a node meets itself).
 * Modes are pf_tour_solve's.  Mode 0, open: the tour ends anywhere.  Mode 1, return: it comes back to node 0.  Mode 2, last: it
 * ends at node n - 1.
 * The order row.  order[0 .. n-1] is a permutation of the nodes with order[0] = 0; in mode 2, order[n-1] = n - 1.  order[n]
 * stands for order[0] in mode 1 and for "none" in modes 0 and 2.  The movable positions are 1 .. hi, with hi = n - 1 in modes 0
 * and 1, and hi = n - 2 in mode 2.
 * n = 1 is a problem in every mode (in mode 2 node 0 is the start and the end): no pair, one sweep, status 0, value {+0.0, +0.0}.
 * One sweep.  For every pair 1 <= i < j <= hi take a = order[i-1], b = order[i], c = order[j], e = order[j+1] and
 *   delta(i, j) = fl( fl(w(a,c) + w(b,e)) - fl(w(a,b) + w(c,e)) ).
 * That is three fp64 operations in the order written; nothing can contract.  The move of the sweep is the pair with the smallest
 * delta.  On a tie it is the one with the smallest i, then the smallest j.  If that delta is < 0 (strictly) and fewer than
 * max_moves moves were applied, positions i .. j are reversed.  That is one move.  Then sweep again.
 * Stopping.  A sweep that finds no delta < 0 (or no pair at all) ends the search: the order is a local optimum, status 0.  A
 * sweep that finds one after max_moves moves ends it too: status 2, the order is whatever the moves so far made.  So a call runs
 * at most max_moves + 1 sweeps per start, 0 <= max_moves <= 2^20, and status 2 says that an improving move exists.  fl is
 * monotone, so an accepted move strictly shortens the real-number length of the tour and the search ends without the cap.
 * Results per start.  value = {total after, total before}.  Each is the left-to-right fp64 sum of w(order[k], order[k+1]) for
 * k = 0 .. n-1, where the last term is the closing leg in mode 1 and +0.0 otherwise.  info = {moves, sweeps, 0, 0}.
 * Entries.  Every upper-triangle entry must be >= 0 and either <= 2^1000 or +inf.  The rule needs finite weights: a problem with
 * a +inf entry anywhere in its upper triangle is NOT searched.  Every start over it has status 1, an order row of all -1,
 * value = {+inf, +inf} and info all 0.  The other problems of the batch are searched.
 * pf_tour_improve: B starts d_order int32 [B][n], in and out, over one matrix d_mat [n][n] (shared = 1) or over d_mat [B][n][n]
 * (shared = 0) -> d_value [B][2], d_status [B], d_info int64 [B][4] (or NULL).  One workgroup of 1024 threads per start holds
 * the order row and its legs in LDS and runs the move loop inside the kernel.  The pairs are dealt evenly to its threads, the
 * minimum is one lexicographic reduction over (delta, i, j), the reversal is applied by the threads in parallel.  The matrix is
 * read through the caches.  One launch per call, whatever B.  The device's orders, values, statuses and infos equal the rule's
 * as 64-bit words, on every run and for every assignment of starts to workgroups.
 * A null handle (-2); n outside [1, 1024], B < 1, a mode outside 0..2, shared outside 0..1, max_moves outside [0, 2^20] or a
 * missing required pointer (-1, with a message) is an argument error found on the host before any launch.  A NaN, a negative
 * entry or a finite entry above 2^1000 in an upper triangle is -1 with a message naming the first (b, i, j).  A start row that
 * is no permutation of 0 .. n-1 with node 0 first (and node n - 1 last in mode 2) is -1 with a message naming the first
 * (b, position): the first position whose node lies outside [0, n), repeats the node of a smaller position or breaks a fixed
 * end.  Two validation kernels find both BEFORE anything is written.  The call is synchronous and ordered on the handle's stream;
 * pf_last_kernel_ms reports the kernels (the validations included). */
#define PF_TOUR_SEARCH_MAX 1024
int pf_tour_improve(pf_handle* h, int32_t mode, int32_t n, int32_t B, int32_t shared, const double* d_mat, int32_t max_moves,
                    int32_t* d_order, double* d_value, int32_t* d_status, int64_t* d_info);

/* ---- fleet routes: k robots over n tasks, 2-opt and segment relocation (pathfit.FleetTours) ------------------------------------
 * A problem is k robots and n tasks, k >= 1, n >= 1, N = k + n <= 1024 (PF_FLEET_MAX).  Nodes 0 .. k-1 are the robots' start
 * cells, nodes k .. N-1 are the tasks.  The weights are an N x N matrix d of doubles.  
 * Weights.  The rule reads the upper triangle only: w(x, y) = d[min(x, y) N + max(x, y)] for x != y.  w(x, x) = +0.0 and
 * w(x, none) = +0.0.  The robot-robot entries, the diagonal and the lower triangle are never read.
 * The route row.  route[0 .. N-1] is a permutation of the nodes.  route[0] = 0, and the robots appear in increasing order: robot
 * r's marker stands before robot r+1's.  The tasks between marker r and the next marker (or the end of the row) are robot r's
 * route, in visiting order.  A route may be empty.  rob(p) is the robot whose stretch holds position p.  cnt[r] is the number of
 * tasks of robot r.  nxt(p) is route[p+1] if p+1 < N and that node is a task; otherwise it is END(rob(p)).  END(r) is "none" in
 * mode 0 (open: a route ends at its last task) and node r in mode 1 (return: each robot comes back to its own start).
 * Capacity.  cap[r] >= 0 is an optional int32 per robot, shared by the batch; NULL means unlimited.  A row is valid only if
 * cnt[r] <= cap[r] for every r.
 * One sweep evaluates two families of candidates.
 * Family code 0, 2-opt inside a route.  For every 1 <= i < j <= N-1 with the positions i .. j all tasks take a = route[i-1],
 * b = route[i], c = route[j], e = nxt(j) and
 *   delta = fl( fl(w(a,c) + w(b,e)) - fl(w(a,b) + w(c,e)) ),
 * pf_tour_improve's form.  Applying it reverses the positions i .. j.
 * Family code L = 1, 2, 3, relocate a segment.  The positions i .. i+L-1 must all be tasks.  j may be any position with j < i-1
 * or j > i+L-1, markers included: j can be the head of another robot's route, or an empty route.  The candidate is admissible
 * iff rob(j) == rob(i) or cnt[rob(j)] + L <= cap[rob(j)].  Take a = route[i-1], s1 = route[i], sL = route[i+L-1], b = nxt(i+L-1),
 * p = route[j], q = nxt(j) and
 *   rem   = fl( fl(w(a,s1) + w(sL,b)) - w(a,b) ),
 *   add   = fl( fl(w(p,s1) + w(sL,q)) - w(p,q) ),
 *   delta = fl( add - rem ).
 * Each line is fp64 operations in the order written; nothing can contract.  Applying it takes the segment out and puts it back,
 * in the same direction, directly behind position j's node.
 * The move of the sweep is the admissible candidate with the smallest (delta, family code, i, j), compared lexicographically.  It
 * is applied iff its delta is < 0 (strictly) and fewer than max_moves moves were applied.  Then sweep again.
 * Stopping.  Status 0: a sweep found no delta < 0.  Status 2: a sweep found one after max_moves moves, 0 <= max_moves <= 2^20.  So
 * a call runs at most max_moves + 1 sweeps per start.  The relocate delta is nested roundings (add and rem are rounded before
 * they meet), so an accepted move need NOT shorten the real-number total, and a search can walk in a circle among rows whose
 * totals agree to a rounding: termination rests on the cap, not on monotonicity.
 * Results per start.  len[r] is robot r's length: the left-to-right fp64 sum of w(route[p], nxt(p)) over the positions of its
 * stretch from its marker on, the END leg last (an empty route is the one leg w(r, END) = +0.0).  value = {total after, total
 * before, makespan after}: total is the left-to-right sum of len[0 .. k-1], makespan the largest len.  info = {moves, sweeps, 2-opt
 * moves, relocate moves}.
 * Entries.  Every readable entry (i < j, j a task) must be >= 0 and either <= 2^1000 or +inf.  A problem with a +inf readable
 * entry is NOT searched: status 1, a route row of all -1, value = {+inf, +inf, +inf}, len all +inf, info all 0.  The other
 * problems of the batch are searched.
 * pf_fleet_improve: B starts d_route int32 [B][N], in and out, over one matrix d_mat [N][N] (shared = 1) or over d_mat [B][N][N]
 * (shared = 0), under d_cap int32 [k] (or NULL) -> d_len [B][k], d_value [B][3], d_status [B], d_info int64 [B][4] (or NULL).
 * One workgroup of 1024 threads per start runs the move loop inside the kernel; LDS holds the route row, rob per position, cnt
 * and cap, nxt and the legs w(route[p], nxt(p)) of the row as it stands and rem per (L, i).  The candidates are dealt evenly to
 * the threads, the minimum is one lexicographic reduction over (delta, code, i, j), the move is applied by the threads in parallel,
 * the lengths are summed by one thread per robot.  The matrix is read through the caches.  One launch per call, whatever B.  The
 * device's routes, lengths, values, statuses and infos equal the rule's as 64-bit words, on every run and for every assignment
 * of starts to workgroups.
 * A null handle (-2); k < 1, n < 1, k + n > 1024, B < 1, a mode outside 0..1, shared outside 0..1, max_moves outside [0, 2^20], a
 * negative cap[r] (the k words are read back first) or a missing required pointer (-1, with a message) is an argument error
 * found on the host before any launch.  A NaN, a negative entry or a finite entry above 2^1000 among the readable entries is -1
 * with a message naming the first (b, i, j).  A start row is -1 with a message naming the first (b, position) whose node lies
 * outside [0, N), repeats the node of a smaller position, is not node 0 at position 0, or is a robot r >= 1 that robot r-1 does
 * not stand in front of.  A robot with more tasks than its capacity is -1 with a message naming the first (b, robot).  Three
 * validation kernels find these, in this order, BEFORE anything is written.  The call is synchronous and ordered on the handle's
 * stream; pf_last_kernel_ms reports the kernels (the validations included). */
#define PF_FLEET_MAX 1024
int pf_fleet_improve(pf_handle* h, int32_t mode, int32_t k, int32_t n, int32_t B, int32_t shared, const double* d_mat,
                     const int32_t* d_cap, int32_t max_moves, int32_t* d_route, double* d_len, double* d_value, int32_t* d_status,
                     int64_t* d_info);

/* ---- fleet routes under the min-max objective: the same candidates, priced by the largest length (pathfit.FleetTours,
 * objective="makespan") -------------------------------------------------------------------------------------------------------------
 * 
 * What is pf_fleet_improve's.
 * - The problem, the weights w, the route row, rob, cnt, nxt, END, the modes and the capacities.
 * - The two candidate families (code 0: 2-opt inside a route; code L = 1, 2, 3: relocation of L tasks behind any position j,
 *   markers included), their (i, j) and their admissibility.
 * - Per candidate delta, and for a relocation rem and add: the formulas above, unchanged, each line fp64 in the order written.
 * - How a candidate is applied.  The entries a problem may hold.  Status 1 for a problem with a +inf readable entry.
 * The lengths the rule carries.
 * - len[0 .. k-1] are doubles.  At the start len[r] is robot r's length in the start row: the left-to-right fp64 sum of
 *   w(route[p], nxt(p)) over the positions of its stretch from its marker on (pf_fleet_improve's len).
 * - span = the largest of len[0 .. k-1].  Lengths are compared by value.
 * The price of a candidate.  s = rob(i), d = rob(j).
 * - A 2-opt, or a relocation with s == d, touches route s alone:
 *     len'[s] = fl( len[s] + delta ),
 *     span'   = the largest of len'[s] and of len[r] over the robots r != s.
 * - A relocation with s != d touches two routes.  rem and add are the changes of the legs AROUND the segment; the segment's own
 *   L-1 legs leave route s and enter route d with it (in the total they cancel, in the two lengths they do not):
 *     inner   = +0.0 for L = 1, w(s1,s2) for L = 2, fl( w(s1,s2) + w(s2,s3) ) for L = 3   (s1, s2, s3 = route[i], route[i+1], route[i+2]),
 *     len'[s] = fl( fl(len[s] - rem) - inner ),
 *     len'[d] = fl( fl(len[d] + add) + inner ),
 *     span'   = the largest of len'[s], len'[d] and of len[r] over the robots r other than s and d.
 * - Over no robots at all (k = 1, or k = 2 with s != d) the last term is absent.
 * One sweep.
 * - The move of the sweep is the admissible candidate with the smallest (span', delta, family code, i, j), compared
 *   lexicographically.
 * - It is applied iff span' < span, or span' == span and delta < 0; and only while fewer than max_moves moves were applied.
 * - When it is applied, the row changes as in pf_fleet_improve, len[s] becomes len'[s] and, for s != d, len[d] becomes len'[d].
 *   Every other len[r] stays.  Nothing is summed again from the row: the next sweep prices its candidates with these words, and
 *   its span is their largest, which is the applied span'.  So span never rises from one sweep to the next.
 * - Then sweep again.
 * Stopping.
 * - Status 0: a sweep has no admissible candidate, or its move fails the test above.
 * - Status 2: a sweep's move passes the test after max_moves moves, 0 <= max_moves <= 2^20.
 * - A call runs at most max_moves + 1 sweeps per start.
 * - With weights that are integers below 2^53 / N every line is exact, the carried len are the true lengths and an applied move
 *   lowers (makespan, total) lexicographically: no row can recur.  With other weights delta and the carried len are rounded,
 *   a move whose true change is 0 may carry a delta of -1 ulp, and a search can walk among such rows until the cap.
 * Results per start.
 * - d_route: the final row.
 * - d_len [k]: the left-to-right lengths of the FINAL ROW, summed again from it as pf_fleet_improve does (not the carried words).
 * - value = {makespan after, total after, makespan before, total before}: total is the left-to-right sum of len[0 .. k-1],
 *   makespan the largest; "after" of d_len, "before" of the start row's lengths.
 * - info = {moves, sweeps, 2-opt moves, relocate moves, moves with span' < span}.
 * - A problem with a +inf readable entry: status 1, a row of all -1, value = {+inf, +inf, +inf, +inf}, len all +inf, info all 0.
 * pf_fleet_balance takes pf_fleet_improve's arguments: B starts d_route int32 [B][N], in and out, over d_mat [N][N] (shared = 1)
 * or [B][N][N] (shared = 0), under d_cap int32 [k] (or NULL) -> d_len [B][k], d_value [B][4], d_status [B], d_info int64 [B][5]
 * (or NULL).  One workgroup of 1024 threads per start runs the move loop inside the kernel, over pf_fleet_improve's LDS rows; LDS
 * also holds len[k] and the three largest lengths with their robots, found at the head of a sweep, so that the largest length
 * outside a candidate's one or two routes is a pick among three (by value: which robot a tie names changes nothing).  One launch
 * per call, whatever B.  The device's routes, lengths, values, statuses and infos equal the rule's as 64-bit words, on every run
 * and for every assignment of starts to workgroups.
 * The argument errors, the validation kernels, their order and their messages are pf_fleet_improve's, under this call's name. */
int pf_fleet_balance(pf_handle* h, int32_t mode, int32_t k, int32_t n, int32_t B, int32_t shared, const double* d_mat,
                     const int32_t* d_cap, int32_t max_moves, int32_t* d_route, double* d_len, double* d_value, int32_t* d_status,
                     int64_t* d_info);

/* ---- placement: which p of m candidate sites to open for n demands, additions and swaps (pathfit.Placement) ---------------------
 * 
 * The problem.
 * - There are m sites, n demands and p slots.
 * - The limits are 1 <= m <= 1 024 (PF_PLACE_SITES_MAX), 1 <= n <= 4 096 (PF_PLACE_DEMANDS_MAX) and 1 <= p <= min(m, 64)
 *   (PF_PLACE_OPEN_MAX).
 * - `fixed` lies in [0, p].
 * - The matrix a is [m][n], row-major.  a[i][j] is what demand j pays at site i.
 * - Every entry is +inf, or finite with +0.0 <= x <= 2^1000.
 * - A NaN, a negative entry, a finite entry above 2^1000 and -0.0 are errors, named by (b, i, j).  The validation tests the sign
 *   bit, because a minimum over +-0.0 would not be a function of the words.
 * - No multiplication occurs anywhere, so nothing can contract.
 * The row.
 * - sel[0 .. p-1]: each entry is -1 (an empty slot) or a site.
 * - No site stands twice.
 * - The slots below `fixed` are not empty and never change.
 * Nearest site.
 * - near(sel, j) is the smallest a[sel[s]][j] over the non-empty slots, or +inf with none.
 * - own(sel, j) is the smallest slot attaining it where it is finite, and -1 otherwise.
 * Cost.  cost(sel) = (uns, sum, max), with uns = 0, sum = +0.0 and max = +0.0 at the start.  Walk j = 0 .. n-1 in order:
 * - If near is +inf, uns += 1.
 * - Otherwise sum = fl(sum + near), and max takes the larger of the two.
 * Key.
 * - Mode 0, "sum": (uns, sum).
 * - Mode 1, "max": (uns, max, sum).
 * - Keys compare lexicographically.  The integer comes first.
 * One sweep.
 * - For every slot o in [fixed, p) and every site i that is not in the row, the candidate is the row with sel[o] = i.
 * - Its key is the key of its cost, computed exactly as above.
 * - The move of the sweep is the candidate with the smallest (key, o, i).
 * - It is applied iff its key is strictly smaller than the row's own key and fewer than max_moves moves were applied.
 * - An empty slot is an ordinary o.  That candidate is an addition.  So the greedy construction from the all-empty row and the
 *   swap search are one rule.
 * Stopping.
 * - Status 0: no candidate was strictly better, or there was no candidate at all (fixed == p, or every site is in the row).
 * - Status 2: a strictly better candidate was found after max_moves moves, with 0 <= max_moves <= 2^20.
 * - Every applied move lowers the key strictly and there are finitely many rows.  So the search ends without the cap.
 * - A call runs at most max_moves + 1 sweeps per start.
 * - A row may end with empty slots, where no addition changes the key.
 * Results per start.
 * - The row.
 * - owner[j] = sel[own(sel, j)], or -1.
 * - value = {sum after, max after, sum before, max before}.
 * - info = {moves, sweeps, uns after, uns before}.
 * pf_place_improve: B starts d_sel int32 [B][p], in and out, over one matrix d_mat [m][n] (shared = 1) or over d_mat [B][m][n]
 * (shared = 0) -> d_owner int32 [B][n] (or NULL), d_value [B][4], d_status [B], d_info int64 [B][4] (or NULL).  One workgroup of
 * 1024 threads per start runs the move loop inside the kernel; LDS holds, per demand, the smallest value over the row with its
 * smallest slot and the second smallest value, so that a candidate's term at j is one minimum; a lane takes a candidate (o, i) --
 * 64 / P sites share a wavefront, P the power of two >= p -- and walks the demands in order; the minimum is one lexicographic
 * reduction over (key, o, i).  One launch per call, whatever B.  The device's rows, owners, values, statuses and infos equal the rule's as 64-bit words, on every run and for every
 * assignment of starts to workgroups.
 * A null handle (-2); m, n or p out of range, `fixed` outside [0, p], a mode outside 0..1, shared outside 0..1, B < 1, max_moves
 * outside [0, 2^20] or a missing required pointer (-1, with a message) is an argument error found on the host before any launch.
 * A bad entry is -1 with a message naming the first (b, i, j).  A bad row is -1 with a message naming the first (b, slot): the
 * first slot that lies outside [-1, m), repeats the site of a smaller slot, or is empty below `fixed`.  Two validation kernels find
 * these, in this order, BEFORE anything is written: after an error no output is touched.  The call is synchronous and ordered on
 * the handle's stream; pf_last_kernel_ms reports the kernels (the validations included). */
#define PF_PLACE_SITES_MAX 1024
#define PF_PLACE_DEMANDS_MAX 4096
#define PF_PLACE_OPEN_MAX 64
int pf_place_improve(pf_handle* h, int32_t mode, int32_t m, int32_t n, int32_t p, int32_t fixed, int32_t B, int32_t shared,
                     const double* d_mat, int32_t max_moves, int32_t* d_sel, int32_t* d_owner, double* d_value,
                     int32_t* d_status, int64_t* d_info);

/* ---- coverage: which p of m sites see or reach the most of n elements, additions, swaps and drops (pathfit.Coverage) -----------
 * 
 * Inputs.
 * - There are m sites, n elements and p slots.
 * - The limits are 1 <= m <= 1 024 (PF_COVER_SITES_MAX), 1 <= n <= 2^20 (PF_COVER_ELEMS_MAX) and 1 <= p <= min(m, 64)
 *   (PF_COVER_OPEN_MAX).
 * - `fixed` lies in [0, p].
 * - W = ceil(n / 64).
 * - Site i has a mask M[i], uint64 [W].  Element j is bit j & 63 of word j >> 6.
 * - A set bit at j >= n is an error, named by (b, i).
 * - An all-zero mask is legal.
 * - Everything is an integer: no result depends on the order of any sum.
 * The row.
 * - sel[0 .. p-1]: each entry is -1 (an empty slot) or a site.
 * - No site stands twice.
 * - The slots below `fixed` are not empty and never change.  This is pf_place_improve's row.
 * Key.
 * - cnt(sel, j) is the number of non-empty slots s with bit j set in M[sel[s]].
 * - cov(sel) is the number of j in [0, n) with cnt(sel, j) > 0.
 * - open(sel) is the number of non-empty slots.
 * - The key is (n - cov, open).  Keys compare lexicographically.
 * One sweep.
 * - For every slot o in [fixed, p) and every site i that is not in the row, the candidate is the row with sel[o] = i.  It is an
 *   addition if slot o is empty and a swap otherwise.
 * - For every non-empty slot o in [fixed, p), the candidate is the row with sel[o] = -1, a drop.  A drop is written as i = m.
 * - The move of the sweep is the candidate with the smallest (key, o, i).
 * - It is applied iff its key is strictly smaller than the row's own key and fewer than max_moves moves were applied.
 * Stopping.
 * - Status 0: no candidate was strictly better, or there was no candidate at all.
 * - Status 2: a strictly better candidate was found after max_moves moves, with 0 <= max_moves <= 2^20.
 * - Every applied move lowers the key strictly and there are finitely many rows.  So the search ends without the cap.
 * - A call runs at most max_moves + 1 sweeps per start.
 * Consequences.
 * - The greedy construction, the swap search and the removal of redundant sites are one rule.
 * - A swap with equal coverage never applies: its key equals the row's.
 * - An addition applies only if it covers something new: otherwise open grows and cov does not.  So a row may end with empty
 *   slots.
 * - A site that has become redundant is dropped: the drop keeps cov and lowers open.
 * - Every empty slot has the same candidates with the same keys, and the smallest o wins the tie.  So the additions of the
 *   smallest empty slot decide.
 * - With p = min(m, 64) and an all-empty start the rule answers "how few sites cover everything that can be covered": it adds
 *   while something new is covered, and swaps and drops afterwards.
 * Results per start.
 * - The row.
 * - covered = the union of the row's masks, uint64 [W].
 * - value = {cov after, open after, cov before, open before}.
 * - info = {moves, sweeps, elements with cnt == 1 after, drops among the moves}.
 * pf_cover_improve: B starts d_sel int32 [B][p], in and out, over one mask set d_mask uint64 [m][W] (shared = 1) or over d_mask
 * [B][m][W] (shared = 0) -> d_covered uint64 [B][W] (or NULL), d_value int64 [B][4], d_status [B], d_info int64 [B][4] (or NULL).
 * One workgroup of 1024 threads per start runs the move loop inside the kernel; per start two planes of W words hold the union
 * and the elements covered exactly once, in LDS up to W = 4 096 and in the handle's scratch above, so that a swap's coverage is
 * sum_w popc((any & ~(once & M[sel o])) | M[i]); a wavefront takes a site, its lanes the words.  One launch per call, whatever B.
 * The device's rows, planes, values, statuses and infos equal the rule's, on every run and for every assignment of starts to
 * workgroups.
 * A null handle (-2); m, n or p out of range, `fixed` outside [0, p], shared outside 0..1, B < 1, max_moves outside [0, 2^20] or a
 * missing required pointer (-1, with a message) is an argument error found on the host before any launch.  A set tail bit is -1
 * with a message naming the first (b, i); a bad row is -1 with a message naming the first (b, slot), as pf_place_improve's.  Two
 * validation kernels find these, in this order, BEFORE anything is written: after an error no output is touched.
 * pf_cover_pack: the masks' builder.  K source rows d_src of leading dimension ld, read at the n cells d_targets (int32 [n] on the
 * device, each in [0, ld)), fill the rows row0 .. row0 + K - 1 of d_mask [.][W].  kind 0: the source is uint8 and the bit is
 * byte != 0 (pf_visibility_field's rows).  kind 1: the source is double and the bit is x <= radius (the fields' rows; +inf and NaN
 * give 0; radius is finite and >= 0).  The tail bits of the last word are 0.  A null handle (-2); a kind outside 0..1, K, n or ld
 * < 1, n above 2^20, a row range that leaves [0, 1 024], a bad radius or a missing pointer (-1, with a message) is found before
 * any launch; a target outside [0, ld) is -1 with a message naming the first, found by a validation kernel before any write.
 * Both calls are synchronous and ordered on the handle's stream; pf_last_kernel_ms reports the kernels (the validations
 * included). */
#define PF_COVER_SITES_MAX 1024
#define PF_COVER_ELEMS_MAX 1048576
#define PF_COVER_OPEN_MAX 64
int pf_cover_pack(pf_handle* h, int32_t kind, int32_t K, int32_t n, const void* d_src, int32_t ld, const int32_t* d_targets,
                  double radius, int32_t row0, uint64_t* d_mask);
int pf_cover_improve(pf_handle* h, int32_t m, int32_t n, int32_t p, int32_t fixed, int32_t B, int32_t shared,
                     const uint64_t* d_mask, int32_t max_moves, int32_t* d_sel, uint64_t* d_covered, int64_t* d_value,
                     int32_t* d_status, int64_t* d_info);

/* ---- the sight graph: exact any-angle shortest paths between cell centres (pathfit.AnyAngle) --------------------------------
 * The yardstick for Euclidean any-angle length: the shortest polyline whose vertices are cell centres and whose
 * segments all pass the smoothing section's visible(a, b, restrict_corner).
 * The nodes.
 * - `nodes` is a host array of M cell ids, strictly increasing, each in [0, R C), 1 <= M <= PF_SIGHT_NODES_MAX.
 * - Everything below speaks of node INDICES 0 .. M - 1, not of cell ids; "smallest" means the smallest node index.
 * The graph.
 * - d_adj is uint64 [M][ld], ld >= W = ceil(M / 64).  Bit j & 63 of word j >> 6 of row i is the pair (i, j).
 * - The bit is set iff visible(nodes[i], nodes[j], restrict_corner) holds and, when max_range_sq >= 0, dr^2 + dc^2 <= max_range_sq.
 * - The diagonal bit (i, i) is the rule's a == b case: set iff the node's cell is free.  It is the node's "usable" flag below.
 * - A node on an obstacle has an all-zero row and column.  The rule is symmetric, and so is the matrix.
 * - The tail bits of word W - 1 are zero.  The words [W, ld) of a row are not written.
 * - The occupancy is the handle's at call time: after pf_update_grid the next pack sees the new map.
 * pf_sight_pack: fills d_adj, one lane per ordered pair, all M^2 pairs.  d_info (or NULL), int64 [4] = {set off-diagonal bits, the
 * largest off-diagonal degree over all M nodes, the smallest node index that attains it, nodes on obstacles}.
 * The labels.
 * - w(i, j) = sqrt((double)(dr^2 + dc^2)), correctly rounded, between the cells of nodes i and j.
 * - set_off and src are host arrays laid out as pf_dist_field_merged's, src holding node indices; here a set may be empty.
 * - A source is usable iff its diagonal bit is set.  d_dist[b][v] = 0 at a usable source of set b.
 * - Elsewhere d_dist[b][v] is the least value, over all walks u0 .. uk = v along set bits from a usable source u0 of set b, of the
 *   left-to-right sum fl(.. fl(fl(0 + w(u0, u1)) + w(u1, u2)) ..), and +inf where there is no such walk (a node on an obstacle, a
 *   set with no usable source).
 * - An edge into v is read from ROW v: bit (v, u).  The matrix must be symmetric, as pf_sight_pack leaves it.
 * - fp64 addition is monotone and every w >= 1, so these are a heap Dijkstra's labels bit for bit, and the unique fixed point of
 *   d[v] = min_u fl(d[u] + w(u, v)): the device relaxes in rounds, in whatever order, and lands on the same words on every run.
 * pf_sight_field: B source sets -> d_dist double [B][M]; d_parent (or NULL) int32 [B][M]; d_info (or NULL) int64 [B][4].
 * - d_parent[b][v] = -1 at a usable source and at a +inf label; else the smallest u with bit (v, u) set, d[u] < d[v] and
 *   fl(d[u] + w(u, v)) == d[v].  A field-only rule, as pf_dist_field_parents has one.
 * - d_info[b] = {finite labels, nodes with label 0 (the distinct usable sources), the smallest node index that holds the largest
 *   finite label or -1, 0}.
 * - One workgroup of 1 024 threads per set, the round loop inside the kernel; the labels of a set live in LDS.
 * pf_sight_field_work: out4 = {the most rounds a set took, the rounds of all sets, candidate sums formed, labels lowered} of the
 * last pf_sight_field call on the handle.  For the probe; the last two depend on the order the device happened to take.
 * pf_sight_paths: n queries.  Query i chases d_parent from node d_target[i] in set d_set[i] (d_set NULL: set 0).
 * - d_way int32 [n][way_cap]: the waypoints' CELL ids source -> target, or target -> source when reverse != 0; d_way_len their number.
 * - d_stats (or NULL) double [n][2] = {the left-to-right sum of the segments' lengths taken source -> target, the turns as
 *   pf_smooth_batch counts them}; both 0 unless the status is 0.  With pf_sight_field's parents the sum is d_dist's word.
 * - d_status: 0 ok; 1 = a set outside [0, B) or a target outside [0, M); 2 = the label is +inf; 3 = more waypoints than way_cap;
 *   4 = parents that are not pf_sight_field's: an index outside [-1, M), a chain of more than M nodes or one that ends at a node
 *   whose label is not 0.  Every walk ends within M steps.  The length is 0 and the row untouched unless the status is 0.
 * All three: a null handle (-2).  M out of range, a node outside the grid or not above its predecessor (the message names the first
 * such index), ld < W, max_range_sq < -1, B < 1, offsets that do not start at 0 or that decrease, a source outside [0, M) (the
 * message names the first index), n < 0, way_cap < 1 or a missing required pointer (-1, with a message) is found on the host before
 * any launch.  pf_sight_paths with n == 0 returns 0 and launches nothing.  Synchronous, ordered on the handle's stream;
 * pf_last_kernel_ms reports the kernels. */
#define PF_SIGHT_NODES_MAX 16384
int pf_sight_pack(pf_handle* h, int32_t restrict_corner, int32_t max_range_sq, int32_t M, const int32_t* nodes, uint64_t* d_adj,
                  int32_t ld, int64_t* d_info);
int pf_sight_field(pf_handle* h, int32_t M, const int32_t* nodes, const uint64_t* d_adj, int32_t ld, int32_t B,
                   const int32_t* set_off, const int32_t* src, double* d_dist, int32_t* d_parent, int64_t* d_info);
int pf_sight_field_work(pf_handle* h, int64_t* out4);
int pf_sight_paths(pf_handle* h, int32_t M, const int32_t* nodes, int32_t B, const double* d_dist, const int32_t* d_parent,
                   int32_t n, const int32_t* d_set, const int32_t* d_target, int32_t reverse, int32_t way_cap, int32_t* d_way,
                   int32_t* d_way_len, double* d_stats, int32_t* d_status);

/* Tuning knobs (results never change): "tour_tables" the most Held-Karp tables pf_tour_solve keeps in flight in HBM (default 0:
 * as many as fit 256 MiB); "components_phases" 0/1 pf_components records a HIP event after each phase
 * (pf_components_phase_ms; default 0); "maaco_pack8_min" ants per batch from which eight ants share a wavefront
 * (default 2048); "maaco_load_ahead" the packed walk kernel's load-ahead form (all of a step's loads issued together plus touches of the
 * records two steps ahead): -1 (default) for batches of at most one wavefront per SIMD, 0 never, 1 always;
 * "mpa_prune" 0/1 exact bound pruning of MPA rebuilds (default 1); "mpa_bounds_device" 0/1 the bound tables of pf_mpa_setup /
 * pf_mpa_batch_create come from one pf_dist_field_batch launch instead of one host Dijkstra per distinct cell (default 0: the
 * launch serialises on corridor maps; the tables are bit-identical either way); "mpa_lookahead" how many iterations one MPA sweep may cover
 * after an iteration that accepted nothing (pf_mpa_iter_ahead; at most 16, 0 = off: exactly pf_mpa_iter_batch's
 * launches; default 8, or the environment's PF_MPA_LOOKAHEAD; < 0 restores the default); test hook "mpa_lookahead_always" 0/1: look ahead after any iteration, so that levels do go stale;
 * "astar_settle" 0/1 closed-set searches (AStarSolver
 * / Dijkstra / GA / PSO decodes) try the parallel label-settling engine first: -1 (default) the Dijkstra variant
 * always (it is always certified) and the A* searches of the decodes at the head of a batch's longest-first queue
 * ("astar_settle_top", per mille of the batch, default 0 since r03; a decode is a chain of W + 1 searches, so a fallback costs
 * one link) and -- "astar_settle_tail", per mille of the search slots, default 400 -- every decode search that starts once
 * the batch's unfinished agents no longer fill that share of the chip (the long chains the batch ends on, on an idle chip); 1 every A* search too (exact -- certified or handed back to the sequential loop -- but slower
 * on batches of single searches); 0 never (the sequential loop's pop / push counters are the reference's).  Test hook: "astar_step_cap" > 0
 * lowers the connectors' step cap below the reference's 3RC / 2RC (astar.py:58, MPA.py:118) so that the cap path
 * (PF_ST_STEP_CAP) can be exercised; 0 restores the reference's value.  "mpa_doubt_log_e15" / "mpa_doubt_round_e15":
 * margins (in 1e-15; < 0 = default) inside which an MPA proposal is handed to the host's libm (tests widen them to
 * force that route).  Test hooks "astar_slot_tag" (24 bit) / "astar_slot_avoid_epoch" (14 bit): before the next search launch
 * (A* batch, decode, MPA sweep) every search slot's solve tag / avoid epoch is moved FORWARD to the value, so that the wipes
 * that precede a wrap (avoid epoch 0x3FF0, tag 0xFFFFFF - 2 * 0x8000) can be reached in a test; one-shot (later launches carry
 * on from there), < 0 withdraws a value not yet applied, and that launch fails with a message if the value lies below a
 * slot's current one (stale stamps would look current).  Like every option the pending value is process-wide, not per handle:
 * it goes to the slots of whichever handle launches a search next, so a test sets it right in front of the launch it is meant
 * for.  pf_selftest_slot_state reads the counters back. */
int pf_set_option(pf_handle* h, const char* name, int64_t value);

/* ---- device self-tests (used by tests/ to pin device arithmetic) ----- */
/* out[i] = device sqrt((double)in[i]) -- must equal libm sqrt bit for bit
 * (heuristic astar.py:90 / helper.py:12). */
int pf_selftest_sqrt(pf_handle* h, int32_t n, const int64_t* d_in, double* d_out);
/* device keyed RNG + CPython derivations for key (seed,dom,it,agent):
 * d_u64[8] next64; d_f64[0..8) random(), [8..28) normalvariate (16 x (0,1),
 * 4 x (0,0.7)), [28..36) uniform(0,2pi); d_i64[0..24) randint as in
 * oracle/capture_golden.py cap_rng, [24..34) randbelow(n) for the same n
 * list, [34..37) draw counters after the randint / normal / choice runs. */
int pf_selftest_rng(pf_handle* h, uint64_t seed, uint64_t dom, uint64_t it, uint64_t agent, uint64_t* d_u64,
                    double* d_f64, int64_t* d_i64);

/* ---- iteration control in HBM -------------------------------------------------------------------
 * list.sort(key=fitness) (MPA.py:321,333,412; ga_solver.py:209): d_order holds the list (position -> id); it is
 * re-ordered by a STABLE device sort on key[pos] = d_vals[d_order[pos] * stride + offset].  Stream ordered. */
int pf_sort_order_by_key(pf_handle* h, int32_t n, const double* d_vals, int32_t stride, int32_t offset, int32_t* d_order);
/* population[0] after the sort (MPA.py:334, :413; ga_solver.py:210): out2 = {id at the head of d_order, its key
 * d_vals[id * stride + offset]} in one 16-byte copy */
int pf_sorted_head(pf_handle* h, const int32_t* d_order, const double* d_vals, int32_t stride, int32_t offset, double* out2);
/* d_dst[i] = d_src[i * stride + offset] (a stats column packed for an all_gather) */
int pf_gather_col(pf_handle* h, int32_t n, const double* d_src, int32_t stride, int32_t offset, double* d_dst);
/* d_out[i] = d_a[i] + sign * d_b[i] (sign = +1 / -1; one IEEE operation per element, in place allowed): the non-strict MAACO
 * exchange (all_reduce of per-rank pheromone deltas; no reference counterpart) forms and applies its deltas with it. */
int pf_vec_add_f64(pf_handle* h, int32_t n, const double* d_a, const double* d_b, double sign, double* d_out);
/* The elite of an MPA iteration (MPA.py:334, population[0] after the sort) lives in a library-owned buffer: cells
 * [R*C] int32, length int32, stats double[5].  pf_mpa_pick_elite copies the row of predator d_order[0] - first_id of
 * this rank's store into it; a sharded run broadcasts the three pieces from the owner instead.  Passing
 * elite_len = -1 to pf_mpa_iter_batch makes the sweep read the length from that buffer (the host never learns it). */
int pf_mpa_elite_buf(pf_handle* h, void** d_cells, void** d_len, void** d_stats);
int pf_mpa_pick_elite(pf_handle* h, int32_t path_cap, const int32_t* d_pop_cells, const int32_t* d_pop_len,
                      const double* d_pop_stats, const int32_t* d_order, int32_t first_id);
/* positions (in the global fitness order d_gorder[N] of ids) and storage slots of the predators with ids in [lo, hi),
 * in position order: the d_gidx / d_slot arrays of pf_mpa_iter_batch for a rank that stores ids [lo, hi) */
int pf_mpa_local_view(pf_handle* h, int32_t N, const int32_t* d_gorder, int32_t lo, int32_t hi, int32_t* d_gidx, int32_t* d_slot);

/* ---- one GA generation in HBM (ga_solver.py:178-213) -----------------------------------------------------------------
 * The population is stored by storage id (= child index of the generation that made the individual): chromosomes
 * d_chrom_all [N][W] cells, fitness d_fit_all [N]; d_gorder [N] is the fitness-sorted list (position -> storage id).
 * pf_ga_select_dev: GASolver._selection for all N slots (one sequential stream per generation, replayed by one
 *   device thread) -> d_psid[s] = storage id of the parent chosen for slot s.
 * pf_ga_breed_dev: _crossover + _mutate for the children with index in [child0, child0 + nchild) (thread per pair,
 *   stream (seed, DOM_GA, gen, pair)) -> d_out [nchild][W].
 * pf_ga_assemble_dev: new individual i = child i if it decoded (d_kid_len > 0) else its fallback parent d_psid[lo + i]
 *   (ga_solver.py:204-205); a fallback parent's path row is copied when this rank stores it (ids [old_lo, old_hi)),
 *   else the row is marked absent (length -1).  All stream ordered, no host copies. */
int pf_ga_select_dev(pf_handle* h, uint64_t seed, int32_t gen, int32_t n, int32_t tournament_size, const double* d_fit_all,
                     const int32_t* d_gorder, int32_t* d_psid);
int pf_ga_breed_dev(pf_handle* h, uint64_t seed, int32_t gen, int32_t N, int32_t W, double crossover_rate, double mutation_rate,
                    const int32_t* d_chrom_all, const int32_t* d_psid, int32_t child0, int32_t nchild, int32_t* d_out);
int pf_ga_assemble_dev(pf_handle* h, int32_t n_loc, int32_t W, int32_t path_cap, int32_t lo, const int32_t* d_kid_len,
                       const int32_t* d_kid_chrom, const double* d_kid_stats, const int32_t* d_kid_cells, const int32_t* d_psid,
                       const int32_t* d_chrom_old, const double* d_stats_old, const int32_t* d_cells_old, const int32_t* d_len_old,
                       int32_t old_lo, int32_t old_hi, int32_t* d_chrom_new, double* d_stats_new, int32_t* d_cells_new,
                       int32_t* d_len_new);

/* ---- K independent GA populations in one batched generation (pathfit.GABatch) -----------------------------------------
 * Population k has its own seed d_seeds[k] (uint64[K] in HBM) and, through pf_decode_batch_multi, its own start and target;
 * the K populations share the grid, N, W and the rates.  Layout of every buffer: population k owns rows [k N, (k + 1) N);
 * the ids inside d_gorder / d_psid are LOCAL (0 .. N - 1).  Population k computes exactly what the solo calls compute on its
 * rows with seed d_seeds[k].  The entries are stateless (the caller owns every buffer; scratch is the handle's), stream
 * ordered, and make no host copies except pf_best_rows_seg.
 * pf_ga_select_batch: GASolver._selection (ga_solver.py:136-142, :181) for all K populations: K replays of the streams
 *   (d_seeds[k], DOM_GA_SELECT, gen, 0) side by side, one wavefront each (pf_ga_select_dev for every k).
 * pf_ga_breed_batch: _crossover + _mutate (ga_solver.py:144-160, :186-194) for all N children of all K populations, thread per
 *   (population, pair), stream (d_seeds[k], DOM_GA, gen, pair) -> d_out [K N][W] (pf_ga_breed_dev with child0 = 0, nchild = N).
 * pf_ga_assemble_batch: ga_solver.py:198-205 for all K N children: child or fallback parent d_psid[k N + i] of the
 *   population's own old rows (pf_ga_assemble_dev with lo = old_lo = 0, old_hi = N: no row is ever absent).
 * pf_sort_order_by_key_seg: K times list.sort(key=fitness) (ga_solver.py:209): segment k of d_order [K n] (position -> LOCAL
 *   id) is re-ordered by a STABLE sort on d_vals[(k n + id) * stride + offset]; no segment sees another's keys.
 * pf_best_rows_seg: population[0] of every population after the sort (ga_solver.py:210-213) in one copy: out[6 k ...] =
 *   {local id at the head of segment k, the five doubles d_stats[(k N + id) * 5 ...]}. */
int pf_ga_select_batch(pf_handle* h, const uint64_t* d_seeds, int32_t gen, int32_t K, int32_t N, int32_t tournament_size,
                       const double* d_fit_all, const int32_t* d_gorder, int32_t* d_psid);
int pf_ga_breed_batch(pf_handle* h, const uint64_t* d_seeds, int32_t gen, int32_t K, int32_t N, int32_t W, double crossover_rate,
                      double mutation_rate, const int32_t* d_chrom_all, const int32_t* d_psid, int32_t* d_out);
int pf_ga_assemble_batch(pf_handle* h, int32_t K, int32_t N, int32_t W, int32_t path_cap, const int32_t* d_kid_len,
                         const int32_t* d_kid_chrom, const double* d_kid_stats, const int32_t* d_kid_cells, const int32_t* d_psid,
                         const int32_t* d_chrom_old, const double* d_stats_old, const int32_t* d_cells_old, const int32_t* d_len_old,
                         int32_t* d_chrom_new, double* d_stats_new, int32_t* d_cells_new, int32_t* d_len_new);
int pf_sort_order_by_key_seg(pf_handle* h, int32_t K, int32_t n, const double* d_vals, int32_t stride, int32_t offset, int32_t* d_order);
int pf_best_rows_seg(pf_handle* h, int32_t K, int32_t N, const double* d_stats, const int32_t* d_order, double* out);

/* ---- K independent PSO swarms in one batched sweep (pathfit.PSOBatch) --------------------------------------------------
 * Swarm k has its own seed d_seeds[k] (uint64[K] in HBM), start cell d_starts[k] and target cell d_targets[k]; the K swarms
 * share the grid, N, W and the coefficients.  Layout: particle a (LOCAL, 0 .. N - 1) of swarm k is row k N + a of d_pos /
 * d_vel / d_pbest [K N][W][2], d_pbest_fit / d_len / d_pb_len [K N], d_stats [K N][5], d_cells / d_pb_cells [K N][path_cap];
 * swarm k owns row k of d_gbest [K][W][2], d_gbest_stats [K][5], d_gbest_path [K][path_cap + 1] ([0] = length) and d_gfit [K].
 * A round of the asynchronous sweep evaluates the particles [cur[k], N) of every swarm, cur[k] being its first particle that
 * is not final yet; these segments back to back are the round's n ITEMS.  d_tab, int32 [2 K + 1], is the round's table:
 * off[0 .. K] (off[k] = first item of swarm k, off[K] = n), then cur[0 .. K).  The d_s_* buffers are STAGING rows, one per
 * item ([K N] rows at most): the new position and velocity, the item's start and target cell, its row k N + a, and -- written
 * by pf_decode_batch_multi(n, W, wp_pos = d_s_pos, d_s_start, d_s_target, ...) between the update and the scan -- its path
 * row, length, status and stats.  Swarm k computes exactly what the solo calls compute on its rows with seed d_seeds[k].  The
 * entries are stateless (the caller owns every buffer) and stream ordered; only pf_pso_scan_batch copies to the host.
 * pf_pso_update_batch: pso.py:186-202 for every item, stream (d_seeds[k], DOM_PSO, iter, a) with waypoint d at draw 4 d and
 *   gbest row k (pf_pso_update per swarm).  Reads the swarms' rows, writes staging only: an item that turns out not to be final
 *   leaves nothing to roll back.
 * pf_pso_scan_batch: the decision of pso.py:216-229 per swarm (pf_pso_scan on its segment with gbest_fit = d_gfit[k]): d_rec[k]
 *   = {int32 index INSIDE the segment of the first item that is feasible with fitness below its own pbest and below d_gfit[k]
 *   -- sync_mode != 0: of the first item holding the smallest such fitness --, or -1; int32 number of items with status
 *   PF_ST_OVERFLOW; double its fitness or inf}, 16 bytes; the K records are copied to out in ONE device-to-host copy.
 * pf_pso_commit_batch: the writes of pso.py:216-229.  Final items are, asynchronously, those at or before their swarm's
 *   improver (the whole segment if d_rec[k] has none), synchronously all: their staging rows become the particle's position,
 *   velocity, path row, length and stats; pso.py:216-220 (strict < against the OLD pbest: position, fitness, path row);
 *   the improver: pso.py:222-229 into gbest row k, d_gbest_stats, d_gbest_path (length first) and d_gfit[k].  Nothing is
 *   written for the other items. */
int pf_pso_update_batch(pf_handle* h, int32_t n, int32_t K, int32_t N, int32_t W, double w, double c1, double c2, double max_vel, uint64_t iter,
                        const uint64_t* d_seeds, const int32_t* d_tab, const int32_t* d_starts, const int32_t* d_targets, const double* d_pos,
                        const double* d_vel, const double* d_pbest, const double* d_gbest, double* d_s_pos, double* d_s_vel, int32_t* d_s_start,
                        int32_t* d_s_target, int32_t* d_s_row);
int pf_pso_scan_batch(pf_handle* h, int32_t K, int32_t N, int32_t sync_mode, const int32_t* d_tab, const double* d_s_stats, const int32_t* d_s_len,
                      const int32_t* d_s_status, const double* d_pbest_fit, const double* d_gfit, void* d_rec, void* out);
int pf_pso_commit_batch(pf_handle* h, int32_t n, int32_t K, int32_t N, int32_t W, int32_t path_cap, int32_t sync_mode, const int32_t* d_tab,
                        const void* d_rec, const int32_t* d_s_row, const double* d_s_pos, const double* d_s_vel, const double* d_s_stats,
                        const int32_t* d_s_len, const int32_t* d_s_cells, double* d_pos, double* d_vel, double* d_stats, int32_t* d_len,
                        int32_t* d_cells, double* d_pbest, double* d_pbest_fit, int32_t* d_pb_cells, int32_t* d_pb_len, double* d_gbest,
                        double* d_gbest_stats, int32_t* d_gbest_path, double* d_gfit);

/* MAACO.py:306-311 in two steps (the multi-GPU fold works on row chunks): _begin marks the cells of the successful
 * ants and computes Q / L per ant, _cells adds the deposits of cells [cell0, cell1) in ant order.  pf_maaco_deposit =
 * _begin + _cells(0, R*C).  All stream ordered. */
int pf_maaco_deposit_begin(pf_handle* h, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len,
                           const double* d_plen);
int pf_maaco_deposit_cells(pf_handle* h, int32_t cell0, int32_t cell1);
/* MAACO.py:343-349 (best ant of an iteration: length, then turns within 1e-9) over device columns of n ants;
 * out3 = {best_len, best_turns, best_idx} (-1: no ant arrived).  One 24-byte device-to-host copy. */
int pf_maaco_best_dev(pf_handle* h, int32_t n, const double* d_plen, const int32_t* d_turns, double* out3);

/* ---- multi-GPU exchange: RCCL over xGMI, bound directly (no reference counterpart) -------------
 * One process per GPU.  librccl is opened on first use.  pf_comm_unique_id (rank 0) produces the 128-byte id the
 * launcher ships to the other ranks (a file, an env var, torch.distributed's store); pf_comm_init joins the
 * communicator on the handle's device.  Every collective below is ENQUEUED on the handle's stream, in order with the
 * kernels: no host synchronisation, device pointers only.  Sizes are bytes.  The population solvers need exactly:
 *   all_gather   per-agent (length, turns) / fitness columns and GA chromosomes          (C2, C3)
 *   broadcast    the winner's / elite's path row and stats from its owner                 (C2)
 *   send/recv    the pheromone matrix chunks of the ordered MAACO fold, rank k-1 -> k    (C1, MAACO.py:306-311)
 *   all_reduce   the non-strict MAACO delta sum, timing maxima                           */
int pf_comm_unique_id(void* id128);
int pf_comm_init(pf_handle* h, int32_t rank, int32_t world, const void* id128);
int pf_comm_destroy(pf_handle* h);
int pf_comm_rank(pf_handle* h);
int pf_comm_world(pf_handle* h);
int pf_comm_all_gather(pf_handle* h, const void* d_send, void* d_recv, int64_t bytes_per_rank);
int pf_comm_broadcast(pf_handle* h, void* d_buf, int64_t bytes, int32_t root);
int pf_comm_all_reduce_f64(pf_handle* h, double* d_buf, int64_t count, int32_t op /* 0 sum, 1 min, 2 max */);
int pf_comm_send(pf_handle* h, const void* d_buf, int64_t bytes, int32_t peer);
int pf_comm_recv(pf_handle* h, void* d_buf, int64_t bytes, int32_t peer);
/* one ring step as a single group: send to `to` (skip if < 0) and receive from `from` (skip if < 0) */
int pf_comm_sendrecv(pf_handle* h, const void* d_send, int64_t send_bytes, int32_t to, void* d_recv, int64_t recv_bytes,
                     int32_t from);

/* pbest -> gbest scan of one evaluated batch of n particles (pso.py:216-229): *idx_out = the first particle that
 * improves the gbest (feasible, fitness below its pbest AND below gbest_fit), or with sync_mode != 0 the first particle
 * with the smallest such fitness; -1 if none.  *fit_out its fitness, *overflow_out the number of particles whose
 * status is PF_ST_OVERFLOW.  One 16-byte device-to-host copy. */
int pf_pso_scan(pf_handle* h, int32_t n, const double* d_stats, const int32_t* d_len, const int32_t* d_status,
                const double* d_pbest_fit, double gbest_fit, int32_t sync_mode, int32_t* idx_out, double* fit_out,
                int32_t* overflow_out);
/* Device-to-host copies made through this handle since pf_create: copies of at most 128 bytes, larger ones, and the
 * bytes of the larger ones (the solver loops keep populations in HBM: SURVEY.md 8 f1/f2). */
int pf_d2h_counts(pf_handle* h, int64_t* small_copies, int64_t* bulk_copies, int64_t* bulk_bytes);

/* Spans: HIP-event timed stretches of work on the handle's stream (kernels, pf_comm_* collectives), recorded without
 * synchronising.  pf_span_begin / pf_span_end bracket one stretch (not nested); pf_span_total synchronises the stream and
 * returns the summed duration (ms) and the number of spans since the last reset.  Measurement only (bench.py times the
 * per-iteration exchange of the sharded solvers with it: SURVEY.md 8e); no reference counterpart. */
int pf_span_begin(pf_handle* h);
int pf_span_end(pf_handle* h);
int pf_span_total(pf_handle* h, double* ms_out, int64_t* count_out, int32_t reset);

/* The epoch counters of search slot `slot` (0 <= slot < the handle's slot count; workgroup b of a search launch owns slot b, so
 * a batch of one search runs on slot 0): out3 = {24-bit solve tag, 14-bit avoid epoch, label epoch of the parallel settling
 * engine (-1: the engine has no scratch on this handle)}.  The slots exist from the first search launch on. */
int pf_selftest_slot_state(pf_handle* h, int32_t slot, int64_t* out3);

/* Branch counters of the A* open list (pf_astar_sw.h, OP_*: 21 of them, in that order), summed over every search of this process
 * since the last reset; the first n are copied to out, the rest of out[0..n) is zeroed; reset != 0 clears them.  They exist only in
 * the diagnostic builds compiled with -DPF_OPEN_PATHS (the stress variants of build.py): any other build zeroes out, sets the
 * handle's error text to "not compiled in" and returns 1.  Synchronises the device. */
int pf_selftest_open_paths(pf_handle* h, int64_t* out, int32_t n, int32_t reset);

/* The same for the branches of the parallel closed-set engine (pf_settle.h, ST_*: 21 of them, in that order): the contract of
 * pf_selftest_open_paths, a device array of its own, and the same -DPF_OPEN_PATHS builds. */
int pf_selftest_settle_paths(pf_handle* h, int64_t* out, int32_t n, int32_t reset);

/* Target-cell proposals of MPA._get_levy_target_node / _get_brownian_target_node (MPA.py:250-282) for n keyed streams
 * (seed, DOM_MPA, 0, i) from cells d_cur[i] (and elite cells d_elite[i], < 0 = None): the device arithmetic, with the
 * proposals whose accept test / rounding lies within the libm-disagreement margin recomputed by the host's glibc
 * exactly as the MPA sweeps do.  *n_doubt = how many took that route. */
int pf_selftest_mpa_targets(pf_handle* h, uint64_t seed, int32_t n, int32_t is_levy, double beta, double sigma,
                            double scale, const int32_t* d_cur, const int32_t* d_elite, int32_t* d_out, int64_t* n_doubt);
/* proposals the host had to confirm since pf_create (expected: 0) */
long long pf_mpa_doubts_resolved(pf_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* PATHFIT_H */
