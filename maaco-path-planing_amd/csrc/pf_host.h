// pf_host.h -- what the translation units of libpathfit.so share on the host: the handle, the error helpers and the few
// functions one unit calls in the other.  pathfit.hip holds the solvers and defines fail / failmsg and the
// handle's life cycle; pathfit_fields.hip holds the field family.  The solvers' own types appear here by name only.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/pathfit.h"
#include "pf_device.h"

#define PF_INTERNAL __attribute__((visibility("hidden")))   /* shared between the units, not exported by the library */

struct DevCounters;
struct MpaAhead;
struct pf_maaco_batch;
struct pf_mpa_batch;

struct pf_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  int R = 0, C = 0, RC = 0;
  uint8_t *d_occ = nullptr, *d_mm_r1 = nullptr, *d_mm_r0 = nullptr, *d_mm_r1_nd = nullptr, *d_mm_r0_nd = nullptr,
          *d_d2near = nullptr;
  std::vector<uint8_t> h_occ;
  int* d_comp[4] = {nullptr, nullptr, nullptr, nullptr};   // component labels per move-mask policy (lazy)
  int nslots = 0;
  int rec_policy = -1;   // which move-mask variant the search records currently carry
  pf::Rec* d_rec = nullptr;
  char* d_tier2 = nullptr;
  uint32_t* d_slot_state = nullptr;
  int* d_work = nullptr;
  DevCounters* d_cnt = nullptr;
  pf_counters last = {};
  double* d_pen = nullptr;
  double pen_min_safe = -1.0;
  int* d_d2wide = nullptr; int wide_W = 0; double* d_penw = nullptr; int penw_n = 0; double penw_min_safe = -1.0;   // min_safe_distance > 15.9
  int edt_radius = 7;      // radius of the obstacle-distance window d2near was built with
  double obst_frac = -1.0; // share of obstacle cells (lazy; picks the plateau kernels on open maps)
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  float last_ms = 0.f;
  std::string err;
  // MAACO
  bool maaco_ready = false;
  pf_maaco_params mp = {};
  double *d_tau = nullptr, *d_taua = nullptr, *d_eta = nullptr, *d_dep = nullptr, *d_tep = nullptr;
  bool bits_clean = false;            // the visit-bit matrix is all zero (k_tau_deposit leaves it so)
  int marks_n = 0; const int* marks_cells = nullptr;   // the last walk batch marked its own deposits (for these n ants / this path buffer)
  double* d_mstate = nullptr;         // pf_maaco_iterate's 13 doubles
  double* h_mstate = nullptr; double* h_mstate_dev = nullptr;   // ... mirrored by the device into pinned host memory (no copy is enqueued)
  int* d_best_row = nullptr; int best_row_cap = 0;   // the overall best ant's path row, [0] = length (pf_maaco_iterate / pf_maaco_best_path)
  char* d_mctl = nullptr;             // pf_maaco_iterate's own {work counter @0, DevCounters @16}: zeroed by k_maaco_best_take for the next walk
  bool mctl_clean = false;
  unsigned* d_visit = nullptr; unsigned* d_visit_epoch = nullptr; int maaco_slots = 0; int maaco_cus = 256;
  unsigned long long* d_bits = nullptr; size_t bits_words = 0; int dep_cap = 0;
  uint8_t* d_flag = nullptr;          // chunk flags of d_bits: [(RC + 63) / 64][bits_words] bytes (MaacoArgs::flag)
  std::vector<pf_maaco_batch*> maaco_batches;   // pf_maaco_batch_create's objects (freed by pf_destroy, invalidated by pf_update_grid)
  std::vector<pf_mpa_batch*> mpa_batches;       // pf_mpa_batch_create's, likewise
  // MPA
  bool mpa_ready = false;
  pf_mpa_params mpp = {};
  pf_score_params mps = {};
  int* d_tmp = nullptr; int tmp_cap = 0;
  double* d_elite_stats = nullptr;
  int* d_init_cells = nullptr; int init_len = 0; int init_cap = 0; double* d_init_stats = nullptr;
  double* d_ds = nullptr; double* d_dt = nullptr;   // static shortest distances from the start / to the target (pruning bounds)
  float* d_est = nullptr; int* d_queue = nullptr; int est_cap = 0;   // work estimates and the longest-first queue of a batch
  void* d_jobs = nullptr; void* d_jres = nullptr; int job_cap = 0;   // the sweep's search jobs / results (k_mpa_plan -> k_mpa_search -> k_mpa_finish)
  int2* d_prop = nullptr; int* d_doubt = nullptr; int prop_cap = 0;   // MPA proposals {idx, target cell}; doubt list [0] = count, [1..] = predators
  long long doubts_resolved = 0;
  void* d_scan = nullptr; void* d_scan3 = nullptr;   // results of the small device scans
  unsigned long long* d_okey = nullptr; int* d_opay = nullptr; unsigned* d_orank = nullptr; int okey_cap = 0;   // rank_sort scratch: key images, payloads, ranks
  int* d_elite_cells = nullptr; int* d_elite_len = nullptr;   // the elite of the iteration (MPA.py:334), device resident
  int* d_ga_pool = nullptr; int ga_pool_cap = 0;              // random.sample's pool copy (small populations; K of them for a batch)
  double* d_seg_rows = nullptr; int seg_rows_cap = 0;         // pf_best_rows_seg: [K][6]
  unsigned long long* d_st_lab = nullptr; int* d_st_touched = nullptr; unsigned char* d_st_par = nullptr; unsigned* d_st_epoch = nullptr;   // pf_settle.h scratch
  int dep_words = 0; long long dep_done = 0;   // MAACO deposit in progress: words of the bit matrix, cells already folded
  ncclComm_t comm = nullptr; int comm_rank = 0, comm_world = 1;   // RCCL communicator over xGMI (pf_comm_init); collectives run on `stream`
  std::vector<hipEvent_t> span_ev; int span_n = 0; bool span_open = false; double span_ms = 0.0; long long span_cnt = 0;   // pf_span_*: HIP-event timed spans on `stream`
  long long d2h_small = 0, d2h_bulk = 0, d2h_bulk_bytes = 0;   // device-to-host copies the library made (f1/f2 accounting): <= 128 B / larger
  MpaAhead* ahead = nullptr;          // pf_mpa_iter_ahead: level buffers and the levels still to be taken (end of pathfit.hip)
  // the field family's scratch (pathfit_fields.hip; freed by pf_destroy)
  int* d_df_lists = nullptr; int df_slots = 0; int* d_df_ctl = nullptr; size_t df_ctl_bytes = 0; int df_cus = 0;   // distance fields: [slots][3][RC] rolling lists; {error word, off[B + 1], ids}
  int* d_cc = nullptr;                                                // pf_components: parent, rank and size words [3][RC], block counts, control block (first use)
  hipEvent_t cc_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; float cc_ms[5] = {0, 0, 0, 0, 0};   // ... its phase spans ("components_phases")
  int* d_clear = nullptr;                                             // pf_clearance_field: control block, envelope stacks [RC] int2, row offsets [RC], column flags [C] (first use)
  char* d_widest = nullptr; size_t widest_bytes = 0; long long widest_work[4] = {0, 0, 0, 0};   // pf_clearance_widest: counters, info words, the sets, tile queues and flags (first use, grown on demand); the last call's work
  long long cost_work[4] = {0, 0, 0, 0};                              // pf_cost_field / pf_cost_field_repair: the last call's work (their scratch is d_widest's block: nothing in it outlives a call)
  long long turn_work[4] = {0, 0, 0, 0};                              // pf_turn_field / pf_turn_field_repair: likewise (pf_spacetime_field keeps its static bit plane and, in the HBM form, its live planes in the same block)
  long long sight_work[4] = {0, 0, 0, 0};                             // pf_sight_field: the last call's work (its scratch is the distance fields' control block: nothing in it outlives a call)
};

PF_INTERNAL int fail(pf_handle* h, const char* what, hipError_t e);   // -> -1, the message on the handle
PF_INTERNAL int failmsg(pf_handle* h, const std::string& m);          // -> -2, likewise
#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(h, #call, e_); } while (0)

// the move masks of a policy (helper order; built by pf_create / pf_update_grid)
inline const uint8_t* move_mask(const pf_handle* h, int allow_diag, int restrict_corner) {
  return allow_diag ? (restrict_corner ? h->d_mm_r1 : h->d_mm_r0) : (restrict_corner ? h->d_mm_r1_nd : h->d_mm_r0_nd);
}

PF_INTERNAL extern bool g_cc_phases;   // pf_components records one HIP event per phase (pf_set_option "components_phases": the probe's spans)
PF_INTERNAL extern long long g_tour_tables;   // pf_tour_solve: the most tables in flight in HBM (pf_set_option "tour_tables"; 0: sized from 256 MiB)

// K single-source distance fields -> rows d_out[k][RC] for the K host cells src[k] (pathfit_fields.hip); `who` names the caller
// in the messages.  The MPA bound tables are built with it ("mpa_bounds_device").
PF_INTERNAL int dist_field_run(pf_handle* h, const char* who, int allow_diag, int restrict_corner, int K, const int32_t* src, double* d_out, int64_t* d_info);
