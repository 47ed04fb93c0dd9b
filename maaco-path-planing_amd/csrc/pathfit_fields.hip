// pathfit_fields.hip -- the field family of libpathfit.so (distance fields, routing trees, nearest-source fields, smoothing,
// connected components, clearance, widest paths, cost fields, turn fields, visibility fields, space-time fields, the sight graph)
// and the planners over it (tours, assignments, the tour search, fleet routes, placement, coverage).  A translation unit, and so a device code
// object, of its own: it shares the handle and the error helpers with pathfit.hip (pf_host.h) and none of the
// solvers' device code.
#include <algorithm>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "pf_host.h"

using namespace pf;

bool g_cc_phases = false;

// ---- what the entry points below say once -----------------------------------------------------------------------------------
// One timed stretch of work on the handle's stream: ev0, whatever `enqueue` puts on the stream (it may return a nonzero code
// of its own), ev1, the error word at d_err where the kernels keep one, synchronise -> last_ms.  timed_end is the second half,
// for a call that records ev0 itself and has reasons to leave between the two.
static int timed_end(pf_handle* h, const int* d_err = nullptr, int* err = nullptr) {
  CK(hipGetLastError());
  CK(hipEventRecord(h->ev1, h->stream));
  if (d_err) CK(hipMemcpyAsync(err, d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  CK(hipStreamSynchronize(h->stream));
  CK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  if (d_err) h->d2h_small += 1;
  return 0;
}

template <typename F>
static int timed(pf_handle* h, F&& enqueue, const int* d_err = nullptr, int* err = nullptr) {
  CK(hipEventRecord(h->ev0, h->stream));
  if constexpr (std::is_void<decltype(enqueue())>::value) enqueue();
  else if (const int rc = enqueue()) return rc;
  return timed_end(h, d_err, err);
}

// Scratch memory: allocated on first use; where `have` counts the bytes p holds, replaced when a call needs more.
// The message: "<who>: no device memory for <what>", with the size in MiB where mib is set.
template <typename T>
static int scratch(pf_handle* h, const std::string& who, T*& p, size_t* have, size_t bytes, const char* what, bool mib) {
  if (p && (!have || bytes <= *have)) return 0;
  if (p) { CK(hipStreamSynchronize(h->stream)); (void)hipFree(p); p = nullptr; *have = 0; }
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    p = nullptr;
    return failmsg(h, who + ": no device memory for " + what + (mib ? " (" + std::to_string(bytes >> 20) + " MiB)" : std::string()));
  }
  if (have) *have = bytes;
  return 0;
}

// The device's compute units, asked for once per handle.
static int cus(pf_handle* h) {
  if (h->df_cus < 1) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || n < 1) n = 256;
    h->df_cus = n;
  }
  return h->df_cus;
}

// The planners' validation kernels report the first offending index, an atomic minimum over the word at d_bad: arm_bad sets the
// word to ~0 (nothing found; it holds over kernels that find nothing) and clears the `flags` ints behind it where a call keeps
// some; first_bad, behind a validation kernel's launch, brings the word back.  Both synchronise the stream.
static int arm_bad(pf_handle* h, unsigned long long* d_bad, int* d_flags = nullptr, size_t flags = 0) {
  const unsigned long long none = ~0ull;
  CK(hipMemcpyAsync(d_bad, &none, sizeof(none), hipMemcpyHostToDevice, h->stream));
  if (d_flags) CK(hipMemsetAsync(d_flags, 0, sizeof(int) * flags, h->stream));
  CK(hipStreamSynchronize(h->stream));
  return 0;
}

static int first_bad(pf_handle* h, const unsigned long long* d_bad, unsigned long long& bad) {
  CK(hipGetLastError());
  CK(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
  CK(hipStreamSynchronize(h->stream));
  h->d2h_small += 1;
  return 0;
}

// The arguments every planner call shares: B problems or starts (`each`), and for the searches one matrix or mask set (`set`)
// per start or one for all, and the moves a start may take.
static int batch_args(pf_handle* h, const std::string& me, int B, const char* each, int shared = 0, int max_moves = 0, const char* set = "matrix") {
  if (B < 1) return failmsg(h, me + ": bad arguments (B = " + std::to_string(B) + ": at least one " + each + " is needed)");
  if (shared != 0 && shared != 1)
    return failmsg(h, me + ": bad arguments (shared = " + std::to_string(shared) + ": 0 a " + set + " per start, 1 one " + set + " for all)");
  if (max_moves < 0 || max_moves > (1 << 20)) return failmsg(h, me + ": bad arguments (max_moves = " + std::to_string(max_moves) + " must lie in [0, 2^20])");
  return 0;
}

// ---------------------------------------------------------------------------
// Distance fields: exact one-to-all path lengths from K sources or source sets (pf_dist_field.h).  One
// workgroup per row, min(rows, CUs) of them looping over the rows; each owns one slot of three rolling cell lists in HBM.  The
// slots are the handle's (allocated on first use, grown when a call needs more, freed by pf_destroy); nothing in them outlives
// a call, so pf_update_grid has nothing to invalidate.
// ---------------------------------------------------------------------------
#include "pf_dist_field.h"

// the handle's list slots for G workgroups (fewer where memory is short: G falls) and a control block of `words` ints
static int dist_field_reserve(pf_handle* h, const std::string& me, int& G, size_t words) {
  CK(hipSetDevice(h->device));
  const size_t slot_bytes = sizeof(int) * 3 * (size_t)h->RC;
  if (G > cus(h)) G = cus(h);
  if (G > h->df_slots) {                                            // grow the slots (a workgroup's lists: 12 RC bytes)
    CK(hipStreamSynchronize(h->stream));
    if (h->d_df_lists) { (void)hipFree(h->d_df_lists); h->d_df_lists = nullptr; h->df_slots = 0; }
    size_t free_b = 0, total_b = 0;
    CK(hipMemGetInfo(&free_b, &total_b));
    const size_t fit = free_b / 2 / slot_bytes;                     // on a large map fewer workgroups loop over more sources each
    if (fit < (size_t)G) G = (int)fit;
    if (G < 1 || hipMalloc(&h->d_df_lists, slot_bytes * (size_t)G) != hipSuccess) {
      (void)hipGetLastError();
      h->d_df_lists = nullptr;
      return failmsg(h, me + ": no device memory for the level lists (" + std::to_string(slot_bytes >> 20) + " MiB per workgroup, " +
                            std::to_string(free_b >> 20) + " MiB are free)");
    }
    h->df_slots = G;
  }
  if (words > 0x7FFFFFFFull) return failmsg(h, me + ": the source table is too large");
  return scratch(h, me, h->d_df_ctl, &h->df_ctl_bytes, sizeof(int) * std::max<size_t>(words, 64), "the source table", false);
}

// The one launch of the level kernel: B source sets, ctl = {error word 0, off[B + 1], ids} -> rows d_out[b][RC], d_info (or null)
static int dist_field_launch(pf_handle* h, const std::string& me, int allow_diag, int restrict_corner, int B, const std::vector<int>& ctl, double* d_out,
                             int64_t* d_info) {
  int G = B;
  if (dist_field_reserve(h, me, G, ctl.size())) return -2;
  CK(hipMemcpyAsync(h->d_df_ctl, ctl.data(), sizeof(int) * ctl.size(), hipMemcpyHostToDevice, h->stream));
  CK(hipStreamSynchronize(h->stream));                              // (ctl is pageable and may leave scope)
  int err = 0;
  const int rc = timed(h, [&] {
    hipLaunchKernelGGL(k_dist_field_merged_source_sets, dim3(G), dim3(PF_DF_THREADS), 0, h->stream, (const uint8_t*)h->d_occ,
                       move_mask(h, allow_diag, restrict_corner), h->RC, h->C, B, (const int*)(h->d_df_ctl + 1), (const int*)(h->d_df_ctl + 2 + B), d_out,
                       h->d_df_lists, (long long*)d_info, h->d_df_ctl);
  }, h->d_df_ctl, &err);
  if (rc) return rc;
  if (err == PF_DF_ERR_LEVELS) return failmsg(h, me + ": internal: level bound");
  if (err) return failmsg(h, me + ": internal: list bound");
  return 0;
}

int dist_field_run(pf_handle* h, const char* who, int allow_diag, int restrict_corner, int K, const int32_t* src, double* d_out, int64_t* d_info) {
  const std::string me(who);
  if (K < 1 || !src || !d_out) return failmsg(h, me + ": bad arguments (K >= 1, sources and rows must not be null)");
  for (int k = 0; k < K; ++k)
    if (src[k] < 0 || src[k] >= h->RC) return failmsg(h, me + ": source " + std::to_string(k) + " lies outside the grid");
  std::vector<int> ctl(1, 0);                                       // K sets of one: off = 0..K
  for (int k = 0; k <= K; ++k) ctl.push_back(k);
  ctl.insert(ctl.end(), src, src + K);
  return dist_field_launch(h, me, allow_diag, restrict_corner, K, ctl, d_out, d_info);
}

extern "C" {

int pf_dist_field_batch(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t K, const int32_t* src, double* d_out, int64_t* d_info) {
  if (!h) return -2;
  return dist_field_run(h, "pf_dist_field_batch", allow_diag, restrict_corner, K, src, d_out, d_info) ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Routing trees: DijkstraSolver's paths from a distance field (pf_field_paths.h).  pf_dist_field_parents turns K
// fields into K parent maps (one byte per cell) by the field-only rule; pf_dist_field_paths chases n (field, target) queries
// through them into path rows laid out as pf_astar_batch's.  Both keep nothing on the handle but the error word of the
// distance-field control block.
// ---------------------------------------------------------------------------
#include "pf_field_paths.h"

extern "C" {

int pf_dist_field_parents(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t K, const double* d_fields, uint8_t* d_parents) {
  if (!h) return -2;
  if (K < 1 || !d_fields || !d_parents) { failmsg(h, "pf_dist_field_parents: bad arguments (K >= 1, fields and parents must not be null)"); return -1; }
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    // (fields computed elsewhere: no control block yet)
    if (scratch(h, "pf_dist_field_parents", h->d_df_ctl, &h->df_ctl_bytes, sizeof(int) * 64, "the error word", false)) return -2;
    CK(hipMemsetAsync(h->d_df_ctl, 0, sizeof(int), h->stream));
    const unsigned gx = (unsigned)((h->RC + PF_FP_THREADS - 1) / PF_FP_THREADS), gy = (unsigned)(K < 65535 ? K : 65535);
    int err = 0;
    const int rc = timed(h, [&] {
      hipLaunchKernelGGL(k_dist_field_parent_map_thread_per_cell, dim3(gx, gy), dim3(PF_FP_THREADS), 0, h->stream, move_mask(h, allow_diag, restrict_corner),
                         h->RC, h->C, K, d_fields, d_parents, h->d_df_ctl);
    }, h->d_df_ctl, &err);
    if (rc) return rc;
    if (err) return failmsg(h, "pf_dist_field_parents: a finite cell has no parent: the fields are no fixed point of this grid and policy");
    return 0;
  };
  return run() ? -1 : 0;
}

int pf_dist_field_paths(pf_handle* h, int32_t K, const uint8_t* d_parents, const double* d_fields, int32_t n, const int32_t* d_field_idx,
                        const int32_t* d_target, int32_t reverse, int32_t path_cap, int32_t* d_cells, int32_t* d_len, int32_t* d_status,
                        int32_t* d_chosen) {
  if (!h) return -2;
  if (K < 1 || n < 0 || path_cap < 1 || !d_parents || !d_target || !d_cells || !d_len || !d_status || (!d_field_idx && !d_fields)) {
    failmsg(h, "pf_dist_field_paths: bad arguments (K >= 1, n >= 0, path_cap >= 1; parents, targets and outputs must not be null; "
               "without field indices the fields are needed for the nearest source)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_dist_field_trace_query_lanes, dim3((unsigned)((n + PF_FP_TRACE_THREADS - 1) / PF_FP_TRACE_THREADS)), dim3(PF_FP_TRACE_THREADS), 0,
                         h->stream, d_parents, d_fields, h->RC, h->C, K, n, d_field_idx, d_target, reverse ? 1 : 0, path_cap, d_cells, d_len, d_status,
                         d_chosen);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Nearest-source fields: one field seeded with a whole source set, and the owner of every cell (pf_nearest_field.h, DESIGN.md
// 4.13).  pf_dist_field_merged runs on the distance fields' list slots; pf_dist_field_owners needs one int32 [B][RC] scratch
// buffer for the length of the call.  Both keep the sets in the distance-field control block: {error word, off[B + 1], ids}.
// ---------------------------------------------------------------------------
#include "pf_nearest_field.h"

// the sets of a call, checked on the host; -> words of the control block
static int nearest_sets_check(pf_handle* h, const std::string& me, int B, const int32_t* set_off, const int32_t* src, std::vector<int>& ctl) {
  if (B < 1) return failmsg(h, me + ": bad arguments (B = " + std::to_string(B) + ": at least one source set is needed)");
  if (!set_off || !src) return failmsg(h, me + ": bad arguments (the set offsets and the sources must not be null)");
  if (set_off[0] != 0) return failmsg(h, me + ": set_off[0] = " + std::to_string(set_off[0]) + ": the offsets must start at 0");
  for (int b = 0; b < B; ++b) {
    if (set_off[b + 1] < set_off[b])
      return failmsg(h, me + ": set " + std::to_string(b) + ": set_off[" + std::to_string(b + 1) + "] = " + std::to_string(set_off[b + 1]) + " lies below set_off[" +
                            std::to_string(b) + "] = " + std::to_string(set_off[b]));
    if (set_off[b + 1] == set_off[b]) return failmsg(h, me + ": set " + std::to_string(b) + " is empty");
  }
  for (int b = 0; b < B; ++b)
    for (int j = set_off[b]; j < set_off[b + 1]; ++j)
      if (src[j] < 0 || src[j] >= h->RC)
        return failmsg(h, me + ": set " + std::to_string(b) + ", source " + std::to_string(j - set_off[b]) + " (index " + std::to_string(j) + ") = " +
                              std::to_string(src[j]) + " lies outside the grid");
  ctl.assign(1, 0);
  ctl.insert(ctl.end(), set_off, set_off + B + 1);
  ctl.insert(ctl.end(), src, src + set_off[B]);
  return 0;
}

extern "C" {

int pf_dist_field_merged(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t B, const int32_t* set_off, const int32_t* src, double* d_out,
                         int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_dist_field_merged");
  std::vector<int> ctl;
  if (nearest_sets_check(h, me, B, set_off, src, ctl)) return -1;
  if (!d_out) { failmsg(h, me + ": bad arguments (the rows must not be null)"); return -1; }
  return dist_field_launch(h, me, allow_diag, restrict_corner, B, ctl, d_out, d_info) ? -1 : 0;
}

int pf_dist_field_owners(pf_handle* h, int32_t B, const uint8_t* d_parents, const int32_t* set_off, const int32_t* src, const int64_t* d_info, int32_t* d_owner,
                         int64_t* d_count) {
  if (!h) return -2;
  const std::string me("pf_dist_field_owners");
  int* d_scratch = nullptr;
  auto run = [&]() -> int {
    std::vector<int> ctl;
    if (nearest_sets_check(h, me, B, set_off, src, ctl)) return -2;
    if (!d_parents || !d_owner) return failmsg(h, me + ": bad arguments (the parent maps and the owner rows must not be null)");
    const int RC = h->RC;
    int G = 0;                                                      // (no list slots: the control block only)
    if (dist_field_reserve(h, me, G, ctl.size())) return -2;
    // the rounds are fixed here, before the first launch: chains of at most n cells resolve in ceil(log2(n)) rounds
    long long n = RC;
    if (d_info) {
      std::vector<long long> info((size_t)B * 4);
      CK(hipMemcpyAsync(info.data(), d_info, sizeof(long long) * info.size(), hipMemcpyDeviceToHost, h->stream));
      CK(hipStreamSynchronize(h->stream));
      const size_t nb = sizeof(long long) * info.size();
      if (nb <= 128) h->d2h_small += 1; else { h->d2h_bulk += 1; h->d2h_bulk_bytes += (long long)nb; }
      long long most = 1;                                           // the cells of a chain lie in distinct live levels
      for (int b = 0; b < B; ++b) most = std::max(most, info[(size_t)b * 4]);
      n = std::min(n, most);
    }
    int rounds = 0;
    while ((1ll << rounds) < n) rounds += 1;
    if (scratch(h, me, d_scratch, nullptr, sizeof(int) * (size_t)B * (size_t)RC, "the second link buffer", true)) return -2;
    CK(hipMemcpyAsync(h->d_df_ctl, ctl.data(), sizeof(int) * ctl.size(), hipMemcpyHostToDevice, h->stream));
    CK(hipStreamSynchronize(h->stream));                            // (ctl is pageable and leaves scope)
    if (d_count) CK(hipMemsetAsync(d_count, 0, sizeof(int64_t) * (size_t)set_off[B], h->stream));
    const int* d_off = h->d_df_ctl + 1;
    const int* d_src = h->d_df_ctl + 2 + B;
    int most_src = 1;
    for (int b = 0; b < B; ++b) most_src = std::max(most_src, set_off[b + 1] - set_off[b]);
    const unsigned gx = (unsigned)((RC + PF_NF_THREADS - 1) / PF_NF_THREADS), gy = (unsigned)(B < 65535 ? B : 65535);
    const unsigned sx = (unsigned)std::min((most_src + PF_NF_THREADS - 1) / PF_NF_THREADS, 64);
    int* buf[2] = {(rounds & 1) ? (int*)d_owner : d_scratch, (rounds & 1) ? d_scratch : (int*)d_owner};   // the last round ends in the scratch buffer
    int err = 0;
    const int rc = timed(h, [&] {
      hipLaunchKernelGGL(k_nearest_owner_links, dim3(gx, gy), dim3(PF_NF_THREADS), 0, h->stream, d_parents, RC, h->C, B, buf[0], h->d_df_ctl);
      hipLaunchKernelGGL(k_nearest_owner_stamp_ranks, dim3(sx, gy), dim3(PF_NF_THREADS), 0, h->stream, RC, B, d_off, d_src, buf[0]);
      for (int t = 0; t < rounds; ++t)
        hipLaunchKernelGGL(k_nearest_owner_doubling, dim3(gx, gy), dim3(PF_NF_THREADS), 0, h->stream, RC, B, (const int*)buf[t & 1], buf[(t + 1) & 1]);
      hipLaunchKernelGGL(k_nearest_owner_write_and_count, dim3(gx, gy), dim3(PF_NF_THREADS), 0, h->stream, RC, B, d_off, (const int*)d_scratch, (int*)d_owner,
                         (unsigned long long*)d_count, h->d_df_ctl);
    }, h->d_df_ctl, &err);
    if (rc) return rc;
    if (err & PF_NF_ERR_CODE) return failmsg(h, me + ": the parent maps hold a code outside 0..8 and 255, or a step off the grid");
    if (err & PF_NF_ERR_ROOT) return failmsg(h, me + ": a root of the parent maps is no source of its set: the maps belong to other sets");
    if (err) return failmsg(h, me + ": a chain holds more cells than the bound of " + std::to_string(n) + " (" + std::to_string(rounds) +
                               " rounds): the parent maps are no forest, or d_info belongs to another field");
    return 0;
  };
  const int rc = run();
  if (d_scratch) { (void)hipStreamSynchronize(h->stream); (void)hipFree(d_scratch); }
  return rc ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Any-angle smoothing: line-of-sight tests and forward string pulling (pf_smooth.h).  Both read the handle's
// occupancy bytes at call time (pf_update_grid keeps working) and keep nothing on the handle.
// ---------------------------------------------------------------------------
#include "pf_smooth.h"

extern "C" {

int pf_line_of_sight_batch(pf_handle* h, int32_t restrict_corner, int32_t n, const int32_t* d_from, const int32_t* d_to, int32_t* d_visible,
                           int32_t* d_first_block) {
  if (!h) return -2;
  if (n < 0 || !d_from || !d_to || !d_visible) {
    failmsg(h, "pf_line_of_sight_batch: bad arguments (n >= 0; the endpoints and the visibility flags must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_line_of_sight_pairs_lanes_on_major, dim3((unsigned)n), dim3(64), 0, h->stream, (const uint8_t*)h->d_occ, h->RC, h->C, restrict_corner ? 1 : 0, n,
                         d_from, d_to, d_visible, d_first_block);
    });
  };
  return run() ? -1 : 0;
}

int pf_smooth_batch(pf_handle* h, int32_t restrict_corner, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, int32_t way_cap,
                    int32_t* d_way_cells, int32_t* d_way_idx, int32_t* d_way_len, double* d_stats, int32_t* d_status) {
  if (!h) return -2;
  if (n < 0 || path_cap < 1 || way_cap < 1 || !d_cells || !d_len || !d_way_cells || !d_way_len || !d_status) {
    failmsg(h, "pf_smooth_batch: bad arguments (n >= 0, path_cap >= 1, way_cap >= 1; the rows, the lengths, the waypoint rows, their lengths and "
               "the statuses must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_smooth_paths_one_wave_per_row, dim3((unsigned)n), dim3(64), 0, h->stream, (const uint8_t*)h->d_occ, h->RC, h->C, restrict_corner ? 1 : 0, n, path_cap,
                         d_cells, d_len, way_cap, d_way_cells, d_way_idx, d_way_len, d_stats, d_status);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Connected components: labels, sizes and reachability queries (pf_components.h).  The masks are read at call
// time (pf_update_grid keeps working); the handle keeps only the scratch words, allocated on first use.  Nothing here touches the
// searches' own labels (ensure_comp / d_comp).
// ---------------------------------------------------------------------------
#include "pf_components.h"

extern "C" {

int pf_components(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t* d_labels, int64_t* d_info) {
  if (!h) return -2;
  if (!d_labels) { failmsg(h, "pf_components: bad arguments (the labels must not be null)"); return -1; }
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    const int RC = h->RC, C = h->C;
    const unsigned nb = (unsigned)((RC + PF_CC_THREADS - 1) / PF_CC_THREADS);
    if (scratch(h, "pf_components", h->d_cc, nullptr, sizeof(unsigned long long) * PF_CC_CTL_WORDS + sizeof(int) * (3 * (size_t)RC + (size_t)nb),
                "the scratch words", true)) return -2;
    if (g_cc_phases) for (hipEvent_t& e : h->cc_ev) if (!e) CK(hipEventCreate(&e));
    unsigned long long* const ctl = (unsigned long long*)h->d_cc;    // (in front: 8-byte aligned whatever RC is)
    int* const parent = h->d_cc + 2 * PF_CC_CTL_WORDS;
    int* const rank = parent + RC;
    int* const size = rank + RC;
    int* const blocks = size + RC;
    const uint8_t* mm = move_mask(h, allow_diag, restrict_corner);
    const uint8_t* occ = h->d_occ;
    const dim3 grid(nb), block(PF_CC_THREADS);
    const unsigned hb = (unsigned)((RC + PF_CC_THREADS * PF_CC_HIST_PER - 1) / (PF_CC_THREADS * PF_CC_HIST_PER));
    int phase = 0;
    auto mark = [&]() -> hipError_t { return g_cc_phases ? hipEventRecord(h->cc_ev[phase++], h->stream) : hipSuccess; };
    const int rc = timed(h, [&]() -> int {
      CK(mark());
      CK(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * PF_CC_CTL_WORDS, h->stream));
#if PF_CC_TILED
      hipLaunchKernelGGL(k_cc_label_tiles_in_lds, dim3((unsigned)((C + PF_CC_TW - 1) / PF_CC_TW), (unsigned)((h->R + PF_CC_TH - 1) / PF_CC_TH)), block, 0, h->stream, occ, mm,
                         h->R, C, parent);
      hipLaunchKernelGGL(k_cc_link_tile_borders, grid, block, 0, h->stream, occ, mm, RC, C, parent);
#else
      hipLaunchKernelGGL(k_cc_init_parent_lowest_back_neighbour, grid, block, 0, h->stream, occ, mm, RC, C, parent);
      hipLaunchKernelGGL(k_cc_link_forward_edges, grid, block, 0, h->stream, occ, mm, RC, C, parent);
#endif
      CK(mark());                                                   // [0] link
      hipLaunchKernelGGL(k_cc_flatten_and_count_roots, grid, block, 0, h->stream, RC, (const int*)parent, (int*)d_labels, blocks);
      CK(mark());                                                   // [1] flatten
      hipLaunchKernelGGL(k_cc_scan_block_counts, dim3(1), dim3(PF_CC_SCAN_THREADS), 0, h->stream, (int)nb, blocks, ctl);
      hipLaunchKernelGGL(k_cc_rank_roots, grid, block, 0, h->stream, RC, (const int*)parent, (const int*)blocks, rank, size);
      CK(mark());                                                   // [2] rank
      hipLaunchKernelGGL(k_cc_write_labels, grid, block, 0, h->stream, RC, (const int*)rank, (int*)d_labels);
      CK(mark());                                                   // [3] labels
      if (d_info) {
        hipLaunchKernelGGL((k_cc_histogram<int>), dim3(hb), block, 0, h->stream, RC, (const int*)d_labels, (const unsigned long long*)ctl, 0, size, (unsigned*)nullptr, ctl + 1);
        hipLaunchKernelGGL(k_cc_largest, dim3(nb < 1024u ? nb : 1024u), block, 0, h->stream, (const int*)size, ctl);
        hipLaunchKernelGGL(k_cc_write_info_block, dim3(1), dim3(64), 0, h->stream, (const unsigned long long*)ctl, (long long*)d_info);
      }
      CK(mark());                                                   // [4] sizes and info
      return 0;
    });
    if (rc) return rc;
    for (int i = 0; i < 5; ++i) {
      h->cc_ms[i] = 0.f;
      if (g_cc_phases) CK(hipEventElapsedTime(&h->cc_ms[i], h->cc_ev[i], h->cc_ev[i + 1]));
    }
    return 0;
  };
  return run() ? -1 : 0;
}

int pf_components_phase_ms(pf_handle* h, float* ms) {
  if (!h) return -2;
  if (!ms) { failmsg(h, "pf_components_phase_ms: bad arguments"); return -1; }
  for (int i = 0; i < 5; ++i) ms[i] = h->cc_ms[i];
  return 0;
}

int pf_component_sizes(pf_handle* h, const int32_t* d_labels, int32_t count, int64_t* d_sizes, int32_t* d_first) {
  if (!h) return -2;
  if (!d_labels || count < 0) { failmsg(h, "pf_component_sizes: bad arguments (count >= 0; the labels must not be null)"); return -1; }
  if (count == 0 || (!d_sizes && !d_first)) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    const int RC = h->RC;
    const unsigned nb = (unsigned)((RC + PF_CC_THREADS - 1) / PF_CC_THREADS), cb = (unsigned)((count + PF_CC_THREADS - 1) / PF_CC_THREADS);
    return timed(h, [&]() -> int {
      if (d_sizes) CK(hipMemsetAsync(d_sizes, 0, sizeof(int64_t) * (size_t)count, h->stream));
      if (d_first) hipLaunchKernelGGL((k_cc_fill_words_with_a_value<unsigned>), dim3(cb), dim3(PF_CC_THREADS), 0, h->stream, (unsigned*)d_first, (int)count, 0xFFFFFFFFu);
      hipLaunchKernelGGL((k_cc_histogram<unsigned long long>), dim3((nb + PF_CC_HIST_PER - 1) / PF_CC_HIST_PER), dim3(PF_CC_THREADS), 0, h->stream, RC, (const int*)d_labels, (const unsigned long long*)nullptr,
                         (int)count, (unsigned long long*)d_sizes, (unsigned*)d_first, (unsigned long long*)nullptr);
      return 0;
    });
  };
  return run() ? -1 : 0;
}

int pf_components_same(pf_handle* h, const int32_t* d_labels, int32_t n, const int32_t* d_a, const int32_t* d_b, int32_t* d_same) {
  if (!h) return -2;
  if (n < 0 || !d_labels || !d_a || !d_b || !d_same) {
    failmsg(h, "pf_components_same: bad arguments (n >= 0; the labels, the two id rows and the answers must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_cc_same_pairs, dim3((unsigned)((n + PF_CC_THREADS - 1) / PF_CC_THREADS)), dim3(PF_CC_THREADS), 0, h->stream, h->RC, (const int*)d_labels, (int)n,
                         (const int*)d_a, (const int*)d_b, (int*)d_same);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Clearance fields: exact squared distances to the nearest obstacle, the margins of path rows and segments (pf_clearance.h,
// DESIGN.md 4.16).  The occupancy is read at call time (pf_update_grid keeps working); the handle keeps only the scratch words,
// allocated on first use.  Nothing here touches the scorer's own tables (ensure_pen / d_d2near / d_d2wide).
// ---------------------------------------------------------------------------
#include "pf_clearance.h"

extern "C" {

int pf_clearance_field(pf_handle* h, int32_t border, int32_t* d_d2, int32_t* d_near, int64_t* d_info) {
  if (!h) return -2;
  if (!d_d2) { failmsg(h, "pf_clearance_field: bad arguments (the squared distances must not be null)"); return -1; }
  if ((long long)h->R * h->R + (long long)h->C * h->C >= 0x7FFFFFFFll) {
    failmsg(h, "pf_clearance_field: bad arguments (R^2 + C^2 must stay below 2^31 - 1)");
    return -1;
  }
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    const int R = h->R, C = h->C, RC = h->RC;
    if (scratch(h, "pf_clearance_field", h->d_clear, nullptr,
                sizeof(unsigned long long) * PF_CL_CTL_WORDS + sizeof(int2) * (size_t)RC + sizeof(int) * ((size_t)RC + (size_t)C), "the scratch words", true))
      return -2;
    unsigned long long* const ctl = (unsigned long long*)h->d_clear;  // (in front: 8-byte aligned whatever RC is)
    int2* const stack = (int2*)(ctl + PF_CL_CTL_WORDS);
    int* const dcol = (int*)(stack + RC);
    int* const colflag = dcol + RC;
    const uint8_t* occ = h->d_occ;
    const unsigned rows_per = PF_CL_THREADS / 64;
    return timed(h, [&]() -> int {
      CK(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * PF_CL_CTL_WORDS, h->stream));
      CK(hipMemsetAsync(colflag, 0, sizeof(int) * (size_t)C, h->stream));
      hipLaunchKernelGGL(k_clear_rows_nearest_in_row, dim3(((unsigned)R + rows_per - 1) / rows_per), dim3(PF_CL_THREADS), 0, h->stream, occ, R, C, dcol);
      hipLaunchKernelGGL(k_clear_cols_outward_scan, dim3(((unsigned)C + 63u) / 64u, ((unsigned)R + rows_per - 1) / rows_per), dim3(PF_CL_THREADS), 0, h->stream,
                         (const int*)dcol, R, C, border ? 1 : 0, clear_scan_rows(C), (int*)d_d2, (int*)d_near, colflag);
      hipLaunchKernelGGL(k_clear_cols_lower_envelope, dim3(((unsigned)C + 63u) / 64u), dim3(64), 0, h->stream, (const int*)dcol, R, C, border ? 1 : 0,
                         (const int*)colflag, stack, (int*)d_d2, (int*)d_near);
      if (d_info) {
        const unsigned nb = (unsigned)((RC + PF_CL_THREADS - 1) / PF_CL_THREADS);
        hipLaunchKernelGGL(k_clear_info_reduce, dim3(nb < 2048u ? nb : 2048u), dim3(PF_CL_THREADS), 0, h->stream, occ, (const int*)d_d2, RC, ctl);
        hipLaunchKernelGGL(k_clear_write_info_block, dim3(1), dim3(64), 0, h->stream, (const unsigned long long*)ctl, RC, (long long*)d_info);
      }
      return 0;
    });
  };
  return run() ? -1 : 0;
}

int pf_clearance_paths(pf_handle* h, const int32_t* d_d2, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, int32_t margin_d2,
                       int32_t* d_out, int32_t* d_profile, int32_t* d_status) {
  if (!h) return -2;
  if (n < 0 || path_cap < 1 || margin_d2 < 0 || !d_d2 || !d_cells || !d_len || !d_out || !d_status) {
    failmsg(h, "pf_clearance_paths: bad arguments (n >= 0, path_cap >= 1, margin_d2 >= 0; the field, the rows, the lengths, the results and the "
               "statuses must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_clear_paths_one_wave_per_row, dim3((unsigned)n), dim3(64), 0, h->stream, (const int*)d_d2, h->RC, (int)n, (int)path_cap, (const int*)d_cells,
                         (const int*)d_len, (int)margin_d2, (int*)d_out, (int*)d_profile, (int*)d_status);
    });
  };
  return run() ? -1 : 0;
}

int pf_clearance_segments(pf_handle* h, const int32_t* d_d2, int32_t touched, int32_t n, const int32_t* d_from, const int32_t* d_to, int32_t* d_min,
                          int32_t* d_at) {
  if (!h) return -2;
  if (n < 0 || !d_d2 || !d_from || !d_to || !d_min) {
    failmsg(h, "pf_clearance_segments: bad arguments (n >= 0; the field, the endpoints and the minima must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_clear_segments_lanes_on_major, dim3((unsigned)n), dim3(64), 0, h->stream, (const int*)d_d2, h->RC, h->C, touched ? 1 : 0, (int)n,
                         (const int*)d_from, (const int*)d_to, (int*)d_min, (int*)d_at);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The tile-queue engine's host half (pf_tile_queue.h), shared by the widest, cost and turn fields: one call's
// view of the handle's scratch block, the round loop that reads a queue length after every launch, and the call's closing.  The
// block is the handle's (grown when a call needs more); nothing in it outlives a call and every call lays it out anew for its own
// B and tile.  A field's entry point supplies its checks, the fill of its rows, its seed launch, its relax launch and its info.
// ---------------------------------------------------------------------------
#include "pf_tile_queue.h"

struct TileCall {
  int B, tiles_x, tiles_y, ntiles;
  size_t T, nsets;                                                  // queue entries (B * ntiles); words of off [B + 1] and ids
  unsigned long long *moved, *top, *cells, *nsrc;                   // {words moved, an error word} | a field's own [B] | cells [B] | sources [B]
  int *count, *arg, *d_off, *d_src, *queue, *flag;                  // queue lengths [2], the offending cell, spare | arg [B] | off, ids | queues [2][T] | flags [2][T]
  unsigned seed_gx, gy;                                             // the seed kernel's grid for 256 threads, and the sets' grid dimension
  long long* work;                                                  // the handle's work words of this entry point
  long long launches = 0, visits = 0;
  unsigned long long end[2] = {0, 0};                               // the two words at `moved` when the call ends
};

// one round's kernel arguments: the current queue, and the queue, flags and length the launch fills
struct TileRound { const int* queue; int n, first; int *flag_now, *count_now, *flag_next, *queue_next, *count_next; };

// Lays the block out for B sets and a tile of TW x TH cells and clears the work words (sets: nearest_sets_check's).  A call may ask
// for extra_flags more words per (set, tile) and extra_ints more words behind the flags (the cost repair's: k.flag + 2 * k.T on).
static int tile_call(pf_handle* h, const std::string& me, int B, const std::vector<int>& sets, int TW, int TH, long long* work, TileCall& k,
                     size_t extra_flags = 0, size_t extra_ints = 0) {
  k.B = B;
  k.tiles_x = (h->C + TW - 1) / TW; k.tiles_y = (h->R + TH - 1) / TH; k.ntiles = k.tiles_x * k.tiles_y;
  if ((long long)B * k.ntiles >= 0x7FFFFFFFll) return failmsg(h, me + ": bad arguments (B times the number of tiles must stay below 2^31 - 1)");
  k.T = (size_t)B * (size_t)k.ntiles; k.nsets = sets.size() - 1;     // (sets[0] is the nearest fields' error word: not uploaded)
  const size_t n64 = 2 + 3 * (size_t)B;
  if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * n64 + sizeof(int) * (4 + (size_t)B + k.nsets + (4 + extra_flags) * k.T + extra_ints), "the scratch words", true)) return -2;
  k.moved = (unsigned long long*)h->d_widest;
  k.top = k.moved + 2;
  k.cells = k.top + B;
  k.nsrc = k.cells + B;
  k.count = (int*)(k.nsrc + B);
  k.arg = k.count + 4;
  k.d_off = k.arg + B;
  k.d_src = k.d_off + B + 1;
  k.queue = k.d_off + k.nsets;
  k.flag = k.queue + 2 * k.T;
  int most_src = 1;
  for (int b = 0; b < B; ++b) most_src = std::max(most_src, sets[b + 2] - sets[b + 1]);
  k.seed_gx = (unsigned)std::min((most_src + 255) / 256, 64);
  k.gy = (unsigned)(B < 65535 ? B : 65535);
  k.work = work;
  work[0] = work[1] = work[2] = work[3] = 0;
  return 0;
}

// Clears the block's counters, queue lengths and flags (the field's own [B] words to top_byte) and uploads the sets
static int tile_upload(pf_handle* h, const TileCall& k, const std::vector<int>& sets, int top_byte) {
  CK(hipMemsetAsync(k.moved, 0, sizeof(unsigned long long) * (2 + 3 * (size_t)k.B) + sizeof(int) * 2, h->stream));   // counters, top, cells, sources, queue lengths
  if (top_byte) CK(hipMemsetAsync(k.top, top_byte, sizeof(unsigned long long) * (size_t)k.B, h->stream));
  CK(hipMemsetAsync(k.arg, 0x7F, sizeof(int) * (size_t)k.B, h->stream));   // (any word above every cell id: 2^24 cells at most, as the level kernel's)
  CK(hipMemsetAsync(k.flag, 0, sizeof(int) * 2 * k.T, h->stream));
  CK(hipMemcpyAsync(k.d_off, sets.data() + 1, sizeof(int) * k.nsets, hipMemcpyHostToDevice, h->stream));
  CK(hipStreamSynchronize(h->stream));                              // (sets is pageable and leaves scope)
  return 0;
}

// The rounds, after the seed launch: launch(r) enqueues one relax kernel over r.n queued tiles; the host reads the next queue's
// length after each and stops at 0.  Queues, flags and lengths alternate by the round's parity.
template <typename F>
static int tile_rounds(pf_handle* h, const std::string& me, TileCall& k, long long round_bound, F&& launch) {
  CK(hipGetLastError());
  int n = 0;
  CK(hipMemcpyAsync(&n, k.count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  CK(hipStreamSynchronize(h->stream));
  for (long long round = 0; n > 0; ++round) {
    if (round > round_bound) return failmsg(h, me + ": internal: round bound");
    if (n < 0 || (size_t)n > k.T) return failmsg(h, me + ": internal: queue bound");
    const size_t now = (size_t)(round & 1) * k.T, next = k.T - now;
    const int p = (int)(round & 1);
    launch(TileRound{k.queue + now, n, round == 0 ? 1 : 0, k.flag + now, k.count + p, k.flag + next, k.queue + next, k.count + (p ^ 1)});
    CK(hipGetLastError());
    k.launches += 1; k.visits += n;
    CK(hipMemcpyAsync(&n, k.count + (p ^ 1), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    CK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

// The end of a call: ev1, the block's two counters, last_ms, the copies made (one per launch, the seed's and this one) and the work words
static int tile_finish(pf_handle* h, TileCall& k) {
  CK(hipGetLastError());
  CK(hipEventRecord(h->ev1, h->stream));
  CK(hipMemcpyAsync(k.end, k.moved, sizeof(k.end), hipMemcpyDeviceToHost, h->stream));
  CK(hipStreamSynchronize(h->stream));
  CK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  h->d2h_small += k.launches + 2;
  k.work[0] = k.launches; k.work[1] = k.visits; k.work[2] = (long long)k.end[0];
  return 0;
}

static int tile_work(pf_handle* h, const char* who, const long long* work, int64_t* out4) {
  if (!h) return -2;
  if (!out4) { failmsg(h, std::string(who) + ": bad arguments (the four words must not be null)"); return -1; }
  for (int i = 0; i < 4; ++i) out4[i] = work[i];
  return 0;
}

// ---------------------------------------------------------------------------
// Widest-path fields over a clearance field (pf_widest.h).  Reads the caller's d2 only, never the handle's
// occupancy or masks; the handle keeps the last call's work counters.  Rounds and scratch: the tile-queue engine's, above.
// ---------------------------------------------------------------------------
#include "pf_widest.h"

extern "C" {

int pf_clearance_widest(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const int32_t* d_d2, int32_t B, const int32_t* set_off, const int32_t* src,
                        int32_t* d_out, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_clearance_widest");
  auto run = [&]() -> int {
    std::vector<int> sets;
    if (nearest_sets_check(h, me, B, set_off, src, sets)) return -2;
    if (!d_d2 || !d_out) return failmsg(h, me + ": bad arguments (the field and the rows must not be null)");
    CK(hipSetDevice(h->device));
    const int R = h->R, C = h->C, RC = h->RC;
    TileCall k;                                                       // top: the smallest (w << 32) | id per set, preset to all ones
    if (const int rc = tile_call(h, me, B, sets, PF_WD_TW, PF_WD_TH, h->widest_work, k)) return rc;
    CK(hipEventRecord(h->ev0, h->stream));
    CK(hipMemsetAsync(d_out, 0, sizeof(int) * (size_t)B * (size_t)RC, h->stream));
    if (tile_upload(h, k, sets, 0xFF)) return -2;
    hipLaunchKernelGGL(k_widest_seed_sets, dim3(k.seed_gx, k.gy), dim3(PF_WD_THREADS), 0, h->stream, (const int*)d_d2, RC, C, k.tiles_x, k.ntiles, (int)B,
                       (const int*)k.d_off, (const int*)k.d_src, (int*)d_out, k.flag, k.queue, k.count, k.nsrc);
    if (const int rc = tile_rounds(h, me, k, RC, [&](const TileRound& r) {
          hipLaunchKernelGGL(k_widest_relax_tiles_in_lds, dim3((unsigned)r.n), dim3(PF_WD_THREADS), 0, h->stream, (const int*)d_d2, R, C, allow_diag ? 1 : 0,
                             restrict_corner ? 1 : 0, k.tiles_x, k.tiles_y, (int*)d_out, r.queue, r.n, r.first, r.flag_now, r.count_now, r.flag_next, r.queue_next,
                             r.count_next, k.moved);
        })) return rc;
    if (d_info) {
      const unsigned nb = (unsigned)((RC + PF_WD_THREADS - 1) / PF_WD_THREADS);
      hipLaunchKernelGGL(k_widest_info_sum, dim3(nb < 1024u ? nb : 1024u, k.gy), dim3(PF_WD_THREADS), 0, h->stream, (const int*)d_out, RC, (int)B, k.top, k.cells);
      hipLaunchKernelGGL(k_widest_write_info, dim3(((unsigned)B + PF_WD_THREADS - 1) / PF_WD_THREADS), dim3(PF_WD_THREADS), 0, h->stream, (int)B,
                         (const unsigned long long*)k.top, (const unsigned long long*)k.cells, (const unsigned long long*)k.nsrc, (long long*)d_info);
    }
    return tile_finish(h, k);
  };
  return run() ? -1 : 0;
}

int pf_clearance_widest_work(pf_handle* h, int64_t* out4) { return tile_work(h, "pf_clearance_widest_work", h ? h->widest_work : nullptr, out4); }

}  // extern "C"

// ---------------------------------------------------------------------------
// Cost fields: exact weighted shortest paths over a per-cell cost map (pf_cost_field.h).  The occupancy and the
// masks are read at call time (pf_update_grid keeps working).  The handle keeps the last call's work counters.  Rounds and
// scratch: the tile-queue engine's, over the widest paths' tile.
// ---------------------------------------------------------------------------
#include "pf_cost_field.h"
#include "pf_cost_repair.h"

// The costs of the free cells, before any output is touched: `word` (device) takes the smallest offending cell.  ev0, where given,
// is recorded behind the upload of the word.  One small copy back.
static int cost_map_check(pf_handle* h, const std::string& me, const double* d_cost, int* word, hipEvent_t ev0) {
  const int RC = h->RC, C = h->C;
  const unsigned nb = (unsigned)((RC + PF_CF_THREADS - 1) / PF_CF_THREADS);
  int bad = 0x7FFFFFFF;
  CK(hipMemcpyAsync(word, &bad, sizeof(int), hipMemcpyHostToDevice, h->stream));
  CK(hipStreamSynchronize(h->stream));
  if (ev0) CK(hipEventRecord(ev0, h->stream));
  hipLaunchKernelGGL(k_cost_validate_free_cells, dim3(nb < 2048u ? nb : 2048u), dim3(PF_CF_THREADS), 0, h->stream, (const uint8_t*)h->d_occ, d_cost, RC, word);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(&bad, word, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  CK(hipStreamSynchronize(h->stream));
  h->d2h_small += 1;
  if (bad != 0x7FFFFFFF)
    return failmsg(h, me + ": bad arguments (the cost of the free cell (" + std::to_string(bad / C) + ", " + std::to_string(bad % C) +
                          ") is not a finite number in [1, 2^20])");
  return 0;
}

// rows [n] become +inf
static void cost_fill_inf(pf_handle* h, double* rows, size_t n) {
  hipLaunchKernelGGL(k_cost_fill_inf, dim3((unsigned)std::min<size_t>((n + PF_CF_THREADS - 1) / PF_CF_THREADS, 4096)), dim3(PF_CF_THREADS), 0, h->stream,
                     (unsigned long long*)rows, n);
}

// info [B][4] of the rows [B][RC] of a call: top takes the largest finite label per set
static void cost_info(pf_handle* h, const TileCall& k, const double* rows, int64_t* d_info) {
  const int RC = h->RC;
  const unsigned nb = (unsigned)((RC + PF_CF_THREADS - 1) / PF_CF_THREADS);
  hipLaunchKernelGGL(k_cost_info_largest, dim3(nb < 1024u ? nb : 1024u, k.gy), dim3(PF_CF_THREADS), 0, h->stream, rows, RC, k.B, k.top, k.cells);
  hipLaunchKernelGGL(k_cost_info_arg, dim3(nb < 1024u ? nb : 1024u, k.gy), dim3(PF_CF_THREADS), 0, h->stream, rows, RC, k.B, (const unsigned long long*)k.top, k.arg);
  hipLaunchKernelGGL(k_cost_write_info, dim3(((unsigned)k.B + PF_CF_THREADS - 1) / PF_CF_THREADS), dim3(PF_CF_THREADS), 0, h->stream, k.B,
                     (const unsigned long long*)k.cells, (const unsigned long long*)k.nsrc, (const int*)k.arg, (long long*)d_info);
}

extern "C" {

int pf_cost_field(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, int32_t B, const int32_t* set_off, const int32_t* src,
                  double* d_out, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_cost_field");
  auto run = [&]() -> int {
    std::vector<int> sets;
    if (nearest_sets_check(h, me, B, set_off, src, sets)) return -2;
    if (!d_cost || !d_out) return failmsg(h, me + ": bad arguments (the cost map and the rows must not be null)");
    CK(hipSetDevice(h->device));
    const int R = h->R, C = h->C, RC = h->RC;
    TileCall k;                                                       // top: the largest finite label's bits per set
    if (const int rc = tile_call(h, me, B, sets, PF_WD_TW, PF_WD_TH, h->cost_work, k)) return rc;
    if (const int rc = cost_map_check(h, me, d_cost, k.count + 2, h->ev0)) return rc;
    if (tile_upload(h, k, sets, 0)) return -2;
    cost_fill_inf(h, d_out, (size_t)B * (size_t)RC);
    hipLaunchKernelGGL(k_cost_seed_sets, dim3(k.seed_gx, k.gy), dim3(PF_CF_THREADS), 0, h->stream, (const uint8_t*)h->d_occ, RC, C, k.tiles_x, k.ntiles, (int)B,
                       (const int*)k.d_off, (const int*)k.d_src, d_out, k.flag, k.queue, k.count, k.nsrc);
    const uint8_t* mm = move_mask(h, allow_diag, restrict_corner);
    if (const int rc = tile_rounds(h, me, k, (long long)RC + 1, [&](const TileRound& r) {
          hipLaunchKernelGGL(k_cost_relax_tiles_in_lds, dim3((unsigned)r.n), dim3(PF_CF_THREADS), 0, h->stream, (const uint8_t*)h->d_occ, mm, d_cost, R, C,
                             allow_diag ? 1 : 0, k.tiles_x, k.tiles_y, d_out, r.queue, r.n, r.first, r.flag_now, r.count_now, r.flag_next, r.queue_next, r.count_next,
                             k.moved);
        })) return rc;
    if (d_info) cost_info(h, k, d_out, d_info);
    return tile_finish(h, k);
  };
  return run() ? -1 : 0;
}

int pf_cost_field_work(pf_handle* h, int64_t* out4) { return tile_work(h, "pf_cost_field_work", h ? h->cost_work : nullptr, out4); }

// Cost-field repair (pf_cost_repair.h): the raise phase and the lower phase, each a run of tile_rounds over the
// same queues (a phase ends with both queue lengths and every flag at 0: the next one starts at parity 0 again).  The block grows
// by the touched flags [T] and the device copy of the changed list, behind the flags.  moved[1] takes the words raised.
int pf_cost_field_repair(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, int32_t n_changed, const int32_t* changed, int32_t B,
                         const int32_t* set_off, const int32_t* src, double* d_rows, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_cost_field_repair");
  auto run = [&]() -> int {
    std::vector<int> listed;
    if (nearest_sets_check(h, me, B, set_off, src, listed)) return -2;
    if (!d_cost || !d_rows) return failmsg(h, me + ": bad arguments (the cost map and the rows must not be null)");
    if (n_changed < 0) return failmsg(h, me + ": bad arguments (n_changed = " + std::to_string(n_changed) + ": the number of changed cells must not be negative)");
    if (n_changed > 0 && !changed) return failmsg(h, me + ": bad arguments (the changed cells must not be null when n_changed > 0)");
    for (int i = 0; i < n_changed; ++i)
      if (changed[i] < 0 || changed[i] >= h->RC)
        return failmsg(h, me + ": changed[" + std::to_string(i) + "] = " + std::to_string(changed[i]) + " lies outside the grid");
    std::vector<int> sets(1, 0);                                      // the sets with every source once: {error word, off [B + 1], ids}
    {
      std::vector<int> off(1, 0), ids;
      for (int b = 0; b < B; ++b) {
        std::vector<int> s(src + set_off[b], src + set_off[b + 1]);
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        ids.insert(ids.end(), s.begin(), s.end());
        off.push_back((int)ids.size());
      }
      sets.insert(sets.end(), off.begin(), off.end());
      sets.insert(sets.end(), ids.begin(), ids.end());
    }
    CK(hipSetDevice(h->device));
    const int R = h->R, C = h->C, RC = h->RC;
    TileCall k;                                                       // top: the largest finite label's bits per set
    if (const int rc = tile_call(h, me, B, sets, PF_WD_TW, PF_WD_TH, h->cost_work, k, 1, (size_t)n_changed)) return rc;
    int* const touched = k.flag + 2 * k.T;
    int* const d_changed = touched + k.T;
    if (const int rc = cost_map_check(h, me, d_cost, k.count + 2, h->ev0)) return rc;
    CK(hipMemsetAsync(touched, 0, sizeof(int) * k.T, h->stream));
    if (n_changed) CK(hipMemcpyAsync(d_changed, changed, sizeof(int) * (size_t)n_changed, hipMemcpyHostToDevice, h->stream));
    if (tile_upload(h, k, sets, 0)) return -2;                        // (it synchronises: the caller's list may leave scope)
    const uint8_t* occ = h->d_occ;
    const uint8_t* mm = move_mask(h, allow_diag, restrict_corner);
    const int most = std::max(std::max((int)std::min<size_t>(k.T, 0x7FFFFFFF), (int)n_changed), sets[B + 1]);
    const dim3 qgrid((unsigned)std::min((n_changed + PF_CF_THREADS - 1) / PF_CF_THREADS, 256), k.gy);
    const dim3 lgrid((unsigned)std::min((most + PF_CF_THREADS - 1) / PF_CF_THREADS, 256), k.gy);
    if (n_changed) {
      hipLaunchKernelGGL(k_repair_queue_changed_blocks, qgrid, dim3(PF_CF_THREADS), 0, h->stream, R, C, k.tiles_x, k.ntiles, (int)B, (int)n_changed, (const int*)d_changed,
                         k.flag, k.queue, k.count);
      if (const int rc = tile_rounds(h, me, k, (long long)RC + 1, [&](const TileRound& r) {
            hipLaunchKernelGGL(k_cost_raise_tiles_in_lds, dim3((unsigned)r.n), dim3(PF_CF_THREADS), 0, h->stream, occ, mm, d_cost, R, C, allow_diag ? 1 : 0, k.tiles_x,
                               k.tiles_y, d_rows, r.queue, r.n, r.flag_now, r.count_now, r.flag_next, r.queue_next, r.count_next, touched, k.moved + 1);
          })) return rc;
    }
    if (n_changed || d_info)                                          // (nothing listed: it only counts the sources, for the info)
      hipLaunchKernelGGL(k_repair_queue_lower, lgrid, dim3(PF_CF_THREADS), 0, h->stream, occ, R, C, k.tiles_x, k.ntiles, (int)B, (int)k.T, (const int*)touched,
                       (int)n_changed, (const int*)d_changed, (const int*)k.d_off, (const int*)k.d_src, n_changed ? 1 : 0, d_rows, k.flag, k.queue, k.count, k.nsrc);
    if (n_changed)
      if (const int rc = tile_rounds(h, me, k, (long long)RC + 1, [&](const TileRound& r) {
            hipLaunchKernelGGL(k_cost_relax_tiles_in_lds, dim3((unsigned)r.n), dim3(PF_CF_THREADS), 0, h->stream, occ, mm, d_cost, R, C, allow_diag ? 1 : 0, k.tiles_x,
                               k.tiles_y, d_rows, r.queue, r.n, r.first, r.flag_now, r.count_now, r.flag_next, r.queue_next, r.count_next, k.moved);
          })) return rc;
    if (d_info) cost_info(h, k, d_rows, d_info);
    if (const int rc = tile_finish(h, k)) return rc;
    k.work[3] = (long long)k.end[1];
    return 0;
  };
  return run() ? -1 : 0;
}

int pf_cost_field_parents(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, int32_t K, const double* d_fields, uint8_t* d_parents) {
  if (!h) return -2;
  if (K < 1 || !d_cost || !d_fields || !d_parents) {
    failmsg(h, "pf_cost_field_parents: bad arguments (K >= 1; the cost map, the fields and the parents must not be null)");
    return -1;
  }
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    if (scratch(h, "pf_cost_field_parents", h->d_df_ctl, &h->df_ctl_bytes, sizeof(int) * 64, "the error word", false)) return -2;
    CK(hipMemsetAsync(h->d_df_ctl, 0, sizeof(int), h->stream));
    const unsigned gx = (unsigned)((h->RC + PF_FP_THREADS - 1) / PF_FP_THREADS), gy = (unsigned)(K < 65535 ? K : 65535);
    int err = 0;
    const int rc = timed(h, [&] {
      hipLaunchKernelGGL(k_cost_parent_map_thread_per_cell, dim3(gx, gy), dim3(PF_FP_THREADS), 0, h->stream, move_mask(h, allow_diag, restrict_corner), d_cost,
                         h->RC, h->C, K, d_fields, d_parents, h->d_df_ctl);
    }, h->d_df_ctl, &err);
    if (rc) return rc;
    if (err) return failmsg(h, "pf_cost_field_parents: a finite cell has no parent: the fields are no fixed point of this grid, policy and cost map");
    return 0;
  };
  return run() ? -1 : 0;
}

int pf_cost_paths(pf_handle* h, const double* d_cost, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, double* d_total, int32_t* d_bad) {
  if (!h) return -2;
  if (n < 0 || path_cap < 1 || !d_cost || !d_cells || !d_len || !d_total || !d_bad) {
    failmsg(h, "pf_cost_paths: bad arguments (n >= 0, path_cap >= 1; the cost map, the rows, the lengths, the totals and the step indices must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_cost_paths_one_wave_per_row, dim3((unsigned)n), dim3(64), 0, h->stream, d_cost, h->RC, h->C, (int)n, (int)path_cap, (const int*)d_cells,
                         (const int*)d_len, d_total, (int*)d_bad);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Turn fields: the exact optimum of length plus a turn penalty over (cell, heading) states (pf_turn_field.h).
// The handle keeps the last call's work counters.  Rounds and scratch: the tile-queue engine's, over the turn tile (PF_TF_TW x
// PF_TF_TH).
// ---------------------------------------------------------------------------
#include "pf_turn_field.h"
#include "pf_turn_repair.h"

static_assert(PF_WD_THREADS == 256 && PF_CF_THREADS == 256 && PF_TF_THREADS == 256, "tile_call sizes the seed grids for 256 threads");

// a turn weight is a finite double in [0, 2^20] (NaN fails both comparisons)
static int turn_weight_check(pf_handle* h, const std::string& me, double turn_weight) {
  if (turn_weight >= 0.0 && turn_weight <= PF_TF_WEIGHT_MAX) return 0;
  return failmsg(h, me + ": bad arguments (the turn weight is not a finite number in [0, 2^20])");
}

extern "C" {

int pf_turn_field(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, double turn_weight, int32_t B, const int32_t* set_off,
                  const int32_t* src, double* d_states, double* d_best, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_turn_field");
  auto run = [&]() -> int {
    std::vector<int> sets;
    if (nearest_sets_check(h, me, B, set_off, src, sets)) return -2;
    if (!d_states || !d_best) return failmsg(h, me + ": bad arguments (the states and the best rows must not be null)");
    if (turn_weight_check(h, me, turn_weight)) return -2;
    CK(hipSetDevice(h->device));
    const int R = h->R, C = h->C, RC = h->RC;
    TileCall k;                                                       // top: the largest finite best label's bits per set; moved[1]: the sweep bound's error word
    if (const int rc = tile_call(h, me, B, sets, PF_TF_TW, PF_TF_TH, h->turn_work, k)) return rc;
    CK(hipEventRecord(h->ev0, h->stream));
    if (d_cost)
      if (const int rc = cost_map_check(h, me, d_cost, k.count + 2, nullptr)) return rc;
    if (tile_upload(h, k, sets, 0)) return -2;
    const size_t words = (size_t)B * (size_t)RC;
    cost_fill_inf(h, d_states, 8 * words);
    cost_fill_inf(h, d_best, words);
    hipLaunchKernelGGL(k_turn_seed_sets, dim3(k.seed_gx, k.gy), dim3(PF_TF_THREADS), 0, h->stream, (const uint8_t*)h->d_occ, RC, C, k.tiles_x, k.ntiles, (int)B,
                       (const int*)k.d_off, (const int*)k.d_src, d_states, d_best, k.flag, k.queue, k.count, k.nsrc);
    const uint8_t* mm = move_mask(h, allow_diag, restrict_corner);
    if (const int rc = tile_rounds(h, me, k, 8 * (long long)RC + 1, [&](const TileRound& r) {
          hipLaunchKernelGGL(k_turn_relax_tiles_in_lds, dim3((unsigned)r.n), dim3(PF_TF_THREADS), 0, h->stream, (const uint8_t*)h->d_occ, mm, d_cost, turn_weight, R, C,
                             allow_diag ? 1 : 0, k.tiles_x, k.tiles_y, d_states, d_best, r.queue, r.n, r.first, r.flag_now, r.count_now, r.flag_next, r.queue_next,
                             r.count_next, k.moved);
        })) return rc;
    if (d_info) cost_info(h, k, d_best, d_info);
    if (const int rc = tile_finish(h, k)) return rc;
    if (k.end[1]) return failmsg(h, me + ": internal: sweep bound");
    return 0;
  };
  return run() ? -1 : 0;
}

int pf_turn_field_work(pf_handle* h, int64_t* out4) { return tile_work(h, "pf_turn_field_work", h ? h->turn_work : nullptr, out4); }

// Turn-field repair (pf_turn_repair.h): pf_cost_field_repair's two runs of tile_rounds over the turn tile.  The
// block grows by the touched flags [T], the raise phase's two words {state words raised, its sweep bound's error word} -- moved[1]
// is the relax kernel's error word in turn calls -- and the device copy of the changed list, behind the flags.
int pf_turn_field_repair(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, const double* d_cost, double turn_weight, int32_t n_changed, const int32_t* changed,
                         int32_t B, const int32_t* set_off, const int32_t* src, double* d_states, double* d_best, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_turn_field_repair");
  auto run = [&]() -> int {
    std::vector<int> listed;
    if (nearest_sets_check(h, me, B, set_off, src, listed)) return -2;
    if (!d_states || !d_best) return failmsg(h, me + ": bad arguments (the states and the best rows must not be null)");
    if (turn_weight_check(h, me, turn_weight)) return -2;
    if (n_changed < 0) return failmsg(h, me + ": bad arguments (n_changed = " + std::to_string(n_changed) + ": the number of changed cells must not be negative)");
    if (n_changed > 0 && !changed) return failmsg(h, me + ": bad arguments (the changed cells must not be null when n_changed > 0)");
    for (int i = 0; i < n_changed; ++i)
      if (changed[i] < 0 || changed[i] >= h->RC)
        return failmsg(h, me + ": changed[" + std::to_string(i) + "] = " + std::to_string(changed[i]) + " lies outside the grid");
    std::vector<int> sets(1, 0);                                      // the sets with every source once: {error word, off [B + 1], ids}
    {
      std::vector<int> off(1, 0), ids;
      for (int b = 0; b < B; ++b) {
        std::vector<int> s(src + set_off[b], src + set_off[b + 1]);
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        ids.insert(ids.end(), s.begin(), s.end());
        off.push_back((int)ids.size());
      }
      sets.insert(sets.end(), off.begin(), off.end());
      sets.insert(sets.end(), ids.begin(), ids.end());
    }
    CK(hipSetDevice(h->device));
    const int R = h->R, C = h->C, RC = h->RC;
    TileCall k;                                                       // top: the largest finite best label's bits per set; moved[1]: the relax kernel's sweep-bound word
    if (const int rc = tile_call(h, me, B, sets, PF_TF_TW, PF_TF_TH, h->turn_work, k, 1, (size_t)n_changed + 6)) return rc;
    int* const touched = k.flag + 2 * k.T;
    unsigned long long* const rwords = (unsigned long long*)(((uintptr_t)(touched + k.T) + 7u) & ~(uintptr_t)7u);   // (8-byte aligned: at most one word of the six is skipped)
    int* const d_changed = (int*)(rwords + 2);
    CK(hipEventRecord(h->ev0, h->stream));
    if (d_cost)
      if (const int rc = cost_map_check(h, me, d_cost, k.count + 2, nullptr)) return rc;
    CK(hipMemsetAsync(touched, 0, sizeof(int) * k.T, h->stream));
    CK(hipMemsetAsync(rwords, 0, sizeof(unsigned long long) * 2, h->stream));
    if (n_changed) CK(hipMemcpyAsync(d_changed, changed, sizeof(int) * (size_t)n_changed, hipMemcpyHostToDevice, h->stream));
    if (tile_upload(h, k, sets, 0)) return -2;                        // (it synchronises: the caller's list may leave scope)
    const uint8_t* occ = h->d_occ;
    const uint8_t* mm = move_mask(h, allow_diag, restrict_corner);
    const int most = std::max(std::max((int)std::min<size_t>(k.T, 0x7FFFFFFF), (int)n_changed), sets[B + 1]);
    const dim3 qgrid((unsigned)std::min((n_changed + PF_TF_THREADS - 1) / PF_TF_THREADS, 256), k.gy);
    const dim3 lgrid((unsigned)std::min((most + PF_TF_THREADS - 1) / PF_TF_THREADS, 256), k.gy);
    if (n_changed) {
      hipLaunchKernelGGL(k_turn_repair_queue_changed_blocks, qgrid, dim3(PF_TF_THREADS), 0, h->stream, R, C, k.tiles_x, k.ntiles, (int)B, (int)n_changed,
                         (const int*)d_changed, k.flag, k.queue, k.count);
      if (const int rc = tile_rounds(h, me, k, 8 * (long long)RC + 1, [&](const TileRound& r) {
            hipLaunchKernelGGL(k_turn_raise_tiles_in_lds, dim3((unsigned)r.n), dim3(PF_TF_THREADS), 0, h->stream, occ, mm, d_cost, turn_weight, R, C, allow_diag ? 1 : 0,
                               k.tiles_x, k.tiles_y, d_states, d_best, r.queue, r.n, r.flag_now, r.count_now, r.flag_next, r.queue_next, r.count_next, touched, rwords);
          })) return rc;
    }
    if (n_changed || d_info)                                          // (nothing listed: it only counts the sources, for the info)
      hipLaunchKernelGGL(k_turn_repair_queue_lower, lgrid, dim3(PF_TF_THREADS), 0, h->stream, occ, R, C, k.tiles_x, k.ntiles, (int)B, (int)k.T, (const int*)touched,
                         (int)n_changed, (const int*)d_changed, (const int*)k.d_off, (const int*)k.d_src, n_changed ? 1 : 0, d_states, d_best, k.flag, k.queue, k.count,
                         k.nsrc);
    if (n_changed)
      if (const int rc = tile_rounds(h, me, k, 8 * (long long)RC + 1, [&](const TileRound& r) {
            hipLaunchKernelGGL(k_turn_relax_tiles_in_lds, dim3((unsigned)r.n), dim3(PF_TF_THREADS), 0, h->stream, occ, mm, d_cost, turn_weight, R, C, allow_diag ? 1 : 0,
                               k.tiles_x, k.tiles_y, d_states, d_best, r.queue, r.n, r.first, r.flag_now, r.count_now, r.flag_next, r.queue_next, r.count_next, k.moved);
          })) return rc;
    if (d_info) cost_info(h, k, d_best, d_info);
    if (const int rc = tile_finish(h, k)) return rc;
    unsigned long long rw[2] = {0, 0};
    CK(hipMemcpyAsync(rw, rwords, sizeof(rw), hipMemcpyDeviceToHost, h->stream));
    CK(hipStreamSynchronize(h->stream));
    h->d2h_small += 1;
    k.work[3] = (long long)rw[0];
    if (k.end[1] || rw[1]) return failmsg(h, me + ": internal: sweep bound");
    return 0;
  };
  return run() ? -1 : 0;
}

int pf_turn_field_paths(pf_handle* h, const double* d_cost, double turn_weight, int32_t B, const double* d_states, int32_t n, const int32_t* d_set_idx,
                        const int32_t* d_target, int32_t reverse, int32_t path_cap, int32_t* d_cells, int32_t* d_len, int32_t* d_status) {
  if (!h) return -2;
  if (B < 1 || n < 0 || path_cap < 1 || !d_states || !d_set_idx || !d_target || !d_cells || !d_len || !d_status) {
    failmsg(h, "pf_turn_field_paths: bad arguments (B >= 1, n >= 0, path_cap >= 1; the states, the set indices, the targets, the rows, the lengths and the statuses must not be null)");
    return -1;
  }
  if (turn_weight_check(h, "pf_turn_field_paths", turn_weight)) return -1;
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_turn_trace_query_lanes, dim3(((unsigned)n + PF_FP_TRACE_THREADS - 1) / PF_FP_TRACE_THREADS), dim3(PF_FP_TRACE_THREADS), 0, h->stream, d_cost,
                         turn_weight, h->R, h->C, (int)B, d_states, (int)n, (const int*)d_set_idx, (const int*)d_target, reverse ? 1 : 0, (int)path_cap, (int*)d_cells,
                         (int*)d_len, (int*)d_status);
    });
  };
  return run() ? -1 : 0;
}

int pf_turn_paths(pf_handle* h, const double* d_cost, double turn_weight, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, double* d_total,
                  int32_t* d_turns, int32_t* d_bad) {
  if (!h) return -2;
  if (n < 0 || path_cap < 1 || !d_cells || !d_len || !d_total || !d_turns || !d_bad) {
    failmsg(h, "pf_turn_paths: bad arguments (n >= 0, path_cap >= 1; the rows, the lengths, the totals, the turn counts and the step indices must not be null)");
    return -1;
  }
  if (turn_weight_check(h, "pf_turn_paths", turn_weight)) return -1;
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_turn_paths_one_wave_per_row, dim3((unsigned)n), dim3(64), 0, h->stream, d_cost, turn_weight, h->RC, h->C, (int)n, (int)path_cap,
                         (const int*)d_cells, (const int*)d_len, d_total, (int*)d_turns, (int*)d_bad);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Visibility fields: what each viewpoint sees, exposure counts and the exposure of path rows (pf_visibility.h).
// The rule is the smoothing section's, one-to-all.  The occupancy is read at call time (pf_update_grid keeps working); the
// viewpoints and the info keys of a call live in the distance fields' control block, and nothing in it outlives the call.
// ---------------------------------------------------------------------------
#include "pf_visibility.h"

// The checks of the two one-to-all calls, then the call's view of the control block: n64 zeroed 64-bit words in front, the
// viewpoints behind them.
static int visibility_views(pf_handle* h, const std::string& me, int max_range_sq, int K, const int32_t* view, const void* d_out, size_t n64,
                            unsigned long long*& keys, int*& d_view) {
  if (K < 1) return failmsg(h, me + ": bad arguments (K = " + std::to_string(K) + ": at least one viewpoint is needed)");
  if (max_range_sq < -1) return failmsg(h, me + ": bad arguments (max_range_sq = " + std::to_string(max_range_sq) + ": -1 means no limit, else >= 0)");
  if (!view || !d_out) return failmsg(h, me + ": bad arguments (the viewpoints and the output must not be null)");
  if ((long long)h->R * h->R + (long long)h->C * h->C >= 0x7FFFFFFFll) return failmsg(h, me + ": bad arguments (R^2 + C^2 must stay below 2^31 - 1)");
  for (int k = 0; k < K; ++k)
    if (view[k] < 0 || view[k] >= h->RC)
      return failmsg(h, me + ": viewpoint " + std::to_string(k) + " = " + std::to_string(view[k]) + " lies outside the grid");
  CK(hipSetDevice(h->device));
  if (scratch(h, me, h->d_df_ctl, &h->df_ctl_bytes, std::max<size_t>(sizeof(unsigned long long) * n64 + sizeof(int) * (size_t)K, 256), "the viewpoints", false)) return -2;
  keys = (unsigned long long*)h->d_df_ctl;                            // (in front: 8-byte aligned)
  d_view = (int*)(keys + n64);
  CK(hipMemcpyAsync(d_view, view, sizeof(int) * (size_t)K, hipMemcpyHostToDevice, h->stream));
  CK(hipStreamSynchronize(h->stream));                                // (view is pageable and the caller's)
  return 0;
}

extern "C" {

int pf_visibility_field(pf_handle* h, int32_t restrict_corner, int32_t max_range_sq, int32_t K, const int32_t* view, uint8_t* d_seen, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_visibility_field");
  auto run = [&]() -> int {
    unsigned long long* keys = nullptr;
    int* d_view = nullptr;
    if (const int rc = visibility_views(h, me, max_range_sq, K, view, d_seen, 2 * (size_t)(K > 0 ? K : 0), keys, d_view)) return rc;
    const int RC = h->RC, C = h->C;
    const unsigned gy = (unsigned)(K < 65535 ? K : 65535);
    return timed(h, [&]() -> int {
#if PF_VIS_WAVE_PER_TARGET
      hipLaunchKernelGGL(k_visibility_field_wave_per_target, dim3(((unsigned)RC + PF_VIS_THREADS / 64 - 1) / (PF_VIS_THREADS / 64), gy), dim3(PF_VIS_THREADS), 0, h->stream,
                         (const uint8_t*)h->d_occ, RC, C, restrict_corner ? 1 : 0, (int)max_range_sq, (int)K, (const int*)d_view, d_seen);
#else
      hipLaunchKernelGGL(k_visibility_field_lane_per_target, dim3(((unsigned)RC + PF_VIS_THREADS - 1) / PF_VIS_THREADS, gy), dim3(PF_VIS_THREADS), 0, h->stream,
                         (const uint8_t*)h->d_occ, RC, C, restrict_corner ? 1 : 0, (int)max_range_sq, (int)K, (const int*)d_view, d_seen);
#endif
      if (d_info) {
        CK(hipMemsetAsync(keys, 0, sizeof(unsigned long long) * 2 * (size_t)K, h->stream));
        const unsigned nb = ((unsigned)RC + PF_VIS_THREADS - 1) / PF_VIS_THREADS;
        hipLaunchKernelGGL(k_visibility_field_info_reduce, dim3(nb < 256u ? nb : 256u, gy), dim3(PF_VIS_THREADS), 0, h->stream, (const uint8_t*)d_seen, RC, C, (int)K,
                           (const int*)d_view, keys);
        hipLaunchKernelGGL(k_visibility_field_write_info, dim3(((unsigned)K + PF_VIS_THREADS - 1) / PF_VIS_THREADS), dim3(PF_VIS_THREADS), 0, h->stream, (int)K,
                           (const unsigned long long*)keys, (long long*)d_info);
      }
      return 0;
    });
  };
  return run() ? -1 : 0;
}

int pf_visibility_count(pf_handle* h, int32_t restrict_corner, int32_t max_range_sq, int32_t K, const int32_t* view, int32_t* d_count, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_visibility_count");
  auto run = [&]() -> int {
    unsigned long long* ctl = nullptr;
    int* d_view = nullptr;
    if (const int rc = visibility_views(h, me, max_range_sq, K, view, d_count, 4, ctl, d_view)) return rc;
    const int RC = h->RC, C = h->C;
    const int per = vis_count_per(RC, K);
    const unsigned chunks = (unsigned)((K + per - 1) / per);
    const unsigned nb = ((unsigned)RC + PF_VIS_THREADS - 1) / PF_VIS_THREADS;
    return timed(h, [&]() -> int {
      CK(hipMemsetAsync(d_count, 0, sizeof(int) * (size_t)RC, h->stream));
      hipLaunchKernelGGL(k_visibility_count_lanes_on_targets, dim3(nb, chunks < 65535u ? chunks : 65535u), dim3(PF_VIS_THREADS), 0, h->stream, (const uint8_t*)h->d_occ, RC, C,
                         restrict_corner ? 1 : 0, (int)max_range_sq, (int)K, per, (const int*)d_view, (int*)d_count);
      if (d_info) {
        CK(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 4, h->stream));
        hipLaunchKernelGGL(k_visibility_count_info_reduce, dim3(nb < 1024u ? nb : 1024u), dim3(PF_VIS_THREADS), 0, h->stream, (const uint8_t*)h->d_occ, (const int*)d_count, RC,
                           ctl);
        hipLaunchKernelGGL(k_visibility_count_write_info, dim3(1), dim3(64), 0, h->stream, (const unsigned long long*)ctl, (long long*)d_info);
      }
      return 0;
    });
  };
  return run() ? -1 : 0;
}

int pf_visibility_paths(pf_handle* h, const int32_t* d_count, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, int64_t* d_out,
                        int32_t* d_profile, int32_t* d_status) {
  if (!h) return -2;
  if (n < 0 || path_cap < 1 || !d_count || !d_cells || !d_len || !d_out || !d_status) {
    failmsg(h, "pf_visibility_paths: bad arguments (n >= 0, path_cap >= 1; the counts, the rows, the lengths, the results and the statuses must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_visibility_paths_one_wave_per_row, dim3((unsigned)n), dim3(64), 0, h->stream, (const int*)d_count, h->RC, (int)n, (int)path_cap, (const int*)d_cells,
                         (const int*)d_len, (long long*)d_out, (int*)d_profile, (int*)d_status);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Space-time fields: arrival ticks and routes among moving obstacles (pf_spacetime.h).  The dynamic planes are the
// caller's buffer; the static occupancy is read at call time (pf_update_grid keeps working).  Scratch: the source table in the
// distance fields' control block; the static bit plane and, where the live planes do not fit LDS, three planes per workgroup
// in the tile-queue block.  Nothing in either outlives a call.
// ---------------------------------------------------------------------------
#include "pf_spacetime.h"

#define PF_STF_T_MAX (1 << 20)

static std::string spacetime_horizon(const std::string& me, int T) {
  return me + ": bad arguments (T = " + std::to_string(T) + ": the horizon must lie in [0, 2^20])";
}

extern "C" {

int pf_spacetime_stamp(pf_handle* h, int32_t T, uint64_t* d_occ, int32_t n, int32_t path_cap, const int32_t* d_cells, const int32_t* d_len, const int32_t* d_t0,
                       int32_t after_end, int32_t corners, int32_t clear, int32_t* d_status) {
  if (!h) return -2;
  const std::string me("pf_spacetime_stamp");
  if (T < 0 || T > PF_STF_T_MAX) { failmsg(h, spacetime_horizon(me, T)); return -1; }
  if (n < 0 || path_cap < 1 || !d_occ || !d_cells || !d_len || !d_status) {
    failmsg(h, me + ": bad arguments (n >= 0, path_cap >= 1; the planes, the rows, the lengths and the statuses must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    const int Wc = (h->C + 63) / 64;
    return timed(h, [&]() -> int {
      if (clear) CK(hipMemsetAsync(d_occ, 0, sizeof(uint64_t) * ((size_t)T + 1) * (size_t)h->R * (size_t)Wc, h->stream));
      hipLaunchKernelGGL(k_spacetime_stamp_one_wave_per_row, dim3((unsigned)n), dim3(64), 0, h->stream, (st_u64*)d_occ, h->R, h->C, Wc, (int)T, (int)n, (int)path_cap,
                         (const int*)d_cells, (const int*)d_len, (const int*)d_t0, after_end ? 1 : 0, corners ? 1 : 0, (int*)d_status);
      return 0;
    });
  };
  return run() ? -1 : 0;
}

int pf_spacetime_field(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t T, const uint64_t* d_occ, int32_t B, const int32_t* set_off, const int32_t* src,
                       int32_t* d_arrive, uint64_t* d_reach, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_spacetime_field");
  auto run = [&]() -> int {
    if (B < 1) return failmsg(h, me + ": bad arguments (B = " + std::to_string(B) + ": at least one source set is needed)");
    if (T < 0 || T > PF_STF_T_MAX) return failmsg(h, spacetime_horizon(me, T));
    if (!d_occ || !set_off || !d_arrive) return failmsg(h, me + ": bad arguments (the planes, the set offsets and the arrival rows must not be null)");
    if (set_off[0] != 0) return failmsg(h, me + ": bad arguments (the set offsets must start at 0)");
    for (int b = 0; b < B; ++b)
      if (set_off[b + 1] < set_off[b]) return failmsg(h, me + ": bad arguments (the offsets of set " + std::to_string(b) + " decrease)");
    const int ns = set_off[B];
    if (ns > 0 && !src) return failmsg(h, me + ": bad arguments (the sources must not be null)");
    for (int i = 0; i < ns; ++i)
      if (src[i] < 0 || src[i] >= h->RC) return failmsg(h, me + ": source " + std::to_string(i) + " = " + std::to_string(src[i]) + " lies outside the grid");
    CK(hipSetDevice(h->device));
    const int R = h->R, C = h->C, Wc = (C + 63) / 64, W = R * Wc;
    const size_t plane = sizeof(st_u64) * (size_t)W;
    const bool lds = PF_STF_LDS_BYTES > 0 && 3 * plane <= (size_t)PF_STF_LDS_BYTES;
    int G = std::min<int>(B, cus(h));
    if (!lds) {                                                       // three planes per workgroup in HBM: at most 1 GiB of them
      const size_t fit = ((size_t)1 << 30) / (3 * plane);
      if ((size_t)G > fit) G = fit < 1 ? 1 : (int)fit;
    }
    if (scratch(h, me, h->d_df_ctl, &h->df_ctl_bytes, sizeof(int) * std::max<size_t>((size_t)B + 1 + (size_t)ns, 64), "the source table", false)) return -2;
    if (scratch(h, me, h->d_widest, &h->widest_bytes, plane * (1 + (lds ? 0 : 3 * (size_t)G)), "the live planes", true)) return -2;
    int* const d_off = h->d_df_ctl;
    int* const d_src = d_off + B + 1;
    CK(hipMemcpyAsync(d_off, set_off, sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice, h->stream));
    if (ns) CK(hipMemcpyAsync(d_src, src, sizeof(int) * (size_t)ns, hipMemcpyHostToDevice, h->stream));
    CK(hipStreamSynchronize(h->stream));                              // (the arrays are pageable and the caller's)
    st_u64* const d_S = (st_u64*)h->d_widest;
    const unsigned nt = (unsigned)std::min<int>(PF_STF_THREADS, (W + 63) / 64 * 64);
    return timed(h, [&] {
      hipLaunchKernelGGL(k_spacetime_pack_static, dim3(((unsigned)W + 255) / 256), dim3(256), 0, h->stream, (const uint8_t*)h->d_occ, R, C, Wc, d_S);
      if (lds)
        hipLaunchKernelGGL(k_spacetime_field_group_per_set<true>, dim3((unsigned)G), dim3(nt), 3 * plane, h->stream, (const st_u64*)d_S, (const st_u64*)d_occ, R, C, Wc, (int)T,
                           allow_diag ? 1 : 0, restrict_corner ? 1 : 0, (int)B, (const int*)d_off, (const int*)d_src, (int*)d_arrive, (st_u64*)d_reach, (long long*)d_info,
                           (st_u64*)nullptr);
      else
        hipLaunchKernelGGL(k_spacetime_field_group_per_set<false>, dim3((unsigned)G), dim3(nt), 0, h->stream, (const st_u64*)d_S, (const st_u64*)d_occ, R, C, Wc, (int)T,
                           allow_diag ? 1 : 0, restrict_corner ? 1 : 0, (int)B, (const int*)d_off, (const int*)d_src, (int*)d_arrive, (st_u64*)d_reach, (long long*)d_info,
                           d_S + W);
    });
  };
  return run() ? -1 : 0;
}

int pf_spacetime_paths(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t T, const uint64_t* d_occ, int32_t B, const uint64_t* d_reach, int32_t n,
                       const int32_t* d_set_idx, const int32_t* d_target, const int32_t* d_tick, int32_t path_cap, int32_t* d_cells, int32_t* d_len, int32_t* d_status,
                       int32_t* d_tick_out) {
  if (!h) return -2;
  const std::string me("pf_spacetime_paths");
  if (T < 0 || T > PF_STF_T_MAX) { failmsg(h, spacetime_horizon(me, T)); return -1; }
  if (B < 1 || n < 0 || path_cap < 1 || !d_occ || !d_reach || !d_set_idx || !d_target || !d_cells || !d_len || !d_status) {
    failmsg(h, me + ": bad arguments (B >= 1, n >= 0, path_cap >= 1; the planes, the reach planes, the set indices, the targets, the rows, the lengths and the statuses "
                    "must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_spacetime_paths_lane_per_query, dim3(((unsigned)n + 63) / 64), dim3(64), 0, h->stream, (const uint8_t*)h->d_occ, (const st_u64*)d_occ,
                         (const st_u64*)d_reach, h->R, h->C, (h->C + 63) / 64, (int)T, allow_diag ? 1 : 0, restrict_corner ? 1 : 0, (int)B, (int)n, (const int*)d_set_idx,
                         (const int*)d_target, (const int*)d_tick, (int)path_cap, (int*)d_cells, (int*)d_len, (int*)d_status, (int*)d_tick_out);
    });
  };
  return run() ? -1 : 0;
}

int pf_spacetime_conflicts(pf_handle* h, int32_t allow_diag, int32_t restrict_corner, int32_t T, const uint64_t* d_occ, int32_t n, int32_t path_cap, const int32_t* d_cells,
                           const int32_t* d_len, const int32_t* d_t0, int32_t hold, int32_t* d_out, int32_t* d_status) {
  if (!h) return -2;
  const std::string me("pf_spacetime_conflicts");
  if (T < 0 || T > PF_STF_T_MAX) { failmsg(h, spacetime_horizon(me, T)); return -1; }
  if (n < 0 || path_cap < 1 || !d_occ || !d_cells || !d_len || !d_out || !d_status) {
    failmsg(h, me + ": bad arguments (n >= 0, path_cap >= 1; the planes, the rows, the lengths, the results and the statuses must not be null)");
    return -1;
  }
  if (n == 0) return 0;
  auto run = [&]() -> int {
    CK(hipSetDevice(h->device));
    return timed(h, [&] {
      hipLaunchKernelGGL(k_spacetime_conflicts_one_wave_per_row, dim3((unsigned)n), dim3(64), 0, h->stream, (const uint8_t*)h->d_occ, (const st_u64*)d_occ, h->R, h->C,
                         (h->C + 63) / 64, (int)T, allow_diag ? 1 : 0, restrict_corner ? 1 : 0, (int)n, (int)path_cap, (const int*)d_cells, (const int*)d_len,
                         (const int*)d_t0, hold ? 1 : 0, (int*)d_out, (int*)d_status);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Tours: the exact best order through up to 16 stops (pf_tour.h).  pf_tour_matrix gathers the stop-to-stop
// matrix out of fields in HBM; pf_tour_solve runs the Held-Karp table over B problems.  Scratch: the stops in the distance
// fields' control block; the first offending entry's index, the finite-state counters and, for m > PF_TOUR_LDS_M, the tables
// of the problems in flight in the tile-queue block.  Nothing in either outlives a call.
// ---------------------------------------------------------------------------
#include "pf_tour.h"

#define PF_TOUR_TABLE_BYTES ((size_t)256 << 20)   /* what the tables in flight may take when "tour_tables" is 0 */

long long g_tour_tables = 0;

extern "C" {

int pf_tour_matrix(pf_handle* h, int32_t n, const int32_t* stops, const double* d_fields, double* d_mat) {
  if (!h) return -2;
  const std::string me("pf_tour_matrix");
  auto run = [&]() -> int {
    if (n < 1 || n > 32768) return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": the number of stops must lie in [1, 32768])");
    if (!stops || !d_fields || !d_mat) return failmsg(h, me + ": bad arguments (the stops, the fields and the matrix must not be null)");
    for (int j = 0; j < n; ++j)
      if (stops[j] < 0 || stops[j] >= h->RC) return failmsg(h, me + ": stop " + std::to_string(j) + " = " + std::to_string(stops[j]) + " lies outside the grid");
    CK(hipSetDevice(h->device));
    if (scratch(h, me, h->d_df_ctl, &h->df_ctl_bytes, sizeof(int) * std::max<size_t>((size_t)n, 64), "the stops", false)) return -2;
    CK(hipMemcpyAsync(h->d_df_ctl, stops, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    CK(hipStreamSynchronize(h->stream));                              // (stops is pageable and the caller's)
    const long long nn = (long long)n * n;
    return timed(h, [&] {
      hipLaunchKernelGGL(k_tour_matrix_gather, dim3((unsigned)((nn + PF_TOUR_THREADS - 1) / PF_TOUR_THREADS)), dim3(PF_TOUR_THREADS), 0, h->stream, d_fields,
                         (const int*)h->d_df_ctl, h->RC, (int)n, d_mat);
    });
  };
  return run() ? -1 : 0;
}

int pf_tour_solve(pf_handle* h, int32_t mode, int32_t n, const uint32_t* need, int32_t B, const double* d_mat, double* d_total, int32_t* d_order, int32_t* d_status,
                  int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_tour_solve");
  auto run = [&]() -> int {
    if (mode < 0 || mode > 2) return failmsg(h, me + ": bad arguments (mode = " + std::to_string(mode) + ": 0 open, 1 return, 2 last)");
    if (n < 1 || (mode == 2 && n < 2))
      return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": at least " + (mode == 2 ? "two nodes are needed in mode 2)" : "one node is needed)"));
    const int m = mode == 2 ? n - 2 : n - 1;
    if (m > PF_TOUR_M_MAX)
      return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + " in mode " + std::to_string(mode) + " leaves " + std::to_string(m) +
                            " middle nodes: at most 16 are solved)");
    if (batch_args(h, me, B, "problem")) return -2;
    if (!d_mat || !d_total || !d_order || !d_status) return failmsg(h, me + ": bad arguments (the matrices, the totals, the orders and the statuses must not be null)");
    TourNeed nd;
    for (int k = 0; k < PF_TOUR_M_MAX; ++k) nd.nm[k] = 0u;
    if (need) {
      if (need[0] != 0u) return failmsg(h, me + ": bad arguments (need[0] = " + std::to_string(need[0]) + ": the start needs nothing)");
      for (int j = 0; j < n; ++j) {
        if ((need[j] >> j) & 1u) return failmsg(h, me + ": bad arguments (need[" + std::to_string(j) + "]: node " + std::to_string(j) + " needs itself)");
        if (n < 32 && (need[j] >> n) != 0u)
          return failmsg(h, me + ": bad arguments (need[" + std::to_string(j) + "] = " + std::to_string(need[j]) + " names a node >= n = " + std::to_string(n) + ")");
      }
      for (int k = 0; k < m; ++k)                                     // (the end's own needs are always met)
        nd.nm[k] = (mode == 2 && ((need[k + 1] >> (n - 1)) & 1u)) ? PF_TOUR_BLOCKED : ((need[k + 1] >> 1) & ((1u << m) - 1u));
    }
    CK(hipSetDevice(h->device));
    const int ncu = cus(h);                                           // (asked before the timed span)
    const bool lds = m >= 1 && m <= PF_TOUR_LDS_M;
    const size_t states = m >= 1 ? ((size_t)1 << m) * (size_t)m : 0;
    long long tables = 0;                                             // the problems in flight of the HBM form
    if (m >= 1 && !lds) {
      tables = g_tour_tables > 0 ? g_tour_tables : (long long)std::max<size_t>(PF_TOUR_TABLE_BYTES / (sizeof(double) * states), 1);
      tables = std::min<long long>(tables, B);
    }
    // the block: {the first bad entry, finite[tables]} in front (8-byte words), the tables behind
    if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * (1 + (size_t)tables) + sizeof(double) * states * (size_t)tables, "the tables", true))
      return -2;
    unsigned long long* const d_bad = (unsigned long long*)h->d_widest;
    unsigned long long* const d_finite = d_bad + 1;
    double* const d_tab = (double*)(d_finite + tables);
    // the entries, before any output is touched
    const long long nn = (long long)n * n, entries = nn * B;
    unsigned long long bad;
    if (arm_bad(h, d_bad)) return -2;
    CK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_tour_validate_entries, dim3((unsigned)std::min<long long>((entries + PF_TOUR_THREADS - 1) / PF_TOUR_THREADS, 2048)), dim3(PF_TOUR_THREADS), 0,
                       h->stream, d_mat, (int)n, entries, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the entry (b, i, j) = (" + std::to_string(e / nn) + ", " + std::to_string(e % nn / n) + ", " + std::to_string(e % n) +
                            ") is neither >= 0 nor +inf)");
    }
    long long* const info = (long long*)d_info;
    if (m == 0) {
      hipLaunchKernelGGL(k_tour_no_middle_nodes, dim3(((unsigned)B + 63) / 64), dim3(64), 0, h->stream, d_mat, (int)mode, (int)n, (int)B, d_total, (int*)d_order,
                         (int*)d_status, info);
    } else if (lds) {
      hipLaunchKernelGGL(k_tour_layers_in_lds_group_per_problem, dim3((unsigned)std::min<long long>(B, 8ll * ncu)), dim3(PF_TOUR_THREADS), 0, h->stream, d_mat,
                         (int)mode, (int)n, m, (int)B, nd, d_total, (int*)d_order, (int*)d_status, info);
    } else {
      const unsigned gx = (unsigned)((states + PF_TOUR_THREADS - 1) / PF_TOUR_THREADS);
      for (long long b0 = 0; b0 < B; b0 += tables) {                  // a chunk of problems: their tables, layer by layer, then the orders
        const int nb = (int)std::min<long long>(tables, B - b0);
        const double* const mat = d_mat + (size_t)b0 * (size_t)nn;
        CK(hipMemsetAsync(d_finite, 0, sizeof(unsigned long long) * (size_t)nb, h->stream));
        for (int c = 1; c <= m; ++c)
          hipLaunchKernelGGL(k_tour_layer_lane_per_state, dim3(gx, (unsigned)std::min(nb, 65535)), dim3(PF_TOUR_THREADS), 0, h->stream, mat, (int)n, m, c, nb, nd, d_tab,
                             d_finite);
        hipLaunchKernelGGL(k_tour_trace_lane_per_problem, dim3(((unsigned)nb + 63) / 64), dim3(64), 0, h->stream, mat, (int)mode, (int)n, m, nb, (const double*)d_tab,
                           (const unsigned long long*)d_finite, d_total + b0, (int*)d_order + (size_t)b0 * (size_t)n, (int*)d_status + b0,
                           info ? info + (size_t)b0 * 4 : nullptr);
      }
    }
    return timed_end(h);
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Assignments: the exact best robot-to-task matching (pf_assign.h).  pf_assign_matrix gathers a rectangular
// robot-to-task matrix out of a chunk of fields in HBM; pf_assign_solve runs the shortest-augmenting-path rule over B problems, a
// wavefront per problem up to 64 columns and a workgroup per problem above, one launch whatever B.  Scratch: the task cells in the
// distance fields' control block, the first offending entry's index in the tile-queue block.  Nothing in either outlives a call.
// ---------------------------------------------------------------------------
#include "pf_assign.h"

extern "C" {

int pf_assign_matrix(pf_handle* h, int32_t n_rows, int32_t n_cols, const int32_t* cols, const double* d_fields, int32_t row0, int32_t ld, int32_t transpose,
                     double* d_mat) {
  if (!h) return -2;
  const std::string me("pf_assign_matrix");
  auto run = [&]() -> int {
    if (n_rows < 1 || n_rows > 32768 || n_cols < 1 || n_cols > 32768)
      return failmsg(h, me + ": bad arguments (n_rows = " + std::to_string(n_rows) + ", n_cols = " + std::to_string(n_cols) + ": both must lie in [1, 32768])");
    if (row0 < 0 || row0 > 32768) return failmsg(h, me + ": bad arguments (row0 = " + std::to_string(row0) + " must lie in [0, 32768])");
    const long long need = transpose ? (long long)row0 + n_rows : (long long)n_cols;
    if ((long long)ld < need)
      return failmsg(h, me + ": bad arguments (ld = " + std::to_string(ld) + " is shorter than a row of the matrix: " + std::to_string(need) + ")");
    if (!cols || !d_fields || !d_mat) return failmsg(h, me + ": bad arguments (the cells, the fields and the matrix must not be null)");
    for (int j = 0; j < n_cols; ++j)
      if (cols[j] < 0 || cols[j] >= h->RC) return failmsg(h, me + ": cell " + std::to_string(j) + " = " + std::to_string(cols[j]) + " lies outside the grid");
    CK(hipSetDevice(h->device));
    if (scratch(h, me, h->d_df_ctl, &h->df_ctl_bytes, sizeof(int) * std::max<size_t>((size_t)n_cols, 64), "the cells", false)) return -2;
    CK(hipMemcpyAsync(h->d_df_ctl, cols, sizeof(int) * (size_t)n_cols, hipMemcpyHostToDevice, h->stream));
    CK(hipStreamSynchronize(h->stream));                              // (cols is pageable and the caller's)
    const long long nn = (long long)n_rows * n_cols;
    return timed(h, [&] {
      hipLaunchKernelGGL(k_assign_matrix_gather, dim3((unsigned)((nn + PF_ASSIGN_GATHER_THREADS - 1) / PF_ASSIGN_GATHER_THREADS)), dim3(PF_ASSIGN_GATHER_THREADS), 0,
                         h->stream, d_fields, (const int*)h->d_df_ctl, h->RC, (int)n_rows, (int)n_cols, (int)row0, (int)ld, transpose ? 1 : 0, d_mat);
    });
  };
  return run() ? -1 : 0;
}

int pf_assign_solve(pf_handle* h, int32_t mode, int32_t n, int32_t m, int32_t B, const double* d_mat, int32_t* d_col, double* d_value, int32_t* d_status,
                    double* d_dual, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_assign_solve");
  auto run = [&]() -> int {
    if (mode < 0 || mode > 2) return failmsg(h, me + ": bad arguments (mode = " + std::to_string(mode) + ": 0 sum, 1 max, 2 max_sum)");
    if (n < 1) return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": at least one row is needed)");
    if (m < n) return failmsg(h, me + ": bad arguments (m = " + std::to_string(m) + " < n = " + std::to_string(n) + ": rows must not outnumber columns)");
    if (m > PF_ASSIGN_MAX) return failmsg(h, me + ": bad arguments (m = " + std::to_string(m) + ": at most " + std::to_string(PF_ASSIGN_MAX) + " columns are solved)");
    if (batch_args(h, me, B, "problem")) return -2;
    if (!d_mat || !d_col || !d_value || !d_status) return failmsg(h, me + ": bad arguments (the matrices, the columns, the values and the statuses must not be null)");
    CK(hipSetDevice(h->device));
    const int ncu = cus(h);                                           // (asked before the timed span)
    if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * 8, "the entry index", false)) return -2;
    unsigned long long* const d_bad = (unsigned long long*)h->d_widest;
    // the entries, before any output is touched
    const long long nm = (long long)n * m, entries = nm * B;
    unsigned long long bad;
    if (arm_bad(h, d_bad)) return -2;
    CK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_assign_validate_entries, dim3((unsigned)std::min<long long>((entries + PF_ASSIGN_GATHER_THREADS - 1) / PF_ASSIGN_GATHER_THREADS, 2048)),
                       dim3(PF_ASSIGN_GATHER_THREADS), 0, h->stream, d_mat, entries, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the entry (b, i, j) = (" + std::to_string(e / nm) + ", " + std::to_string(e % nm / m) + ", " + std::to_string(e % m) +
                            ") is neither +inf nor finite within 2^1000)");
    }
    long long* const info = (long long*)d_info;
    if (m <= PF_ASSIGN_WAVE_M) {
      hipLaunchKernelGGL(k_assign_wave_per_problem, dim3((unsigned)(((long long)B + PF_ASSIGN_WAVES - 1) / PF_ASSIGN_WAVES)), dim3(64 * PF_ASSIGN_WAVES), 0, h->stream, d_mat,
                         (int)mode, (int)n, (int)m, (int)B, (int*)d_col, d_value, (int*)d_status, d_dual, info);
    } else {
      const long long groups = (long long)(PF_ASSIGN_THREADS == 256 ? 8 : 2) * ncu;
      hipLaunchKernelGGL(k_assign_group_per_problem<PF_ASSIGN_THREADS>, dim3((unsigned)std::min<long long>(B, groups)), dim3(PF_ASSIGN_THREADS), 0, h->stream, d_mat,
                         (int)mode, (int)n, (int)m, (int)B, (int*)d_col, d_value, (int*)d_status, d_dual, info);
    }
    return timed_end(h);
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Tour search: best-improvement 2-opt over up to 1024 stops (pf_tour_search.h).  pf_tour_improve takes B start
// orders over one shared matrix or over B matrices, checks the entries and the start rows with two validation kernels, and runs
// the move loops in one launch, a workgroup per start.  Scratch: the first offending index and the matrices' "holds +inf" words in
// the tile-queue block (h->d_widest, h->widest_bytes).  Nothing in it outlives a call.
// ---------------------------------------------------------------------------
#include "pf_tour_search.h"

extern "C" {

int pf_tour_improve(pf_handle* h, int32_t mode, int32_t n, int32_t B, int32_t shared, const double* d_mat, int32_t max_moves, int32_t* d_order, double* d_value,
                    int32_t* d_status, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_tour_improve");
  auto run = [&]() -> int {
    if (mode < 0 || mode > 2) return failmsg(h, me + ": bad arguments (mode = " + std::to_string(mode) + ": 0 open, 1 return, 2 last)");
    if (n < 1 || n > PF_TOUR_SEARCH_MAX)
      return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": the number of nodes must lie in [1, " + std::to_string(PF_TOUR_SEARCH_MAX) + "])");
    if (batch_args(h, me, B, "start", shared, max_moves)) return -2;
    if (!d_mat || !d_order || !d_value || !d_status) return failmsg(h, me + ": bad arguments (the matrices, the orders, the values and the statuses must not be null)");
    CK(hipSetDevice(h->device));
    const int ncu = cus(h);                                           // (asked before the timed span)
    const long long mats = shared ? 1 : (long long)B;
    // the block: {the first bad index, a spare word} in front, the matrices' "holds +inf" words behind
    if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * 2 + sizeof(int) * (size_t)mats, "the entry index", false)) return -2;
    unsigned long long* const d_bad = (unsigned long long*)h->d_widest;
    int* const d_inf = (int*)(d_bad + 2);
    const long long nn = (long long)n * n, entries = nn * mats;
    unsigned long long bad;
    if (arm_bad(h, d_bad, d_inf, (size_t)mats)) return -2;
    CK(hipEventRecord(h->ev0, h->stream));
    // the entries, then the start rows, before any output is touched
    hipLaunchKernelGGL(k_tour_search_validate_entries, dim3((unsigned)std::min<long long>((entries + PF_TOUR_SEARCH_THREADS - 1) / PF_TOUR_SEARCH_THREADS, 2048)),
                       dim3(PF_TOUR_SEARCH_THREADS), 0, h->stream, d_mat, (int)n, entries, d_bad, d_inf);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the entry (b, i, j) = (" + std::to_string(e / nn) + ", " + std::to_string(e % nn / n) + ", " + std::to_string(e % n) +
                            ") is neither +inf nor a number in [0, 2^1000])");
    }
    hipLaunchKernelGGL(k_tour_search_validate_orders, dim3((unsigned)std::min<long long>(B, 8ll * ncu)), dim3(PF_TOUR_SEARCH_THREADS), 0, h->stream,
                       (const int*)d_order, (int)mode, (int)n, (int)B, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the start (b, position) = (" + std::to_string(e / n) + ", " + std::to_string(e % n) +
                            ") is no permutation of the nodes with node 0 first" + (mode == 2 ? " and node n - 1 last)" : ")"));
    }
    long long* const info = (long long*)d_info;
    const long long groups = (long long)(32 * 64 / PF_TOUR_SEARCH_GROUP) * ncu;               // what is resident at once
    hipLaunchKernelGGL(k_tour_search_group_per_start, dim3((unsigned)std::min<long long>(B, groups)), dim3(PF_TOUR_SEARCH_GROUP), 0, h->stream, d_mat, (const int*)d_inf,
                       (int)mode, (int)n, (int)B, (int)shared, (int)max_moves, (int*)d_order, d_value, (int*)d_status, info);
    return timed_end(h);
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Fleet routes: best-improvement 2-opt and segment relocation over k robots and n tasks (pf_fleet.h).
// pf_fleet_improve takes B start rows over one shared matrix or over B matrices, checks the entries, the rows and the capacities
// with validation kernels, and runs the move loops in one launch, a workgroup per start.  Scratch: the first offending index and
// the matrices' "holds +inf" words in the tile-queue block (h->d_widest, h->widest_bytes).  Nothing in it outlives a call.
// pf_fleet_balance (pf_fleet_balance.h) is the same call with the move loop of the min-max rule: the argument
// checks, the validation kernels and the launch geometry are one function, fleet_call, that takes the kernel.
// ---------------------------------------------------------------------------
#include "pf_fleet_balance.h"

using fleet_kernel = void (*)(const double*, const int*, const int*, int, int, int, int, int, int, int*, double*, double*, int*, long long*);

static int fleet_call(pf_handle* h, const std::string& me, fleet_kernel kernel, int32_t mode, int32_t k, int32_t n, int32_t B, int32_t shared, const double* d_mat,
                      const int32_t* d_cap, int32_t max_moves, int32_t* d_route, double* d_len, double* d_value, int32_t* d_status, int64_t* d_info) {
  if (!h) return -2;
  auto run = [&]() -> int {
    if (mode < 0 || mode > 1) return failmsg(h, me + ": bad arguments (mode = " + std::to_string(mode) + ": 0 open, 1 return)");
    if (k < 1) return failmsg(h, me + ": bad arguments (k = " + std::to_string(k) + ": at least one robot is needed)");
    if (n < 1) return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": at least one task is needed)");
    if ((long long)k + (long long)n > PF_FLEET_MAX)
      return failmsg(h, me + ": bad arguments (k + n = " + std::to_string((long long)k + (long long)n) + ": robots and tasks together must not exceed " +
                            std::to_string(PF_FLEET_MAX) + ")");
    if (batch_args(h, me, B, "start", shared, max_moves)) return -2;
    if (!d_mat || !d_route || !d_len || !d_value || !d_status)
      return failmsg(h, me + ": bad arguments (the matrices, the routes, the lengths, the values and the statuses must not be null)");
    CK(hipSetDevice(h->device));
    const int N = k + n;
    if (d_cap) {                                // the capacities are k words: read back and checked on the host before any launch
      std::vector<int32_t> cap((size_t)k);
      CK(hipMemcpyAsync(cap.data(), d_cap, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, h->stream));
      CK(hipStreamSynchronize(h->stream));
      h->d2h_small += 1;
      for (int r = 0; r < k; ++r)
        if (cap[(size_t)r] < 0) return failmsg(h, me + ": bad arguments (cap[" + std::to_string(r) + "] = " + std::to_string(cap[(size_t)r]) + " is negative)");
    }
    const int ncu = cus(h);                                           // (asked before the timed span)
    const long long mats = shared ? 1 : (long long)B;
    // the block: {the first bad index, a spare word} in front, the matrices' "holds +inf" words behind
    if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * 2 + sizeof(int) * (size_t)mats, "the entry index", false)) return -2;
    unsigned long long* const d_bad = (unsigned long long*)h->d_widest;
    int* const d_inf = (int*)(d_bad + 2);
    const long long nn = (long long)N * N, entries = nn * mats;
    unsigned long long bad;
    if (arm_bad(h, d_bad, d_inf, (size_t)mats)) return -2;
    CK(hipEventRecord(h->ev0, h->stream));
    // the entries, then the start rows, then the capacities, before any output is touched
    const dim3 rows_grid((unsigned)std::min<long long>(B, 8ll * ncu));
    hipLaunchKernelGGL(k_fleet_validate_entries, dim3((unsigned)std::min<long long>((entries + PF_FLEET_THREADS - 1) / PF_FLEET_THREADS, 2048)), dim3(PF_FLEET_THREADS), 0,
                       h->stream, d_mat, (int)k, N, entries, d_bad, d_inf);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the entry (b, i, j) = (" + std::to_string(e / nn) + ", " + std::to_string(e % nn / N) + ", " + std::to_string(e % N) +
                            ") is neither +inf nor a number in [0, 2^1000])");
    }
    hipLaunchKernelGGL(k_fleet_validate_rows, rows_grid, dim3(PF_FLEET_THREADS), 0, h->stream, (const int*)d_route, (int)k, N, (int)B, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the start (b, position) = (" + std::to_string(e / N) + ", " + std::to_string(e % N) +
                            ") is no permutation of the nodes with node 0 first and the robots in increasing order)");
    }
    if (d_cap) {
      hipLaunchKernelGGL(k_fleet_validate_caps, rows_grid, dim3(PF_FLEET_THREADS), 0, h->stream, (const int*)d_route, (const int*)d_cap, (int)k, N, (int)B, d_bad);
      if (first_bad(h, d_bad, bad)) return -2;
      if (bad != ~0ull) {
        const long long e = (long long)bad;
        return failmsg(h, me + ": bad arguments (the start (b, robot) = (" + std::to_string(e / k) + ", " + std::to_string(e % k) + ") holds more tasks than its capacity)");
      }
    }
    long long* const info = (long long*)d_info;
    const long long groups = (long long)(32 * 64 / PF_FLEET_GROUP) * ncu;                    // what is resident at once
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<long long>(B, groups)), dim3(PF_FLEET_GROUP), 0, h->stream, d_mat, (const int*)d_inf, (const int*)d_cap, (int)mode,
                       (int)k, N, (int)B, (int)shared, (int)max_moves, (int*)d_route, d_len, d_value, (int*)d_status, info);
    return timed_end(h);
  };
  return run() ? -1 : 0;
}

extern "C" {

int pf_fleet_improve(pf_handle* h, int32_t mode, int32_t k, int32_t n, int32_t B, int32_t shared, const double* d_mat, const int32_t* d_cap, int32_t max_moves,
                     int32_t* d_route, double* d_len, double* d_value, int32_t* d_status, int64_t* d_info) {
  return fleet_call(h, "pf_fleet_improve", k_fleet_group_per_start, mode, k, n, B, shared, d_mat, d_cap, max_moves, d_route, d_len, d_value, d_status, d_info);
}

int pf_fleet_balance(pf_handle* h, int32_t mode, int32_t k, int32_t n, int32_t B, int32_t shared, const double* d_mat, const int32_t* d_cap, int32_t max_moves,
                     int32_t* d_route, double* d_len, double* d_value, int32_t* d_status, int64_t* d_info) {
  return fleet_call(h, "pf_fleet_balance", k_fleet_balance_group_per_start, mode, k, n, B, shared, d_mat, d_cap, max_moves, d_route, d_len, d_value, d_status, d_info);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Placement: which p of m candidate sites to open for n demands (pf_place.h).  pf_place_improve takes B start
// rows over one shared matrix or over B matrices, checks the entries and the rows with two validation kernels, and runs the move
// loops in one launch, a workgroup per start.  Scratch: the first offending index in the tile-queue block (h->d_widest,
// h->widest_bytes).  Nothing in it outlives a call.
// ---------------------------------------------------------------------------
#include "pf_place.h"

extern "C" {

int pf_place_improve(pf_handle* h, int32_t mode, int32_t m, int32_t n, int32_t p, int32_t fixed, int32_t B, int32_t shared, const double* d_mat, int32_t max_moves,
                     int32_t* d_sel, int32_t* d_owner, double* d_value, int32_t* d_status, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_place_improve");
  auto run = [&]() -> int {
    if (mode < 0 || mode > 1) return failmsg(h, me + ": bad arguments (mode = " + std::to_string(mode) + ": 0 sum, 1 max)");
    if (m < 1 || m > PF_PLACE_SITES_MAX)
      return failmsg(h, me + ": bad arguments (m = " + std::to_string(m) + ": the number of sites must lie in [1, " + std::to_string(PF_PLACE_SITES_MAX) + "])");
    if (n < 1 || n > PF_PLACE_DEMANDS_MAX)
      return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": the number of demands must lie in [1, " + std::to_string(PF_PLACE_DEMANDS_MAX) + "])");
    if (p < 1 || p > std::min<int>(m, PF_PLACE_OPEN_MAX))
      return failmsg(h, me + ": bad arguments (p = " + std::to_string(p) + ": the number of slots must lie in [1, min(m, " + std::to_string(PF_PLACE_OPEN_MAX) + ")])");
    if (fixed < 0 || fixed > p) return failmsg(h, me + ": bad arguments (fixed = " + std::to_string(fixed) + " must lie in [0, p])");
    if (batch_args(h, me, B, "start", shared, max_moves)) return -2;
    if (!d_mat || !d_sel || !d_value || !d_status) return failmsg(h, me + ": bad arguments (the matrices, the rows, the values and the statuses must not be null)");
    CK(hipSetDevice(h->device));
    const int ncu = cus(h);                                           // (asked before the timed span)
    if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * 2, "the entry index", false)) return -2;
    unsigned long long* const d_bad = (unsigned long long*)h->d_widest;
    const long long mn = (long long)m * n, entries = mn * (shared ? 1 : (long long)B), slots = (long long)B * p;
    unsigned long long bad;
    if (arm_bad(h, d_bad)) return -2;
    CK(hipEventRecord(h->ev0, h->stream));
    // the entries, then the rows, before any output is touched
    hipLaunchKernelGGL(k_place_validate_entries, dim3((unsigned)std::min<long long>((entries + PF_PLACE_THREADS - 1) / PF_PLACE_THREADS, 2048)), dim3(PF_PLACE_THREADS), 0,
                       h->stream, d_mat, entries, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the entry (b, i, j) = (" + std::to_string(e / mn) + ", " + std::to_string(e % mn / n) + ", " + std::to_string(e % n) +
                            ") is neither +inf nor a number in [+0.0, 2^1000])");
    }
    hipLaunchKernelGGL(k_place_validate_rows, dim3((unsigned)std::min<long long>((slots + PF_PLACE_THREADS - 1) / PF_PLACE_THREADS, 2048)), dim3(PF_PLACE_THREADS), 0,
                       h->stream, (const int*)d_sel, (int)m, (int)p, (int)fixed, slots, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the row (b, slot) = (" + std::to_string(e / p) + ", " + std::to_string(e % p) +
                            ") lies outside [-1, m), repeats the site of a smaller slot or is empty below fixed)");
    }
    const size_t lds = (size_t)n * (2 * sizeof(double) + 1);          // d1, d2 and n1 per demand
    CK(hipFuncSetAttribute((const void*)k_place_group_per_start, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_place_group_per_start, dim3((unsigned)std::min<long long>(B, 2ll * ncu)), dim3(PF_PLACE_GROUP), lds, h->stream, d_mat, (int)mode, (int)m,
                       (int)n, (int)p, (int)fixed, (int)B, (int)shared, (int)max_moves, (int*)d_sel, (int*)d_owner, d_value, (int*)d_status, (long long*)d_info);
    return timed_end(h);
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Coverage: which p of m sites see or reach the most of n elements (pf_cover.h).  pf_cover_pack turns a chunk of
// visibility rows (bytes) or field rows (doubles) in HBM into rows of the bit masks, 64 targets a word; pf_cover_improve takes B
// start rows over one shared mask set or over B of them, checks the tail bits and the rows with two validation kernels, and runs
// the move loops in one launch, a workgroup per start.  Scratch: the first offending index and, where the two planes of a start
// do not fit LDS, a block of 2 W words per workgroup (one workgroup a CU then), both in the tile-queue block (h->d_widest, h->widest_bytes).  Nothing in it
// outlives a call.
// ---------------------------------------------------------------------------
#include "pf_cover.h"

extern "C" {

int pf_cover_pack(pf_handle* h, int32_t kind, int32_t K, int32_t n, const void* d_src, int32_t ld, const int32_t* d_targets, double radius, int32_t row0,
                  uint64_t* d_mask) {
  if (!h) return -2;
  const std::string me("pf_cover_pack");
  auto run = [&]() -> int {
    if (kind < 0 || kind > 1) return failmsg(h, me + ": bad arguments (kind = " + std::to_string(kind) + ": 0 bytes != 0, 1 doubles <= radius)");
    if (K < 1 || K > PF_COVER_SITES_MAX)
      return failmsg(h, me + ": bad arguments (K = " + std::to_string(K) + ": the number of source rows must lie in [1, " + std::to_string(PF_COVER_SITES_MAX) + "])");
    if (n < 1 || n > PF_COVER_ELEMS_MAX)
      return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": the number of elements must lie in [1, " + std::to_string(PF_COVER_ELEMS_MAX) + "])");
    if (ld < 1) return failmsg(h, me + ": bad arguments (ld = " + std::to_string(ld) + ": a source row holds at least one entry)");
    if (row0 < 0 || (long long)row0 + K > PF_COVER_SITES_MAX)
      return failmsg(h, me + ": bad arguments (row0 = " + std::to_string(row0) + ", K = " + std::to_string(K) + ": the rows must lie in [0, " +
                            std::to_string(PF_COVER_SITES_MAX) + "])");
    if (kind == 1 && !(radius >= 0.0 && radius < std::numeric_limits<double>::infinity()))
      return failmsg(h, me + ": bad arguments (radius = " + std::to_string(radius) + " must be finite and >= 0)");
    if (!d_src || !d_targets || !d_mask) return failmsg(h, me + ": bad arguments (the source rows, the targets and the masks must not be null)");
    CK(hipSetDevice(h->device));
    if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * 2, "the target index", false)) return -2;
    unsigned long long* const d_bad = (unsigned long long*)h->d_widest;
    unsigned long long bad;
    if (arm_bad(h, d_bad)) return -2;
    CK(hipEventRecord(h->ev0, h->stream));
    // the targets, before any source entry is read
    hipLaunchKernelGGL(k_cover_validate_targets, dim3((unsigned)std::min<long long>(((long long)n + PF_COVER_THREADS - 1) / PF_COVER_THREADS, 2048)), dim3(PF_COVER_THREADS), 0,
                       h->stream, (const int*)d_targets, (int)n, (int)ld, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) return failmsg(h, me + ": bad arguments (target " + std::to_string((long long)bad) + " lies outside [0, ld))");
    const int W = (n + 63) / 64, per = PF_COVER_THREADS / 64;
    const dim3 grid((unsigned)((W + per - 1) / per), (unsigned)K);
    if (kind == 0)
      hipLaunchKernelGGL(k_cover_pack<0>, grid, dim3(PF_COVER_THREADS), 0, h->stream, d_src, (const int*)d_targets, (int)n, (int)ld, radius, (int)row0,
                         (unsigned long long*)d_mask);
    else
      hipLaunchKernelGGL(k_cover_pack<1>, grid, dim3(PF_COVER_THREADS), 0, h->stream, d_src, (const int*)d_targets, (int)n, (int)ld, radius, (int)row0,
                         (unsigned long long*)d_mask);
    return timed_end(h);
  };
  return run() ? -1 : 0;
}

int pf_cover_improve(pf_handle* h, int32_t m, int32_t n, int32_t p, int32_t fixed, int32_t B, int32_t shared, const uint64_t* d_mask, int32_t max_moves, int32_t* d_sel,
                     uint64_t* d_covered, int64_t* d_value, int32_t* d_status, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_cover_improve");
  auto run = [&]() -> int {
    if (m < 1 || m > PF_COVER_SITES_MAX)
      return failmsg(h, me + ": bad arguments (m = " + std::to_string(m) + ": the number of sites must lie in [1, " + std::to_string(PF_COVER_SITES_MAX) + "])");
    if (n < 1 || n > PF_COVER_ELEMS_MAX)
      return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ": the number of elements must lie in [1, " + std::to_string(PF_COVER_ELEMS_MAX) + "])");
    if (p < 1 || p > std::min<int>(m, PF_COVER_OPEN_MAX))
      return failmsg(h, me + ": bad arguments (p = " + std::to_string(p) + ": the number of slots must lie in [1, min(m, " + std::to_string(PF_COVER_OPEN_MAX) + ")])");
    if (fixed < 0 || fixed > p) return failmsg(h, me + ": bad arguments (fixed = " + std::to_string(fixed) + " must lie in [0, p])");
    if (batch_args(h, me, B, "start", shared, max_moves, "mask set")) return -2;
    if (!d_mask || !d_sel || !d_value || !d_status) return failmsg(h, me + ": bad arguments (the masks, the rows, the values and the statuses must not be null)");
    CK(hipSetDevice(h->device));
    const int W = (n + 63) / 64;
    const bool lds = W <= PF_COVER_LDS_WORDS;
    // two workgroups a CU in the LDS form; the HBM form's registers leave room for one, so a second half of the grid would only queue
    const long long G = std::min<long long>(B, (lds ? 2ll : 1ll) * cus(h));
    const size_t plane_bytes = lds ? 0 : sizeof(unsigned long long) * 2 * (size_t)W * (size_t)G;
    if (scratch(h, me, h->d_widest, &h->widest_bytes, sizeof(unsigned long long) * 2 + plane_bytes, "the planes", true)) return -2;
    unsigned long long* const d_bad = (unsigned long long*)h->d_widest;
    const long long rows = (long long)m * (shared ? 1 : (long long)B), slots = (long long)B * p;
    unsigned long long bad;
    if (arm_bad(h, d_bad)) return -2;
    CK(hipEventRecord(h->ev0, h->stream));
    // the tail bits, then the rows, before any output is touched
    hipLaunchKernelGGL(k_cover_validate_tail, dim3((unsigned)std::min<long long>((rows + PF_COVER_THREADS - 1) / PF_COVER_THREADS, 2048)), dim3(PF_COVER_THREADS), 0,
                       h->stream, (const unsigned long long*)d_mask, (int)n, W, rows, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the mask (b, i) = (" + std::to_string(e / m) + ", " + std::to_string(e % m) + ") holds a bit at an element >= n)");
    }
    hipLaunchKernelGGL(k_place_validate_rows, dim3((unsigned)std::min<long long>((slots + PF_PLACE_THREADS - 1) / PF_PLACE_THREADS, 2048)), dim3(PF_PLACE_THREADS), 0,
                       h->stream, (const int*)d_sel, (int)m, (int)p, (int)fixed, slots, d_bad);
    if (first_bad(h, d_bad, bad)) return -2;
    if (bad != ~0ull) {
      const long long e = (long long)bad;
      return failmsg(h, me + ": bad arguments (the row (b, slot) = (" + std::to_string(e / p) + ", " + std::to_string(e % p) +
                            ") lies outside [-1, m), repeats the site of a smaller slot or is empty below fixed)");
    }
    if (lds) {
      const size_t bytes = sizeof(unsigned long long) * 2 * (size_t)W;   // any and once
      CK(hipFuncSetAttribute((const void*)k_cover_group_per_start<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(sizeof(unsigned long long) * 2 * PF_COVER_LDS_WORDS)));   // (the most any call asks for: never shrunk between calls)
      hipLaunchKernelGGL(k_cover_group_per_start<true>, dim3((unsigned)G), dim3(PF_COVER_GROUP), bytes, h->stream, (const unsigned long long*)d_mask, (int)m, (int)n, (int)p,
                         (int)fixed, (int)B, (int)shared, (int)max_moves, (int*)d_sel, (unsigned long long*)d_covered, (long long*)d_value, (int*)d_status,
                         (long long*)d_info, (unsigned long long*)nullptr);
    } else {
      hipLaunchKernelGGL(k_cover_group_per_start<false>, dim3((unsigned)G), dim3(PF_COVER_GROUP), 0, h->stream, (const unsigned long long*)d_mask, (int)m, (int)n, (int)p,
                         (int)fixed, (int)B, (int)shared, (int)max_moves, (int*)d_sel, (unsigned long long*)d_covered, (long long*)d_value, (int*)d_status,
                         (long long*)d_info, d_bad + 2);
    }
    return timed_end(h);
  };
  return run() ? -1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The sight graph and exact any-angle shortest paths in it (pf_sight.h).  pf_sight_pack reads the handle's
// occupancy at call time (pf_update_grid keeps working); the matrix, the labels and the parents are the caller's buffers.  Scratch:
// four 64-bit words (info keys or work counters), the node list, the nodes' coordinates and the sets of a call, all in the
// distance fields' control block; nothing in it outlives a call.  The handle keeps the last field call's work counters.
// ---------------------------------------------------------------------------
#include "pf_sight.h"

// The node list of a call, checked on the host, then the call's view of the control block: four 64-bit words in front (the caller zeroes them), the
// node cells, their coordinates and `extra` ints behind them.
static int sight_nodes_check(pf_handle* h, const std::string& me, int M, const int32_t* nodes) {
  if (M < 1 || M > PF_SIGHT_NODES_MAX)
    return failmsg(h, me + ": bad arguments (M = " + std::to_string(M) + ": the number of nodes must lie in [1, " + std::to_string(PF_SIGHT_NODES_MAX) + "])");
  if (!nodes) return failmsg(h, me + ": bad arguments (the nodes must not be null)");
  if ((long long)h->R * h->R + (long long)h->C * h->C >= 0x7FFFFFFFll) return failmsg(h, me + ": bad arguments (R^2 + C^2 must stay below 2^31 - 1)");
  for (int i = 0; i < M; ++i) {
    if (nodes[i] < 0 || nodes[i] >= h->RC) return failmsg(h, me + ": node " + std::to_string(i) + " = " + std::to_string(nodes[i]) + " lies outside the grid");
    if (i > 0 && nodes[i] <= nodes[i - 1])
      return failmsg(h, me + ": node " + std::to_string(i) + " = " + std::to_string(nodes[i]) + " does not lie above node " + std::to_string(i - 1) + " = " +
                            std::to_string(nodes[i - 1]) + ": the cells must increase strictly");
  }
  return 0;
}

static int sight_nodes(pf_handle* h, const std::string& me, int M, const int32_t* nodes, size_t extra, unsigned long long*& ctl, int*& d_nodes, int*& d_rc, int*& d_extra) {
  if (sight_nodes_check(h, me, M, nodes)) return -2;
  CK(hipSetDevice(h->device));
  const size_t bytes = sizeof(unsigned long long) * 4 + sizeof(int) * (2 * (size_t)M + extra);
  if (scratch(h, me, h->d_df_ctl, &h->df_ctl_bytes, std::max<size_t>(bytes, 256), "the nodes", false)) return -2;
  ctl = (unsigned long long*)h->d_df_ctl;                             // (in front: 8-byte aligned)
  d_nodes = (int*)(ctl + 4);
  d_rc = d_nodes + M;
  d_extra = d_rc + M;
  CK(hipMemcpyAsync(d_nodes, nodes, sizeof(int) * (size_t)M, hipMemcpyHostToDevice, h->stream));
  CK(hipStreamSynchronize(h->stream));                                // (nodes is pageable and the caller's)
  return 0;
}

static int sight_matrix_args(pf_handle* h, const std::string& me, int M, const void* d_adj, int ld) {
  if (!d_adj) return failmsg(h, me + ": bad arguments (the adjacency matrix must not be null)");
  if (M >= 1 && ld < (M + 63) / 64)
    return failmsg(h, me + ": bad arguments (ld = " + std::to_string(ld) + ": a row holds at least ceil(M / 64) = " + std::to_string((M + 63) / 64) + " words)");
  return 0;
}

extern "C" {

int pf_sight_pack(pf_handle* h, int32_t restrict_corner, int32_t max_range_sq, int32_t M, const int32_t* nodes, uint64_t* d_adj, int32_t ld, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_sight_pack");
  auto run = [&]() -> int {
    if (max_range_sq < -1) return failmsg(h, me + ": bad arguments (max_range_sq = " + std::to_string(max_range_sq) + ": -1 means no limit, else >= 0)");
    if (sight_matrix_args(h, me, M, d_adj, ld)) return -2;
    unsigned long long* ctl = nullptr;
    int *d_nodes = nullptr, *d_rc = nullptr, *d_extra = nullptr;
    if (const int rc = sight_nodes(h, me, M, nodes, 0, ctl, d_nodes, d_rc, d_extra)) return rc;
    const int W = (M + 63) / 64, per = PF_SIGHT_THREADS / 64;
    return timed(h, [&]() -> int {
      hipLaunchKernelGGL(k_sight_pack_lane_per_pair, dim3((unsigned)((W + per - 1) / per), (unsigned)M), dim3(PF_SIGHT_THREADS), 0, h->stream, (const uint8_t*)h->d_occ,
                         h->C, restrict_corner ? 1 : 0, (int)max_range_sq, (int)M, (const int*)d_nodes, (unsigned long long*)d_adj, (int)ld);
      if (d_info) {
        CK(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 4, h->stream));
        const unsigned nb = (unsigned)((M + per - 1) / per);
        hipLaunchKernelGGL(k_sight_pack_info_reduce, dim3(nb < 1024u ? nb : 1024u), dim3(PF_SIGHT_THREADS), 0, h->stream, (const unsigned long long*)d_adj, (int)ld, (int)M,
                           ctl);
        hipLaunchKernelGGL(k_sight_pack_write_info, dim3(1), dim3(64), 0, h->stream, (const unsigned long long*)ctl, (long long*)d_info);
      }
      return 0;
    });
  };
  return run() ? -1 : 0;
}

int pf_sight_field(pf_handle* h, int32_t M, const int32_t* nodes, const uint64_t* d_adj, int32_t ld, int32_t B, const int32_t* set_off, const int32_t* src,
                   double* d_dist, int32_t* d_parent, int64_t* d_info) {
  if (!h) return -2;
  const std::string me("pf_sight_field");
  auto run = [&]() -> int {
    if (sight_matrix_args(h, me, M, d_adj, ld)) return -2;
    if (B < 1) return failmsg(h, me + ": bad arguments (B = " + std::to_string(B) + ": at least one source set is needed)");
    if (!set_off) return failmsg(h, me + ": bad arguments (the set offsets must not be null)");
    if (set_off[0] != 0) return failmsg(h, me + ": set_off[0] = " + std::to_string(set_off[0]) + ": the offsets must start at 0");
    for (int b = 0; b < B; ++b)
      if (set_off[b + 1] < set_off[b])
        return failmsg(h, me + ": set " + std::to_string(b) + ": set_off[" + std::to_string(b + 1) + "] = " + std::to_string(set_off[b + 1]) + " lies below set_off[" +
                              std::to_string(b) + "] = " + std::to_string(set_off[b]));
    const int total = set_off[B];
    if (total > 0 && !src) return failmsg(h, me + ": bad arguments (the sources must not be null)");
    if (!d_dist) return failmsg(h, me + ": bad arguments (the labels must not be null)");
    if (M >= 1 && M <= PF_SIGHT_NODES_MAX)
      for (int j = 0; j < total; ++j)
        if (src[j] < 0 || src[j] >= M) return failmsg(h, me + ": source " + std::to_string(j) + " = " + std::to_string(src[j]) + " lies outside [0, M)");
    unsigned long long* work = nullptr;
    int *d_nodes = nullptr, *d_rc = nullptr, *d_sets = nullptr;
    if (const int rc = sight_nodes(h, me, M, nodes, (size_t)B + 1 + (size_t)total, work, d_nodes, d_rc, d_sets)) return rc;
    CK(hipMemcpyAsync(d_sets, set_off, sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice, h->stream));
    if (total) CK(hipMemcpyAsync(d_sets + B + 1, src, sizeof(int) * (size_t)total, hipMemcpyHostToDevice, h->stream));
    CK(hipMemsetAsync(work, 0, sizeof(unsigned long long) * 4, h->stream));
    CK(hipStreamSynchronize(h->stream));                              // (the sets are pageable and the caller's)
    const bool lds = M <= PF_SIGHT_LDS_NODES;
    const unsigned G = (unsigned)std::min<long long>(B, 8ll * cus(h));
    const unsigned nb = (unsigned)((M + PF_SIGHT_THREADS - 1) / PF_SIGHT_THREADS);
    const int rc = timed(h, [&]() -> int {
      hipLaunchKernelGGL(k_sight_node_coords, dim3(nb), dim3(PF_SIGHT_THREADS), 0, h->stream, (const int*)d_nodes, (int)M, h->C, d_rc);
      if (lds) {
        CK(hipFuncSetAttribute((const void*)k_sight_field_group_per_set<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(sizeof(double) * (PF_SIGHT_LDS_NODES < PF_SIGHT_NODES_MAX ? PF_SIGHT_LDS_NODES : PF_SIGHT_NODES_MAX))));   // (the most any call asks for)
        hipLaunchKernelGGL(k_sight_field_group_per_set<true>, dim3(G), dim3(PF_SIGHT_GROUP), sizeof(double) * (size_t)M, h->stream, (const unsigned long long*)d_adj, (int)ld,
                           (int)M, (const int*)d_rc, (int)B, (const int*)d_sets, (const int*)(d_sets + B + 1), d_dist, (long long*)d_info, work);
      } else {
        hipLaunchKernelGGL(k_sight_field_group_per_set<false>, dim3(G), dim3(PF_SIGHT_GROUP), 0, h->stream, (const unsigned long long*)d_adj, (int)ld, (int)M,
                           (const int*)d_rc, (int)B, (const int*)d_sets, (const int*)(d_sets + B + 1), d_dist, (long long*)d_info, work);
      }
      if (d_parent)
        hipLaunchKernelGGL(k_sight_parents, dim3(nb, (unsigned)(B < 65535 ? B : 65535)), dim3(PF_SIGHT_THREADS), 0, h->stream, (const unsigned long long*)d_adj, (int)ld,
                           (int)M, (const int*)d_rc, (int)B, (const double*)d_dist, (int*)d_parent);
      return 0;
    });
    if (rc) return rc;
    unsigned long long w4[4];
    CK(hipMemcpyAsync(w4, work, sizeof(w4), hipMemcpyDeviceToHost, h->stream));
    CK(hipStreamSynchronize(h->stream));
    h->d2h_small += 1;
    for (int i = 0; i < 4; ++i) h->sight_work[i] = (long long)w4[i];
    return 0;
  };
  return run() ? -1 : 0;
}

int pf_sight_field_work(pf_handle* h, int64_t* out4) { return tile_work(h, "pf_sight_field_work", h ? h->sight_work : nullptr, out4); }

int pf_sight_paths(pf_handle* h, int32_t M, const int32_t* nodes, int32_t B, const double* d_dist, const int32_t* d_parent, int32_t n, const int32_t* d_set,
                   const int32_t* d_target, int32_t reverse, int32_t way_cap, int32_t* d_way, int32_t* d_way_len, double* d_stats, int32_t* d_status) {
  if (!h) return -2;
  const std::string me("pf_sight_paths");
  auto run = [&]() -> int {
    if (n < 0 || B < 1 || way_cap < 1)
      return failmsg(h, me + ": bad arguments (n = " + std::to_string(n) + ", B = " + std::to_string(B) + ", way_cap = " + std::to_string(way_cap) +
                            ": n >= 0, B >= 1 and way_cap >= 1 are needed)");
    if (!d_dist || !d_parent || !d_target || !d_way || !d_way_len || !d_status)
      return failmsg(h, me + ": bad arguments (the labels, the parents, the targets, the waypoint rows, their lengths and the statuses must not be null)");
    if (sight_nodes_check(h, me, M, nodes)) return -2;
    if (n == 0) return 0;
    unsigned long long* ctl = nullptr;
    int *d_nodes = nullptr, *d_rc = nullptr, *d_extra = nullptr;
    if (const int rc = sight_nodes(h, me, M, nodes, 0, ctl, d_nodes, d_rc, d_extra)) return rc;
    return timed(h, [&] {
      hipLaunchKernelGGL(k_sight_paths, dim3((unsigned)((n + PF_SIGHT_THREADS - 1) / PF_SIGHT_THREADS)), dim3(PF_SIGHT_THREADS), 0, h->stream, (int)M, (const int*)d_nodes,
                         h->C, (int)B, (const double*)d_dist, (const int*)d_parent, (int)n, (const int*)d_set, (const int*)d_target, reverse ? 1 : 0, (int)way_cap,
                         (int*)d_way, (int*)d_way_len, (double*)d_stats, (int*)d_status);
    });
  };
  return run() ? -1 : 0;
}

}  // extern "C"
