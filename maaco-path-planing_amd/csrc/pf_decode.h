// pf_decode.h -- K3: the chained waypoint decode (+ K1) and its planner, included twice by pathfit.hip.
//
// PF_DECODE_MULTI 0: k_plan_decode / DecodeArgs / k_decode_batch<PLAT> -- ONE start and ONE target cell for the whole launch, in
// the launch arguments.  This expansion is token for token the source these kernels had in pathfit.hip, at the place they had
// it, so their code is the code they had.
// PF_DECODE_MULTI 1: k_plan_decode_multi / DecodeMultiArgs / k_decode_multi<PLAT> -- every agent has its own start and target
// (int32[n] in HBM, the convention of pf_astar_batch), so decodes of different start / target pairs share one launch, one
// longest-first queue and one tail (GABatch: K populations in one generation).  Everything else is the same text.  This
// expansion is included at the end of pathfit.hip and its kernels are templates on a dummy parameter (PF_LATE, always 0): the
// compiler emits them behind every kernel the code object had before (pf_mpa_batch.h says why that matters).
//
// What differs is in the macros below: the kernels' names, the argument block, how an agent's endpoints are obtained
// (PF_DEC_ENDS), and the names the bodies then use for them (PF_DEC_START / PF_DEC_TARGET).  PF_DECODE_PART says which half is
// wanted: 1 the planner, 2 the kernel (the solo halves stay where they always were in pathfit.hip), 3 both.
#undef PF_DEC_PLAN
#undef PF_DEC_PLAN_EXTRA
#undef PF_DEC_PLAN_ENDS
#undef PF_DEC_PLAN_START
#undef PF_DEC_PLAN_TARGET
#undef PF_DEC_ENDS_T
#undef PF_DEC_ARGS
#undef PF_DEC_ENDS_DECL
#undef PF_DEC_TEMPLATE
#undef PF_DEC_KERNEL
#undef PF_DEC_ENDS
#undef PF_DEC_START
#undef PF_DEC_TARGET
#if PF_DECODE_MULTI
#define PF_DEC_PLAN template <int PF_LATE = 0> __global__ void k_plan_decode_multi
#define PF_DEC_ENDS_T const int*
#define PF_DEC_PLAN_EXTRA , int* bad
// the planner is also the argument check: an endpoint outside the grid raises *bad (the host reads it BEFORE the decode is
// launched) and is never used as an index; est may be null (n <= 64: no queue, the check alone)
#define PF_DEC_PLAN_ENDS(a)                                                                                             \
  const int a_start = start[a], a_target = target[a];                                                                  \
  if ((unsigned)a_start >= (unsigned)(G.R * G.C) || (unsigned)a_target >= (unsigned)(G.R * G.C)) { *bad = 1; return; } \
  if (!est) return;
#define PF_DEC_PLAN_START a_start
#define PF_DEC_PLAN_TARGET a_target
#define PF_DEC_ARGS DecodeMultiArgs
#define PF_DEC_ENDS_DECL const int* start; const int* target
#define PF_DEC_TEMPLATE template <bool PLAT, int PF_LATE = 0>
#define PF_DEC_KERNEL k_decode_multi
// one agent per wavefront: its two cells are wave-uniform, but the compiler cannot prove that of a load at an index that came
// out of next_agent -- readfirstlane puts them into scalar registers, where k_decode_batch's launch arguments live
#define PF_DEC_ENDS(a) const int a_start = __builtin_amdgcn_readfirstlane(p.start[a]), a_target = __builtin_amdgcn_readfirstlane(p.target[a]);
#define PF_DEC_START a_start
#define PF_DEC_TARGET a_target
#else
#define PF_DEC_PLAN __global__ void k_plan_decode
#define PF_DEC_ENDS_T int
#define PF_DEC_PLAN_EXTRA
#define PF_DEC_PLAN_ENDS(a)
#define PF_DEC_PLAN_START start
#define PF_DEC_PLAN_TARGET target
#define PF_DEC_ARGS DecodeArgs
#define PF_DEC_ENDS_DECL int start, target
#define PF_DEC_TEMPLATE template <bool PLAT>
#define PF_DEC_KERNEL k_decode_batch
#define PF_DEC_ENDS(a)
#define PF_DEC_START p.start
#define PF_DEC_TARGET p.target
#endif

#if PF_DECODE_PART & 1
PF_DEC_PLAN(Grid G, int n, int W, const int* wp_cells, const double* wp_pos, PF_DEC_ENDS_T start, PF_DEC_ENDS_T target, float* est PF_DEC_PLAN_EXTRA) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  PF_DEC_PLAN_ENDS(a)
  int cur = PF_DEC_PLAN_START; float e = 0.f;
  for (int k = 0; k <= W; ++k) {
    int goal = PF_DEC_PLAN_TARGET;
    if (k < W) {
      if (wp_cells) goal = wp_cells[(size_t)a * W + k];
      else {
        long r = (long)__builtin_rint(wp_pos[((size_t)a * W + k) * 2]), c = (long)__builtin_rint(wp_pos[((size_t)a * W + k) * 2 + 1]);
        r = r < 0 ? 0 : (r > G.R - 1 ? G.R - 1 : r); c = c < 0 ? 0 : (c > G.C - 1 ? G.C - 1 : c);
        goal = (int)(r * G.C + c);
      }
    }
    e += cell_dist(G, cur, goal); cur = goal;
  }
  est[a] = e;
}
#endif

#if PF_DECODE_PART & 2
struct PF_DEC_ARGS {
  Common c; ScoreP sp; int do_score;
  int n, W, path_cap; PF_DEC_ENDS_DECL;
  const int* wp_cells; const double* wp_pos;
  int* cells; int* len; int* status; double* stats;
};
PF_DEC_TEMPLATE
__global__ __launch_bounds__(64) void PF_DEC_KERNEL(PF_DEC_ARGS p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id();
  const Grid& G = p.c.G;
  const int RC = G.R * G.C;
  Open O = make_open(smem, p.c.S, p.c.tier2);
  Slot s = slot_load(p.c, RC);
  AStat tot = {0, 0, 0, 0, 0, 0};
  unsigned long long cells = 0, ovf = 0;
  for (;;) {
    int qpos = 0;
    const int a = next_agent(p.c, p.n, lane, &qpos);
    if (a < 0) break;
    if (p.c.retry && p.status[a] != 3) continue;
    PF_DEC_ENDS(a)
    s.sm.astar_too = p.c.st_astar || (p.c.queue && qpos < p.c.st_top);
    slot_begin_eval(s, RC, lane);
    int* out = p.cells + (size_t)a * p.path_cap;
    int n = 1, cur = PF_DEC_START, rc = 0;
    // Exact short cut.  A waypoint on an obstacle makes its segment's connector return [] at once (astar.py:37-39), and an empty
    // segment makes the whole decode return [] (ga_solver.py:74 / pso.py:77) -- whatever the segments before it found, and they
    // have no effect outside the call.  So the answer is known before the first search: PSO positions round onto obstacles
    // 27 % of the time per waypoint (~80 % of a swarm on G512), and the reference spends their earlier segments for nothing.
    for (int k = 0; k < p.W && rc == 0; ++k) {
      int goal;
      if (p.wp_cells) goal = p.wp_cells[(size_t)a * p.W + k];
      else {
        const double x = p.wp_pos[((size_t)a * p.W + k) * 2], y = p.wp_pos[((size_t)a * p.W + k) * 2 + 1];
        long r = (long)__builtin_rint(x), c = (long)__builtin_rint(y);
        r = r < 0 ? 0 : (r > G.R - 1 ? G.R - 1 : r);
        c = c < 0 ? 0 : (c > G.C - 1 ? G.C - 1 : c);
        goal = (int)(r * G.C + c);
      }
      if ((unsigned)goal >= (unsigned)RC || G.occ[goal] == 1) rc = 1;
    }
    if (lane == 0) { out[0] = PF_DEC_START; s.rec[PF_DEC_START].meta = s.avoid_ep << PF_AVOID_SHIFT; }   // ga_solver.py:63-65
    for (int k = 0; k <= p.W && rc == 0; ++k) {
      int goal = PF_DEC_TARGET;
      if (k < p.W) {
        if (p.wp_cells) goal = p.wp_cells[(size_t)a * p.W + k];
        else {                                                   // pso.py:61,69-70: round-half-even then clamp
          double x = p.wp_pos[((size_t)a * p.W + k) * 2], y = p.wp_pos[((size_t)a * p.W + k) * 2 + 1];
          long r = (long)__builtin_rint(x), c = (long)__builtin_rint(y);
          r = r < 0 ? 0 : (r > G.R - 1 ? G.R - 1 : r);
          c = c < 0 ? 0 : (c > G.C - 1 ? G.C - 1 : c);
          goal = (int)(r * G.C + c);
        }
      }
      int m = 0;
      if (p.c.st_tail > 0 && !s.sm.astar_too) {                  // the batch's tail: few agents left, the chip mostly idle -> shorten the chain
        const unsigned long long dn = __hip_atomic_load(&p.c.cnt->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((long long)p.n - (long long)first_u64(dn) <= (long long)p.c.st_tail) s.sm.astar_too = true;
      }
      rc = astar<0, PLAT>(G, s, O, cur, goal, out + n - 1, p.path_cap - (n - 1), m, tot, lane, out, n);   // ga_solver.py:68-72 (avoid = the cells visited so far)
      if (rc != 0) break;                                        // :74 / :85 -> []
      mark_avoid(s, out + n, m - 1, lane);                       // :76 nodes_in_path_so_far.update
      n += m - 1;
      cur = goal;
    }
    // ga_solver.py:90-93 (drop consecutive duplicates) is a no-op here: a segment's tail never starts with its head
    if (rc != 0) n = 0;
    double sc[5];
    if (p.do_score) score_path(G, p.sp, out, n, lane, sc);
    if (lane == 0) { p.len[a] = n; p.status[a] = rc; atomicAdd(&p.c.cnt->done, 1ull); }
    if (p.do_score && lane < 5) p.stats[(size_t)a * 5 + lane] = sc[lane];
    cells += n; ovf += rc == 3;
  }
  slot_store(p.c, s, lane);
  flush_counters(p.c.cnt, tot, cells, ovf, lane);
}
#endif
#undef PF_DECODE_PART
#undef PF_DECODE_MULTI
