// pf_maaco_walk.h -- the MAACO walk kernels (K4), compiled twice by pathfit.hip: PF_MAACO_BATCH 0 gives the solo kernels
// k_maaco_walk / k_maaco_walk8, 1 the batched ones k_maaco_walk_batch / k_maaco_walk8_batch (K colonies of mc.nper ants, global
// ant a = local ant a % nper of colony a / nper).  The solo expansion is token for token the kernels as they were before the
// batched form existed, so their code objects are unchanged.  PF_B(b, s): the batched / the solo form of an expression.
__global__ __launch_bounds__(64) void PF_WALK1(MaacoArgs p PF_COLONIES) {
  const int lane = lane_id();
  const Grid& G = p.G;
  const int R = G.R, C = G.C, RC = R * C;
  unsigned* visit = p.visit + (size_t)blockIdx.x * p.vstride;
  unsigned epoch = p.slot_epoch[blockIdx.x];
  const int WPR = p.wpr;
  TabuLast tl;
  const int k = lane & 7;
  const int mdr = AM_DR[k], mdc = AM_DC[k];
  const unsigned hbit = 1u << AM_TO_HM[k];
#if PF_MAACO_BATCH
  int sr = 0, sc = 0, tr = 0, tc = 0; unsigned O1 = 0;               // (per ant: its colony's)
#else
  const int sr = row_of(G, p.start), sc = p.start - sr * C;
  const int tr = row_of(G, p.target), tc = p.target - tr * C;
  // MAACO.py:147-150 start->target orientation: static per move
  const int vrS = tr - sr, vcS = tc - sc;
  const bool o1 = !((vcS > 0 && mdc < 0) || (vcS < 0 && mdc > 0) || (vrS > 0 && mdr < 0) || (vrS < 0 && mdr > 0));
  const unsigned O1 = (unsigned)(__ballot(o1 && lane < 8) & 0xFF);
#endif
  const double mcost = (mdr != 0 && mdc != 0) ? PF_SQRT2 : 1.0;
  const uint64_t q0_bits = p.q0 >= 1.0 ? ~0ull : (p.q0 < 0.0 ? 0ull : (uint64_t)(p.q0 * 9007199254740992.0));   // q <= q0 as an integer test (k_maaco_walk8)
  unsigned long long steps_tot = 0, cand_tot = 0, cells_tot = 0, ovf_tot = 0;
  for (;;) {
    const int a = next_work(p.work, lane);
    if (a >= p.n) break;
    epoch += 1;
    if (epoch >= PF_TABU_WRAP) {
      for (int i = lane; i < p.vstride; i += 64) visit[i] = 0;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      epoch = 1;
    }
#if PF_MAACO_BATCH
    // the ant's colony: start, target, orientation, stream, tables and deposit matrix (the ant's bit and deposit at its local index)
    const int col = a / mc.nper, la = a - col * mc.nper;
    const int start = mc.start[col]; sr = row_of(G, start); sc = start - sr * C;
    { const int target = mc.target[col]; tr = row_of(G, target); tc = target - tr * C; }
    O1 = colony_o1(sr, sc, tr, tc);
    const double* tau = p.tau + (size_t)col * RC; const double* eta = p.eta + (size_t)mc.eta_of[col] * 2 * RC;
    Rng g; g.init(mc.seed[col], DOM_MAACO, (unsigned long long)p.iter, (unsigned long long)la);
#else
    Rng g; g.init(p.seed, DOM_MAACO, (unsigned long long)p.iter, (unsigned long long)(p.ant0 + a));
#endif
    int* out = p.cells + (size_t)a * p.path_cap;
    int cr = sr, cc = sc, n = 1, prev_k = -1, nturn = 0, rc = 0;
    double plen = 0.0;
    tl.reset();
    {
      const int wi = sr * WPR + (sc >> 4); const unsigned wv = tabu_set(0u, epoch, sc);
      if (lane == 0) { out[0] = PF_B(start, p.start); visit[wi] = wv; }
      tl.stored(wi, wv);
    }
    const int max_steps = RC * 2;                                  // MAACO.py:283 (<= 2^25)
    int steps = 0;
    while (!(cr == tr && cc == tc) && steps < max_steps) {
      const int cur = cr * C + cc;
      const int nr = cr + mdr, nc = cc + mdc;
      const bool inb = lane < 8 && nr >= 0 && nr < R && nc >= 0 && nc < C;
      const int nidx = nr * C + nc;
      const int turn = (prev_k >= 0 && k != prev_k) ? 1 : 0;     // MAACO.py:184-195
      unsigned vw = 0, mmask = 0; double tv = 0.0, ev = 0.0;
      const int widx = nr * WPR + (nc >> 4);
      if (inb) { vw = tl.patch(widx, visit[widx]); tv = PF_B(tau, p.tau)[nidx]; ev = PF_B(eta, p.eta)[(size_t)nidx * 2 + turn]; }
      else if (lane == 9) mmask = G.mm[cur];
      const unsigned M = (unsigned)bcast_i((int)mmask, 9);
      // valid, not tabu, no corner cut (:93-95,:100-120); the low byte of the mask = lanes 0..7
      const unsigned mall = (unsigned)(B((unsigned)nr < (unsigned)R) & B((unsigned)nc < (unsigned)C) & B((M & hbit) != 0u) &
                                       ~(B((vw >> 16) == epoch) & B(((vw >> (nc & 15)) & 1u) != 0u))) & 0xFFu;
      // strategy 2 orientation: current -> target (:152-157)
      // (RowMask[sign vr] & ColMask[sign vc] from two constants: see k_maaco_walk8)
      const unsigned ur = (unsigned)min(max(tr + 1 - cr, 0), 2), uc = (unsigned)min(max(tc + 1 - cc, 0), 2);
      const unsigned O2 = __builtin_amdgcn_ubfe(0xF8FF1Fu, ur << 3, 8u) & __builtin_amdgcn_ubfe(0xD6FF6Bu, uc << 3, 8u);
      unsigned cand = mall & O1;                                  // :165
      if (!cand) cand = mall & O2;                                // :168-169
      if (!cand) cand = mall;                                     // :172-180
      if (!cand) { rc = 1; break; }                               // :287-288
      const int ncand = __builtin_popcount(cand);
      cand_tot += ncand;
      const bool cmine = lane < 8 && ((cand >> k) & 1u);
      // ONE mix serves the step (see k_maaco_walk8): lane j mixes word j + 1 of the ant's stream -- q, the first word of the choice
      // and six more for random.choice's rejection loop, which used to cost a full mix64 per extra draw.
      const uint64_t Wk = g.peek64(1 + (uint64_t)k);
      const bool greedy = (__builtin_amdgcn_ballot_w64((Wk >> 11) <= q0_bits) & 1ull) != 0;   // :232 q = word 1 (lane 0); q <= q0 as integers
      const double attr = cmine ? tv * ev : 0.0;                  // :238 tau^alpha * eta'^beta; the other lanes add exact zeros
      const double Mx = gmax8(cmine ? attr : -1.0);               // (lanes 0..7 are one 8-lane group)
      int pick = 0;
      unsigned msel = cand;                                       // the set random.choice draws from
      bool chosen = false;
      if (greedy) {                                               // :241-250 running max with absolute tolerance, closed form (k_maaco_walk8)
        const unsigned eq = (unsigned)(B(attr == Mx)) & cand;      // (cand = the lanes 0..7 that hold a candidate)
        if (!eq) { rc = 1; break; }
        msel = (unsigned)(B(k >= __builtin_ctz(eq)) & B(fabs(attr - Mx) < 1e-9)) & cand;
      } else if (!(bcast_d(Mx, 0) * 8.0 < 5e-10)) {               // (else the ordered sum is below 1e-9 whatever its rounding: k_maaco_walk8)
        const double sum = bcast_d(gscan8(attr, k), 7);           // :252 sum() in candidate order (ordered 8-lane scan)
        if (!(sum < 1e-9)) {                                      // else :253-254: random.choice over all candidates
          const double p0 = attr / sum;                           // :255
          double pj = p0;
          if (!(sum < 1.0e300)) {                                 // :256-258 cannot renormalise for a finite sum (see k_maaco_walk8)
            const double ps = bcast_d(gscan8(p0, k), 7);
            if (fabs(ps - 1.0) > 1e-6) pj = p0 / ps;
          }
          const double u = Rng::to_unit(((uint64_t)(unsigned)bcast_i((int)(Wk >> 32), 1) << 32) | (unsigned)bcast_i((int)Wk, 1));   // :259 np.random.choice -> one random_sample: word 2
          const double mine = gscan8(pj, k);                      // cdf = cumsum(p); cdf /= cdf[-1]
          const double last = bcast_d(mine, 7);
          const unsigned tm = (unsigned)__ballot(cmine && mine / last <= u) & 0xFFu;   // searchsorted(cdf, u, side='right')
          int idx = tm ? __builtin_popcount(cand & ((2u << (31 - __builtin_clz(tm))) - 1u)) : 0;
          if (idx > ncand - 1) idx = ncand - 1;
          pick = nth_set_bit(cand, idx);
          chosen = true;
          g.advance(2);
        }
      }
      if (!chosen) {
        // random.choice(set) = set[_randbelow(n)]: the first of words 2..8 whose top bit_length(n) bits are below n (a ballot)
        const unsigned nsel = (unsigned)__builtin_popcount(msel);
        const int kb = 32 - __builtin_clz(nsel);
        const unsigned rk = (unsigned)(Wk >> (64 - kb));
        const unsigned acc = (unsigned)B(rk < nsel) & 0xFEu;
        unsigned r;
        if (acc) { const int first = __builtin_ctz(acc); r = (unsigned)bcast_i((int)rk, first); g.advance(1u + (unsigned)first); }
        else { g.advance(8); do { r = (unsigned)(g.next64() >> (64 - kb)); } while (r >= nsel); }
        pick = nth_set_bit(msel, (int)r);
      }
      plen += bcast_d(mcost, pick);                               // :293
      if (prev_k >= 0 && pick != prev_k) nturn += 1;              // :264-276 counted on the fly
      prev_k = pick;
      cr += bcast_i(mdr, pick); cc += bcast_i(mdc, pick);
      if (n >= p.path_cap) { rc = 3; break; }
      {
        const int wi = cr * WPR + (cc >> 4);                        // = lane `pick`'s word, which it holds up to date
        const unsigned wv = tabu_set((unsigned)bcast_i((int)vw, pick), epoch, cc);
        if (lane == 0) { out[n] = cr * C + cc; visit[wi] = wv; }
        tl.stored(wi, wv);
      }
      n += 1; steps += 1;
    }
    if (rc == 0 && !(cr == tr && cc == tc)) rc = 2;               // :301-302 step cap
    steps_tot += (unsigned long long)steps;
    if (lane == 0) {
      p.len[a] = rc == 0 ? n : 0;
      p.plen[a] = rc == 0 ? plen : PF_INF;
      p.turns[a] = rc == 0 ? nturn : -1;
      p.status[a] = rc;
    }
    if (p.bits) {
      const bool good = rc == 0 && n > 0 && plen > 1e-6;           // MAACO.py:307
#if PF_MAACO_BATCH
      double* dep = p.dep + (size_t)col * mc.dep_stride; unsigned long long* bits = p.bits + (size_t)col * mc.bits_stride;
      uint8_t* flag = p.flag + (size_t)col * mc.flag_stride;
#endif
      if (lane == 0) PF_B(dep[la], p.dep[a]) = good ? p.Q / plen : 0.0;   // :308
      if (good) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // lane 0 wrote the path
        const unsigned long long bit = 1ull << (PF_B(la, a) & 63);
        uint8_t* fl = PF_B(flag, p.flag) + (PF_B(la, a) >> 6);
        for (int i = lane; i < n; i += 64) { const int c = out[i]; atomicOr(&PF_B(bits, p.bits)[bits_idx(c, PF_B(la, a) >> 6, p.fstride)], bit); fl[(size_t)(c >> 6) * p.fstride] = 1; }
      }
    }
    cells_tot += rc == 0 ? n : 0; ovf_tot += rc == 3;
  }
  if (lane == 0) {
    p.slot_epoch[blockIdx.x] = epoch;
    atomicAdd(&p.cnt->steps, steps_tot); atomicAdd(&p.cnt->candidates, cand_tot); atomicAdd(&p.cnt->path_cells, cells_tot);
    if (ovf_tot) atomicAdd(&p.cnt->overflow, ovf_tot);
  }
}

// ---------------------------------------------------------------------------
// K4, packed form: EIGHT ants per wavefront.  A walk step only ever uses 8 lanes (the 8 moves), so each group
// of 8 lanes walks its own ant; "per-ant uniform" values are replicated in the group's lanes, broadcasts are
// ds_bpermute inside the group, candidate masks are 8-bit slices of the wave ballot.  A group that finishes
// its ant emits the result and immediately fetches the next ant from the queue inside the same loop, so no
// lanes idle until the queue is empty.  Same draws, same arithmetic, same order as k_maaco_walk.
// ---------------------------------------------------------------------------
#if !PF_MAACO_BATCH
PF_DEV unsigned gballot8(bool p) { return (unsigned)(__builtin_amdgcn_ballot_w64(p) >> (lane_id() & 56)) & 0xFFu; }
// (g8: my group's byte of a wave mask; compound predicates as B(a) & B(b): pf_device.h)
PF_DEV unsigned g8(pf_u64 m) { return (unsigned)(m >> (lane_id() & 56)) & 0xFFu; }
PF_DEV int gbcast8_i(int v, int k) { return __builtin_amdgcn_ds_bpermute(((lane_id() & 56) + k) << 2, v); }
// index of the idx-th set bit of an 8-bit mask (lane k tests bit k)
PF_DEV int gnth8(unsigned m, int idx, int k) {
  return __builtin_ctz(g8(B(((m >> k) & 1u) != 0u) & B(__builtin_popcount(m & ((1u << k) - 1u)) == idx)) | 0x100u);
}
PF_DEV double gbcast8_d(double v, int k) {
  const int lo = gbcast8_i(__double2loint(v), k), hi = gbcast8_i(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}
#endif

// eight ants per wavefront: the 8 lanes of a group hold the 8 moves of one ant
// AHEAD, the form for batches that leave a SIMD ONE wavefront (8 192 ants: a step then waits ~2 000 clocks for memory, and nothing
// else runs meanwhile): all of a step's loads are issued before anything waits for one of them (the compiler otherwise sinks the
// pheromone load behind the candidate test: a second round trip), and every move lane also asks for the pheromone record and
// the tabu word two steps ahead in its direction -- where the NEXT step's neighbours live -- right behind the step's own loads
// (memory returns in order: they cannot delay them; results unused).  A/B on one box (M evals/s): 8 192 ants @1024^2 2.87 -> 3.04;
// 16 384 ants @512^2 (two wavefronts per SIMD, issue-bound) 8.75 -> 8.50 -- so the host picks the form by occupancy.
template <bool AHEAD>
__global__ __launch_bounds__(64) void PF_WALK8(MaacoArgs p PF_COLONIES) {
  const Grid& G = p.G;
  const int R = G.R, C = G.C, RC = R * C;
  const int lane = lane_id();
  const int k = lane & 7, grp = lane >> 3;
  const int slot = blockIdx.x * 8 + grp;
  unsigned* visit = p.visit + (size_t)slot * p.vstride;
  unsigned epoch = p.slot_epoch[slot];
  const int WPR = p.wpr;
  TabuLast tl; tl.reset();
  const int mdr = AM_DR[k], mdc = AM_DC[k];
  const unsigned hbit = 1u << AM_TO_HM[k];
#if PF_MAACO_BATCH
  // the groups of a wavefront may walk ants of different colonies: the colony's values are per group, set by fetch()
  int sr = 0, sc = 0, tr = 0, tc = 0, start = 0, la = 0, col = 0; unsigned O1 = 0;
  const double* tep = p.tep;
#else
  const int sr = row_of(G, p.start), sc = p.start - sr * C;
  const int tr = row_of(G, p.target), tc = p.target - tr * C;
  const int vrS = tr - sr, vcS = tc - sc;
  const bool o1 = !((vcS > 0 && mdc < 0) || (vcS < 0 && mdc > 0) || (vrS > 0 && mdr < 0) || (vrS < 0 && mdr > 0));
  const unsigned O1 = gballot8(o1);
#endif
  const int max_steps = RC * 2;                                    // MAACO.py:283
  // q0 is in [0.01, 0.99] (MAACO.py:226): q0 2^53 is exact, its floor the largest 53-bit draw that still takes the greedy rule
  // (as `draw < q0_lim`: a `<=` against a run-time bound compiles to two compares, one for the bound's all-ones case)
  const uint64_t q0_lim = p.q0 >= 1.0 ? (1ull << 53) : (p.q0 < 0.0 ? 0ull : (uint64_t)(p.q0 * 9007199254740992.0) + 1ull);
  unsigned long long steps_tot = 0, cand_tot = 0, cells_tot = 0, ovf_tot = 0;
  // per-ant state (replicated in the 8 lanes of the group)
  int a = -1, cr = 0, cc = 0, n = 0, prev_k = -1, nturn = 0, rc = 0;
  int steps = 0;                                                   // (<= 2 R C <= 2^25)
  double plen = 0.0;
  Rng g; g.key = 0; g.ctr = 0; g.kc = 0;
  int* out = p.cells;
  bool alive = grp < p.groups;
#ifdef PF_WALK_PROBE
  unsigned long long pr_wait = 0, pr_rounds = 0, pr_mark = 0, pr_sel0 = 0, pr_sel1 = 0, pr_head = 0, pr_emit = 0, pr_upd = 0, pr_loop = 0, pr_end = 0, pr_act = 0; const unsigned long long pr_t0 = __builtin_amdgcn_s_memtime();
#endif
  // fetch + initialise the next ant of this group (alive = false when the queue is empty)
  auto fetch = [&]() {
    int w = 0;
    if (k == 0) w = atomicAdd(p.work, 1);
    w = gbcast8_i(w, 0);
    if (w >= p.n) alive = false;
    else {
      a = w;
      epoch += 1;
      if (epoch >= PF_TABU_WRAP) {
        for (int i = k; i < p.vstride; i += 8) visit[i] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        epoch = 1;
      }
#if PF_MAACO_BATCH
      col = a / mc.nper; la = a - col * mc.nper;
      start = mc.start[col]; sr = row_of(G, start); sc = start - sr * C;
      { const int target = mc.target[col]; tr = row_of(G, target); tc = target - tr * C; }
      O1 = colony_o1(sr, sc, tr, tc);
      tep = p.tep + (size_t)col * 3 * RC;
      g.init(mc.seed[col], DOM_MAACO, (unsigned long long)p.iter, (unsigned long long)la);
#else
      g.init(p.seed, DOM_MAACO, (unsigned long long)p.iter, (unsigned long long)(p.ant0 + a));
#endif
      out = p.cells + (size_t)a * p.path_cap;
      cr = sr; cc = sc; n = 1; prev_k = -1; nturn = 0; rc = 0; plen = 0.0; steps = 0;
      tl.reset();
      const int wi = sr * WPR + (sc >> 4); const unsigned wv = tabu_set(0u, epoch, sc);
      if (k == 0) { out[0] = PF_B(start, p.start); visit[wi] = wv; }
      tl.stored(wi, wv);
    }
  };
  if (alive) fetch();
  // One wave-uniform test per round: "did an ant finish?" (one round in a hundred).  Emitting, deposit marking, fetching the group's
  // next ant and the end-of-queue test all sit behind it; a round that only steps pays for nothing else.  (A wave none of whose
  // groups got an ant -- the queue was drained by the others' first fetches -- never enters the loop: every exit is behind any_fin.)
  unsigned pft0 = 0, pft1 = 0;
  if (__ballot(alive)) for (;;) {
    bool done = alive & (((cr == tr) & (cc == tc)) | (steps >= max_steps));
    const unsigned pft0_prev = pft0, pft1_prev = pft1;
#ifdef PF_WALK_PROBE
    __builtin_amdgcn_sched_barrier(0); const unsigned long long pr_r0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0);
    bool pr_stepped = false; unsigned long long pr_u0 = 0;
    if (pr_end) pr_loop += pr_r0 - pr_end;
#endif
    if (alive && !done) {
      // (rows, columns and cells fit 24 bits -- R, C <= 4096 --: v_mad_u32_u24 at full rate and 32-bit byte offsets on a scalar
      // base, where `int` indices cost a quarter-rate 64-bit multiply-add, a sign extension and a 64-bit add per load)
      const unsigned cur = __umul24((unsigned)cr, (unsigned)C) + (unsigned)cc;
      const int nr = cr + mdr, nc = cc + mdc;
      const bool inb = ((unsigned)nr < (unsigned)R) & ((unsigned)nc < (unsigned)C);
      const unsigned nidx = __umul24((unsigned)nr, (unsigned)C) + (unsigned)nc;
      const int turn = ((prev_k >= 0) & (k != prev_k)) ? 1 : 0;    // MAACO.py:184-195
      unsigned vw = 0; double tv = 0.0, ev = 0.0;
      const unsigned M = *((const uint8_t*)G.mm + (size_t)cur);
      const unsigned widx = __umul24((unsigned)nr, (unsigned)WPR) + ((unsigned)nc >> 4);
      // Every step that finds a candidate draws q (:232) and then at least one more 64-bit word (random.choice's first
      // getrandbits at :250 / :254, or numpy's random_sample at :259): both words are mixed here, before the loads below
      // are waited for, and the counter advances only when the step gets that far.
      // ONE mix serves the whole step: lane j of the ant's group mixes word j + 1 of the stream (the same instructions in every
      // lane), i.e. the eight next words at once -- q, the first word of the choice, and six more for random.choice's rejection
      // loop (_randbelow redraws while the k-bit value is >= n: every second draw for n = 1, every fourth for n = 3), which used to
      // cost the wave a full mix64 (~25 instructions, eight quarter-rate multiplies) per extra draw of its unluckiest ant.
      uint64_t Wk = 0;
      if (!AHEAD) Wk = g.peek64(1 + (uint64_t)k);
#ifdef PF_WALK_PROBE
      __builtin_amdgcn_sched_barrier(0); const unsigned long long pr_ta = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0);
      pr_head += pr_ta - pr_r0; pr_stepped = true; pr_act += 1;   // (per-lane copies: lane 0 reports, so the in-step stamps cover the rounds in which group 0 stepped)
#endif
      {
        // unconditional loads (a move that leaves the map reads cell 0 and is rejected by `inb` below): a branch around them costs
        // a scalar round trip on the mask, and loads under a branch keep the compiler from counting them
        const unsigned widx_c = inb ? widx : 0u, nidx_c = inb ? nidx : 0u;
        const unsigned vw_raw = visit[widx_c];
        // one divergent vector load less per step: tau and eta'[turn] in one
        const unsigned toff = __umul24(nidx_c, 24u) + ((unsigned)turn << 3);
        const pf_d2u te = *(const pf_d2u*)((const char*)PF_B(tep, p.tep) + (size_t)toff);
        if (AHEAD) {
          const int r2 = nr + mdr, c2 = nc + mdc;
          const bool in2 = ((unsigned)r2 < (unsigned)R) & ((unsigned)c2 < (unsigned)C);
          const unsigned t2 = in2 ? __umul24((unsigned)r2, (unsigned)C) + (unsigned)c2 : nidx_c;
          const unsigned w2 = in2 ? __umul24((unsigned)r2, (unsigned)WPR) + ((unsigned)c2 >> 4) : widx_c;
          pft0 = *(const unsigned*)((const char*)PF_B(tep, p.tep) + (size_t)__umul24(t2, 24u));
          pft1 = visit[w2];
          __builtin_amdgcn_sched_barrier(0);                        // (all of the step's loads are issued before anything waits for one of them)
        }
        vw = tl.patch((int)widx_c, vw_raw);
        tv = turn ? te.x : te.y; ev = turn ? te.y : te.x;
        if (AHEAD) asm volatile("" :: "v"(pft0_prev), "v"(pft1_prev));   // (the previous step's touches: older than the loads just waited for)
      }
      if (AHEAD) Wk = g.peek64(1 + (uint64_t)k);                    // (in the shadow of the loads just issued)
#ifdef PF_WALK_PROBE
      { __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
        pr_wait += __builtin_amdgcn_s_memtime() - pr_ta; }
#endif
      // (bitwise on purpose: the short-circuit forms compiled to branches, each a scalar round trip on a freshly written lane mask)
      const unsigned mall = g8(B((unsigned)nr < (unsigned)R) & B((unsigned)nc < (unsigned)C) & B((M & hbit) != 0u) &
                               ~(B((vw >> 16) == epoch) & B(((vw >> (nc & 15)) & 1u) != 0u)));
      // strategy 2 orientation, current -> target (:152-157): a move is kept iff its row step does not oppose sign(vr) and its column
      // step does not oppose sign(vc) -- the eight-move mask is RowMask[sign vr] & ColMask[sign vc], two bit-field extracts from
      // constants (moves 0..7 = AM_DR / AM_DC order) instead of eight compares, their scalar mask logic and a ballot
      const unsigned ur = (unsigned)min(max(tr + 1 - cr, 0), 2), uc = (unsigned)min(max(tc + 1 - cc, 0), 2);
      const unsigned O2 = __builtin_amdgcn_ubfe(0xF8FF1Fu, ur << 3, 8u) & __builtin_amdgcn_ubfe(0xD6FF6Bu, uc << 3, 8u);
      unsigned cand = mall & O1;                                    // :165
      if (!cand) cand = mall & O2;                                  // :168-169
      if (!cand) cand = mall;                                       // :172-180
      // (AHEAD: the dead end "uses" the pheromone record too, so that its load stays in front of the candidate test)
      if (!cand) { rc = 1; done = true; if (AHEAD) asm volatile("" :: "v"(tv), "v"(ev)); }   // :287-288
      else {
        const int ncand = __builtin_popcount(cand);
        cand_tot += ncand;
        const bool cmine = (cand >> k) & 1u;
        // :232 q = word 1 of the step (lane 0 of the group holds it): one ballot tells the group which rule applies
        // (q = (w >> 11) 2^-53 exactly, so q <= q0 iff w >> 11 <= floor(q0 2^53): two integer instructions instead of the conversion)
        const bool greedy = (g8(B((Wk >> 11) < q0_lim)) & 1u) != 0;
        const double attr = cmine ? tv * ev : 0.0;                  // :238; the other lanes add an exact zero to the ordered sums below
        int pick = 0;
#ifdef PF_WALK_PROBE
        __builtin_amdgcn_sched_barrier(0); const unsigned long long pr_s0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0);
        pr_sel0 += pr_s0 - pr_ta;
#endif
        // Both rules end in random.choice over a set of candidates: the greedy rule (:241-250) over its tie set, the other one
        // (:252-254) over all candidates whenever the attractiveness sum is below 1e-9 -- on the 512^2 and 1024^2 maps with beta = 7
        // that is EVERY non-greedy step (eta'^7 ~ 1e-19: SURVEY H8 measured 0 % roulette picks).  So the two rules only differ in
        // the set, and ONE choice serves every ant of the wave; the roulette proper runs behind a wave-uniform test.
        // The largest attractiveness among the candidates is the greedy rule's maximum AND a bound on the other rule's sum: the
        // ordered sum of at most 8 non-negative terms, none above Mx, is at most 8 Mx (1 + 2^-53)^7 -- with 8 Mx < 5e-10 it is
        // below 1e-9 whatever its rounding, and the 7-step ordered scan need not run.
        const double Mx = gmax8(cmine ? attr : -1.0);
        // :241-250, the running maximum with its absolute tolerance, in closed form: the tie set restarts at the FIRST occurrence of
        // the maximum (`attr > max` drops every earlier member there) and from then on collects the candidates within 1e-9 of it
        // (none can exceed it).  NaN neither restarts nor joins, as in the loop.
        const pf_u64 cmm = B(((cand >> k) & 1u) != 0u);
        const unsigned eq = g8(cmm & B(attr == Mx));
        const unsigned bm = g8(cmm & B(k >= __builtin_ctz(eq | 0x100u)) & B(fabs(attr - Mx) < 1e-9));
        const bool tiny = Mx * 8.0 < 5e-10;                         // (a NaN maximum compares false: the sum decides)
        if (greedy && !eq) { rc = 1; done = true; }
        bool chosen = false;                                        // the roulette proper picked (two words of the stream: q and u)
        if (B(true) & ~B(greedy) & ~B(tiny)) {
          // The sums of :252-259 run over the candidates in candidate order.  Candidate j lives in lane j, so each is one
          // ordered 8-lane scan (7 dependent DPP steps, no LDS round trip per candidate); every quotient belongs to one
          // candidate and is computed in its lane.  (The scans run for the whole wave; only the ants that need them use the result.)
          const double sum = glast8(gscan8(attr, k));               // :252
          if (!greedy && !tiny && !(sum < 1e-9)) {                  // else :253-254: random.choice over all candidates, below
            const double p0 = attr / sum;                           // :255 probabilities[j]
            // :256-258 renormalise when |sum(probabilities) - 1| > 1e-6.  For a finite sum of at most 8 non-negative terms
            // that never happens: sum = S(1 + e), |e| <= 7u (u = 2^-53), every quotient is a_j / sum (1 + d_j), |d_j| <= u
            // (an underflowing quotient errs by < 2^-1074), and adding them in order costs another 7u, so
            // |sum(probabilities) - 1| < 16u ~ 2e-15.  Only an overflowed sum takes the general route.
            double pj = p0;
            if (!(sum < 1.0e300)) {
              const double ps = glast8(gscan8(p0, k));              // :256 sum(probabilities)
              if (fabs(ps - 1.0) > 1e-6) pj = p0 / ps;              // :257-258
            }
            const double u = gbcast8_d(Rng::to_unit(Wk), 1);        // :259 numpy.random.choice: cdf = cumsum(p); cdf /= cdf[-1]; word 2 of the step
            const double mine = gscan8(pj, k);                      // cdf[position of my move]
            const double last = glast8(mine);
            const unsigned tm = gballot8(cmine && mine / last <= u);   // searchsorted(cdf, u, side="right")
            int idx = tm ? __builtin_popcount(cand & ((2u << (31 - __builtin_clz(tm))) - 1u)) : 0;
            if (idx > ncand - 1) idx = ncand - 1;
            pick = gnth8(cand, idx, k);
            chosen = true;
            g.advance(2);
          }
        }
        {
          // random.choice(set) = set[_randbelow(n)]: kb = n.bit_length() bits of a word, redrawn while >= n (:250 / :254).  Word j + 1
          // of the step sits in lane j: every lane tests ITS word, the first acceptable one (a ballot) is the draw.
          const unsigned msel = greedy ? bm : cand;
          const unsigned nsel = (unsigned)__builtin_popcount(msel) | (msel ? 0u : 1u);   // (>= 1: a failed ant's value is never used)
          const int kb = 32 - __builtin_clz(nsel);
          unsigned rk = (unsigned)(Wk >> (64 - kb));
          const unsigned acc = g8(B(rk < nsel)) & 0xFEu;             // (word 1 is q: lanes k >= 1)
          unsigned r = (unsigned)gbcast8_i((int)rk, __builtin_ctz(acc | 0x80u));
          if (!chosen) g.advance(acc ? 1u + (unsigned)__builtin_ctz(acc) : 8u);
          if (B(acc == 0u)) {                                        // all seven rejected (n = 1: once in 128 steps): draw on, one word at a time
            if (!chosen && !done && acc == 0u) { do { r = (unsigned)(g.next64() >> (64 - kb)); } while (r >= nsel); }
          }
          if (!chosen) pick = gnth8(msel, (int)r, k);
        }
#ifdef PF_WALK_PROBE
        int t_ = pick; asm volatile("" : "+v"(t_)); __builtin_amdgcn_sched_barrier(0); const unsigned long long pr_s1 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0);
        pr_sel1 += pr_s1 - pr_s0; pr_u0 = pr_s1;
#endif
        if (!done) {
          plen += ((0xA5u >> pick) & 1u) ? PF_SQRT2 : 1.0;         // :293 (moves 0, 2, 5, 7 are the diagonals)
          if (prev_k >= 0 && pick != prev_k) nturn += 1;
          prev_k = pick;
          cr += (int)((0xA940u >> (2 * pick)) & 3u) - 1;            // AM_DR[pick] + 1, two bits a move
          cc += (int)((0x9224u >> (2 * pick)) & 3u) - 1;            // AM_DC[pick] + 1
          {
            // a full path row (rc 3) is the exception: predicated, not a branch of its own
            const bool ovf = n >= p.path_cap;
            rc = ovf ? 3 : rc; done = ovf;
            const int wi = cr * WPR + (cc >> 4);                   // = lane `pick`'s word, which it holds up to date
            const unsigned wv = tabu_set((unsigned)gbcast8_i((int)vw, pick), epoch, cc);
            if (k == 0 && !ovf) { out[n] = cr * C + cc; visit[wi] = wv; }
            if (!ovf) tl.stored(wi, wv);
            n += ovf ? 0 : 1; steps += ovf ? 0 : 1;
          }
        }
      }
    }
#ifdef PF_WALK_PROBE
    __builtin_amdgcn_sched_barrier(0); const unsigned long long pr_e0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0);
    if (pr_u0) pr_upd += pr_e0 - pr_u0;
#endif
    // an ant finishes in about one round of a hundred: everything that only a finished ant needs sits behind ONE wave-uniform test
    const bool any_fin = __ballot(alive && done) != 0ull;
    if (any_fin && alive && done) {                                 // emit, then fetch a new ant next round
      if (rc == 0 && !(cr == tr && cc == tc)) rc = 2;               // :301-302 step cap
      steps_tot += (unsigned long long)steps;
      if (k == 0) {
        p.len[a] = rc == 0 ? n : 0;
        p.plen[a] = rc == 0 ? plen : PF_INF;
        p.turns[a] = rc == 0 ? nturn : -1;
        p.status[a] = rc;
      }
      cells_tot += rc == 0 ? n : 0; ovf_tot += rc == 3;
    }
#ifdef PF_WALK_PROBE
    pr_rounds += 1; const unsigned long long pr_m0 = __builtin_amdgcn_s_memtime(); pr_emit += pr_m0 - pr_e0;
#endif
    if (any_fin && p.bits) {
      // the ants that finished in this round mark their deposits: the WHOLE wave walks each finished path (64 cells a round;
      // the other groups would only wait for a group that marked alone, 8 cells a round)
      const bool fin = alive && done;
      const bool good = fin && rc == 0 && n > 0 && plen > 1e-6;    // MAACO.py:307
      if (fin && k == 0) PF_B(p.dep[(size_t)col * mc.dep_stride + la], p.dep[a]) = good ? p.Q / plen : 0.0;   // :308
      unsigned long long gm = __ballot(good && k == 0);
      if (gm) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // lane k == 0 wrote the path
        for (; gm; gm &= gm - 1) {
          const int l = __builtin_ctzll(gm);
          const int aa = bcast_i(a, l), nn = bcast_i(n, l);
          const int* oo = p.cells + (size_t)aa * p.path_cap;
#if PF_MAACO_BATCH
          const int ll = bcast_i(la, l), cl = bcast_i(col, l);       // (the colony's matrix, at the local index)
          unsigned long long* bits = p.bits + (size_t)cl * mc.bits_stride;
          const unsigned long long bit = 1ull << (ll & 63);
          uint8_t* fl = p.flag + (size_t)cl * mc.flag_stride + (ll >> 6);
#else
          const unsigned long long bit = 1ull << (aa & 63);
          uint8_t* fl = p.flag + (aa >> 6);
#endif
          for (int i = lane; i < nn; i += 256) {                    // four cell loads in flight, then their (unwaited) atomics
            int c4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) c4[u] = i + 64 * u < nn ? oo[i + 64 * u] : -1;
#pragma unroll
            for (int u = 0; u < 4; ++u) if (c4[u] >= 0) {
              __hip_atomic_fetch_or(&PF_B(bits, p.bits)[bits_idx(c4[u], PF_B(ll, aa) >> 6, p.fstride)], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              fl[(size_t)(c4[u] >> 6) * p.fstride] = 1;
            }
          }
        }
      }
    }
    if (any_fin) {
      if (alive && done) fetch();                                   // the group's next ant starts in the next round
      if (!__ballot(alive)) break;
    }
#ifdef PF_WALK_PROBE
    pr_end = __builtin_amdgcn_s_memtime(); pr_mark += pr_end - pr_m0;
#endif
  }
#ifdef PF_WALK_PROBE
  // (diagnostic build: wave clocks in the counters the MAACO path leaves unused -- scripts/probe_walk_split.py)
  if (lane == 0) { atomicAdd(&p.cnt->pops, pr_wait); atomicAdd(&p.cnt->pushes, __builtin_amdgcn_s_memtime() - pr_t0); atomicAdd(&p.cnt->nbr, pr_rounds);
                   atomicAdd(&p.cnt->deckey, pr_mark); atomicMax(&p.cnt->pruned, __builtin_amdgcn_s_memtime() - pr_t0);
                   atomicAdd(&p.cnt->settled, pr_sel0); atomicAdd(&p.cnt->sequential, pr_sel1);
                   atomicAdd(&p.cnt->candidates, pr_head); atomicAdd(&p.cnt->path_cells, pr_act); (void)pr_emit; atomicAdd(&p.cnt->steps, pr_upd); atomicAdd(&p.cnt->overflow, pr_loop); }
#endif
  if (k == 0) {
    p.slot_epoch[slot] = epoch;
#ifndef PF_WALK_PROBE
    atomicAdd(&p.cnt->candidates, cand_tot); atomicAdd(&p.cnt->path_cells, cells_tot); atomicAdd(&p.cnt->steps, steps_tot);
    if (ovf_tot) atomicAdd(&p.cnt->overflow, ovf_tot);
#endif
  }
}
