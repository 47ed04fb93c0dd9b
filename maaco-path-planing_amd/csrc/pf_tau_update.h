// pf_tau_update.h -- the one-pass pheromone update (K5), compiled twice by pathfit.hip: PF_MAACO_BATCH 0 gives k_tau_update,
// 1 k_tau_update_batch (grid: stretch blocks x K; block row c updates colony c with its own matrix, flags, deposits and state).
__global__ __launch_bounds__(1024) void PF_TAU_UPDATE(double* tau, const uint8_t* occ, int RC, unsigned long long* bits, int nwords,
                                                    const double* dep, double keep, const double* state, double tmin_a, double tmax_a,
                                                    uint8_t* flag, int fstride PF_COLONIES) {
#if PF_MAACO_BATCH
  {                                                                // block row c: colony c's pheromone, matrix, flags, deposits, state
    const size_t c = blockIdx.y;
    tau += c * RC; bits += c * mc.bits_stride; dep += c * mc.dep_stride; state += 13 * c; flag += c * mc.flag_stride;
  }
#endif
  extern __shared__ __attribute__((aligned(16))) double sdep[];    // [PF_UPD_CHUNK] deposits, then [PF_UPD_CHUNK] pre-scaled (dep_word_scaled)
  double* sdeps = sdep + PF_UPD_CHUNK;
  if (state && state[8] != 0.0) return;                            // an ant overflowed: the iteration is redone, tau stays
  const double tmin = state ? state[6] : tmin_a, tmax = state ? state[7] : tmax_a;
  // a wavefront owns one 64-cell stretch (512-byte word loads); the 16 wavefronts of a block take stretches gridDim.x apart, so the
  // few busy parts of the map -- around the start, the target and the corridors every ant uses -- land on different CUs
  const int lane = threadIdx.x & 63;
  const int seg = (threadIdx.x >> 6) * gridDim.x + blockIdx.x;
  const int i = seg * 64 + lane;
  const bool live = i < RC, seg_live = seg * 64 < RC;              // (seg_live is wave-uniform)
  double t = live ? tau[i] * keep : 0.0;                           // :305
#if PF_TAU_PROBE == 2
  const unsigned long long probe_t0 = __builtin_amdgcn_s_memtime();
  int probe_dense = 0, probe_chunks = 0;
#endif
  uint8_t* frow = flag + (size_t)seg * fstride;
  for (int c0 = 0; c0 < nwords; c0 += PF_UPD_CHUNK / 64) {
    const int cw = nwords - c0 < PF_UPD_CHUNK / 64 ? nwords - c0 : PF_UPD_CHUNK / 64;
    __syncthreads();
    bool big = false;                                              // a deposit of 4 or more (or a NaN) would overflow its scaling by 2^1022
    for (int k = threadIdx.x; k < cw * 64; k += blockDim.x) {
      const double v = dep[c0 * 64 + k];
      sdep[k] = v; sdeps[k] = __builtin_ldexp(v, 1023 - (1 << ((k & 63) % 11))); big |= !(v < 4.0);
    }
    const bool scaled = __syncthreads_or(big) == 0;                 // (block-uniform; Q / L is ~4e-3 with the reference's parameters)
    if (!seg_live) continue;
    for (int k0 = 0; k0 < cw; k0 += 64) {
      // which of the next 64 words have anything in this stretch: one flag byte per lane -> a wave-uniform mask, walked in word
      // (= ant) order; only those chunks are loaded at all (measured: 23 % of them at 512^2 / 16 384 ants, 14 % at 1024^2 / 8 192)
      const int wl = c0 + k0 + lane;
      const bool mine = k0 + lane < cw;
      const uint8_t f = mine ? frow[wl] : (uint8_t)0;
      if (f) frow[wl] = 0;
      unsigned long long m = __ballot(f != 0);
      // PF_TAU_FLY chunks in flight, the next PF_TAU_FLY requested before these are summed.  The loads are unconditional (an empty slot
      // re-reads chunk 0 of the stretch and is masked afterwards): loads under a branch make the compiler wait for ALL of them.
      unsigned long long* cb = bits + (size_t)seg * fstride * 64 + lane;   // bits_idx(i, w, fstride) = cb[w * 64]
      int idx[PF_TAU_FLY], nidx[PF_TAU_FLY];
      unsigned long long b[PF_TAU_FLY], nb[PF_TAU_FLY];
#pragma unroll
      for (int u = 0; u < PF_TAU_FLY; ++u) {
        idx[u] = m ? c0 + k0 + (int)__builtin_ctzll(m) : -1; m &= m - 1;
        b[u] = cb[(size_t)(idx[u] < 0 ? 0 : idx[u]) * 64];
      }
      while (idx[0] >= 0) {
#pragma unroll
        for (int u = 0; u < PF_TAU_FLY; ++u) {
          nidx[u] = m ? c0 + k0 + (int)__builtin_ctzll(m) : -1; m &= m - 1;
          nb[u] = cb[(size_t)(nidx[u] < 0 ? 0 : nidx[u]) * 64];
        }
#pragma unroll
        for (int u = 0; u < PF_TAU_FLY; ++u) {
          if (idx[u] < 0) break;                                    // (wave-uniform)
          const unsigned long long x = live ? b[u] : 0ull;
          // the matrix goes back zeroed; every lane stores (a store under a branch would again cost exact wait counts, and the
          // flagged chunks are 1/4 of the matrix)
          cb[(size_t)idx[u] * 64] = 0ull;
#if PF_TAU_PROBE == 2
          probe_chunks += 1; probe_dense += __any((int)__builtin_popcountll(x) > PF_DEP_DENSE) ? 1 : 0;
#endif
#if PF_TAU_PROBE != 1
          t = scaled ? dep_word_scaled(t, x, sdep + (idx[u] - c0) * 64, sdeps + (idx[u] - c0) * 64) : dep_word(t, x, sdep + (idx[u] - c0) * 64);
#else
          t += x == 12345ull ? 1.0 : 0.0;
#endif
        }
#pragma unroll
        for (int u = 0; u < PF_TAU_FLY; ++u) { idx[u] = nidx[u]; b[u] = nb[u]; }
      }
    }
  }
#if PF_TAU_PROBE == 2
  // (timing probe, wrong pheromone on purpose: lane 0 leaves the wave's shader clocks, lane 1 its dirty chunks, lane 2 the dense ones)
  if (live) tau[i] = lane == 0 ? (double)(__builtin_amdgcn_s_memtime() - probe_t0) : lane == 1 ? (double)probe_chunks : lane == 2 ? (double)probe_dense : t;   // (t stays live: the sums must not be optimised away)
  return;
#endif
  if (live) tau[i] = occ[i] == 1 ? 1e-9 : fmin(fmax(t, tmin), tmax);   // :326-332 (paths never cross obstacles: their words are empty)
}
