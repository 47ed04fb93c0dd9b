// pf_tile_queue.h -- the tile-queue engine behind the widest, cost and turn fields (pf_widest.h, pf_cost_field.h, pf_turn_field.h;
// DESIGN.md 4.21): what a workgroup does on entering and on leaving a queued (set, tile), and how a seed kernel fills the first
// queue.  The relax body in between -- the rule, the sweeps, the stores of the words that moved -- is the field's own.
//
// The protocol.  A field is B rows of cells cut into tiles of TW x TH; entry q = b * ntiles + ty * tiles_x + tx names tile (ty, tx)
// of set b.  There are two queues, two flag arrays (one word per entry) and two queue lengths, used by parity: the launch of round k
// reads queue k & 1 and fills queue (k + 1) & 1.  tq_enqueue puts an entry on a queue at most once: an exchange on its flag word
// admits the first caller, and an add on the queue's length gives it a slot.  The seed kernel (tq_seed_sets) fills queue 0; the
// host reads its length n and launches n workgroups, one per entry; each sweeps its tile to the fixed point under the halo it read,
// stores the words that moved and queues, for the NEXT launch, the neighbour tiles that hold a moved cell in their halo (tq_close:
// N, S, W, E for a moved border row or column, a diagonal neighbour for a moved corner cell when diagonals are allowed).  A tile never
// queues itself: it is at its fixed point until a halo word moves, and whoever moves one queues it.  In the first launch a tile also
// reports the seeds on its border, which moved in the seed kernel.  The host reads the next queue's length (4 bytes) after every
// launch and stops at 0.  On entering (tq_entry, tq_open) a workgroup clears its own flag of the current parity, so that the launch after
// next can queue the tile again, and the first workgroup clears the current queue's length: the host has read it already, and the
// word is the launch after next's.
//
// Why no more synchronisation is needed (the second half of each field's exactness argument; the first half, that every stored
// value is a valid bound and moves one way only, is the field's own).  Per-XCD L2s are not coherent with each other and a CU's L1 is
// never refreshed by another CU's stores, so a halo word that the neighbour tile is moving in the same launch may be read old or
// new.  A word has ONE writer per launch, the workgroup of its (set, tile): the flags admit an entry once per queue, so two
// workgroups never hold the same (set, tile) in one launch; it is stored whole, so a reader sees a value that was stored, never a
// mixture, and by the field's first half an old value is still a valid bound.  Whoever moved it re-queues the reader for the NEXT
// launch, and the kernel boundary in between makes the store visible: a reader that saw the old word runs again and sees the new
// one.  When no tile is queued, every tile was last relaxed from halo words that did not change afterwards: the whole array is a
// fixed point above the seeds, and the field's first half makes it the least one, whatever the timing.
// Which accesses have to be agent-scope atomics for this: the field's loads of its words into LDS and its stores of the moved
// words (relaxed __hip_atomic_load / __hip_atomic_store: whole words, not cached across the launch in a way the compiler may
// assume stable), the seed kernel's claim of a source's word, and here the exchange on the flag word and the add on the next queue's
// length.  The current queue, this round's flags and the read-only inputs are written by nobody else in the launch (a workgroup
// clears its own current flag only): plain accesses.  Kernel boundaries are the only synchronisation: no spin-wait, no cooperative
// launch, no fence across workgroups.
#pragma once

namespace pf {

// (set, tile) q goes on the queue whose length is *count, once: the flag word says it is there already
__device__ __forceinline__ void tq_enqueue(int q, int* __restrict__ flag, int* __restrict__ queue, int* __restrict__ count) {
  if (__hip_atomic_exchange(flag + q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
    queue[__hip_atomic_fetch_add(count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = q;
}

struct tq_visit { int q, b, ty, tx, ntiles; };                       // this workgroup's queue entry, taken apart

// the visit's two LDS words: the side bits of the cells that moved, and the words that moved
struct tq_words { int sides, moved; };
__device__ __forceinline__ tq_words& tq_lds() { __shared__ tq_words w; return w; }

// Opening a visit, in two steps so that a kernel may form its pointers in between (its loads then issue ahead of the stores here):
// the entry of this workgroup; then its flag and the two LDS words are cleared, and the first workgroup clears the current queue's
// length.  The caller's first barrier publishes the LDS words.
__device__ __forceinline__ tq_visit tq_entry(const int* queue, int tiles_x, int tiles_y) {
  const int q = queue[blockIdx.x], ntiles = tiles_x * tiles_y;
  const int b = q / ntiles, t = q - b * ntiles, ty = t / tiles_x, tx = t - ty * tiles_x;
  return {q, b, ty, tx, ntiles};
}
__device__ __forceinline__ void tq_open(const tq_visit& v, int* flag_now, int* count_now) {
  if (threadIdx.x == 0) { flag_now[v.q] = 0; tq_lds().sides = 0; tq_lds().moved = 0; }
  if (threadIdx.x == 0 && blockIdx.x == 0) *count_now = 0;           // the host has read this queue's length: the word is the launch after next's
}

// The neighbour tiles that hold cell (lr, lcn) of a TW x TH tile in their halo: bits 0..3 N, S, W, E; bits 4..7 NW, NE, SW, SE
template <int TW, int TH>
__device__ __forceinline__ int tq_side_bits(int lr, int lcn) {
  const int n = lr == 0, s = lr == TH - 1, wst = lcn == 0, e = lcn == TW - 1;
  return n | (s << 1) | (wst << 2) | (e << 3) | ((n & wst) << 4) | ((n & e) << 5) | ((s & wst) << 6) | ((s & e) << 7);
}

// Closing a visit: every thread brings the side bits of its moved cells and their number; the neighbour tiles named by the bits of
// the whole workgroup go on the next queue (4 threads, 8 with diagonals) and the words moved are added to the call's counter.
__device__ __forceinline__ void tq_close(const tq_visit& v, int sides, int moved, int allow_diag, int tiles_x, int tiles_y,
                                         int* flag_next, int* queue_next, int* count_next, unsigned long long* moved_total) {
  const int tid = (int)threadIdx.x;
  tq_words& lds = tq_lds();
  if (sides) atomicOr(&lds.sides, sides);
  if (moved) atomicAdd(&lds.moved, moved);
  __syncthreads();
  if (tid < (allow_diag ? 8 : 4) && ((lds.sides >> tid) & 1)) {
    const int dy = (tid == 0 || tid == 4 || tid == 5) ? -1 : (tid == 1 || tid == 6 || tid == 7) ? 1 : 0;
    const int dx = (tid == 2 || tid == 4 || tid == 6) ? -1 : (tid == 3 || tid == 5 || tid == 7) ? 1 : 0;
    const int ny = v.ty + dy, nx = v.tx + dx;
    if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x) tq_enqueue(v.b * v.ntiles + ny * tiles_x + nx, flag_next, queue_next, count_next);
  }
  if (tid == 0 && lds.moved) atomicAdd(moved_total, (unsigned long long)lds.moved);
}

// The body of a seed kernel: one thread per listed source of every set.  claim(b, s) makes cell s a seed of row b and says whether
// this listing counted (false: no source there, or listed before); what counted is added to nsrc[b] and its tile goes on the queue.
template <int THREADS, int TW, int TH, typename Claim>
__device__ __forceinline__ void tq_seed_sets(int RC, int C, int tiles_x, int ntiles, int B, const int* __restrict__ off, const int* __restrict__ src,
                                             int* __restrict__ flag, int* __restrict__ queue, int* __restrict__ count, unsigned long long* __restrict__ nsrc,
                                             Claim claim) {
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const int end = off[b + 1];
    int counted = 0;
    for (int j = off[b] + (int)(blockIdx.x * THREADS + threadIdx.x); j < end; j += (int)(gridDim.x * THREADS)) {
      const int s = src[j];
      if ((unsigned)s >= (unsigned)RC) continue;                     // (the host has checked the ids)
      if (!claim(b, s)) continue;
      counted += 1;
      const int r = s / C, c = s - r * C;
      tq_enqueue(b * ntiles + (r / TH) * tiles_x + c / TW, flag, queue, count);
    }
    if (counted) atomicAdd(nsrc + b, (unsigned long long)counted);
  }
}

}  // namespace pf
