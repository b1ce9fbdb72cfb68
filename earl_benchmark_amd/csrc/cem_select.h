// cem_select.h -- the elite set of a CEM update in O(K): a radix select over the 64-bit order-preserving keys of one env's K returns (tabletop_cem.h: cem_key), run by
// ONE workgroup of THREADS lanes (a multiple of 64) that holds the keys in registers, PER per lane: lane `tid` owns the branches k = tid + r * THREADS, r = 0 .. PER - 1.
// It names no env, no planner block and no array layout, so that any CEM update kernel can call it (device code only; the host twins sort).
//   the order    key descending, k ascending among equal keys; a key of 0 (cem_key of a NaN: below every number's key) is never selected.  That IS item 4 of the
//                CEM contracts: "k is an elite iff rank_k < E and ret[k] is not NaN".
//   the search   eight passes over the key's bytes from the top.  A pass counts, in a 256-bin LDS histogram, the byte of every key that still matches the bytes
//                decided so far (a wave whose matching keys agree on the byte adds its popcount once: equal returns -- the sparse reward's real case -- and the shared
//                exponent bytes cost one LDS atomic per wave, not one per key); wave 0 then takes a suffix sum over the bins and narrows to the bin that holds rank
//                E - 1.  After the last pass tau is the key of rank E - 1 and G = #{key > tau}.
//   the elites   every key > tau and, unless tau == 0, the first E - G branches with key == tau in ascending k: an ordered block-wide prefix count (ballot and popcount
//                inside a wave, the (round, wave) totals through LDS, scanned by wave 0).  Their indices are compacted into LDS, the keys > tau first.
// Work is O(PER) per lane per pass; every trip count is a compile-time constant; no loop exit depends on data; no global memory is touched.
#pragma once
#include <cstdint>

namespace earl {

template <int THREADS, int PER, int MAXE>
struct CemSelectLds {
  static_assert(THREADS % 64 == 0 && THREADS >= 256 && PER >= 1 && PER <= 32 && THREADS * PER < 65536 && (PER * (THREADS / 64)) % 64 == 0,
                "one lane per histogram bin in the first 256, a uint32 of flags per lane, 16-bit counts and indices, whole chunks of (round, wave) totals per lane of wave 0");
  uint32_t hist[256];                    // the pass's histogram
  uint32_t cnt[PER * (THREADS / 64)];    // per (round, wave) in k order: #{key > tau} << 16 | #{key == tau}, then the exclusive prefix sums of those
  uint32_t digit, rem;                   // a pass's decision, from wave 0 to all
  uint16_t elite[MAXE];                  // the elites' branch indices
};

// key[r] = the key of branch tid + r * THREADS (anything for a branch >= K).  1 <= E <= min(K, MAXE), K <= THREADS * PER; called by all THREADS lanes of the workgroup
// (it holds barriers).  -> Ne; L.elite[0 .. Ne) = the elites; bit r of `mine` = whether branch tid + r * THREADS is one.  L is free for reuse after the caller's next
// barrier past its last read of L.elite.
template <int THREADS, int PER, int MAXE>
__device__ __forceinline__ int cem_select(const uint64_t (&key)[PER], int K, int E, CemSelectLds<THREADS, PER, MAXE>& L, uint32_t& mine) {
  constexpr int WAVES = THREADS / 64, CH = PER * WAVES / 64;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t prefix = 0;                  // the bytes decided so far, in place
  uint32_t rem = (uint32_t)(E - 1);     // the rank still to find among the keys that match them
#pragma unroll 1
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) L.hist[tid] = 0;
    __syncthreads();
    const uint64_t decided = shift == 56 ? 0ull : ~0ull << (shift + 8);
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      if (r * THREADS < K) {            // (uniform over the workgroup)
        const bool on = tid + r * THREADS < K && ((key[r] ^ prefix) & decided) == 0;
        const uint32_t dg = (uint32_t)(key[r] >> shift) & 255u;
        const uint64_t act = __ballot(on);
        if (act != 0) {                 // (uniform over the wave)
          const int first = __ffsll((long long)act) - 1;
          const uint32_t d0 = (uint32_t)__shfl((int)dg, first);
          if (__ballot(on && dg == d0) == act) {
            if (lane == first) atomicAdd(&L.hist[d0], (uint32_t)__popcll(act));
          } else if (on) {
            atomicAdd(&L.hist[dg], 1u);
          }
        }
      }
    }
    __syncthreads();
    if (wave == 0) {                    // lane l owns bins 4 l .. 4 l + 3; `above` = the keys in the bins of the lanes above it
      const uint32_t h0 = L.hist[4 * lane], h1 = L.hist[4 * lane + 1], h2 = L.hist[4 * lane + 2], h3 = L.hist[4 * lane + 3];
      const uint32_t own = h0 + h1 + h2 + h3;
      uint32_t incl = own;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const uint32_t v = (uint32_t)__shfl_down((int)incl, s);
        if (lane + s < 64) incl += v;
      }
      const uint32_t above = incl - own;
      if (above <= rem && rem < incl) {  // (one lane: rem < the number of matching keys, because E <= K)
        uint32_t a = above, d = 3;
        if (rem >= a + h3) { a += h3; d = 2;
          if (rem >= a + h2) { a += h2; d = 1;
            if (rem >= a + h1) { a += h1; d = 0; } } }
        L.digit = 4u * (uint32_t)lane + d;
        L.rem = rem - a;
      }
    }
    __syncthreads();
    prefix |= (uint64_t)L.digit << shift;
    rem = L.rem;
  }
  const uint64_t tau = prefix;
  const uint32_t G = (uint32_t)(E - 1) - rem, take = tau != 0 ? rem + 1 : 0;      // G keys stand above tau; `take` of the keys equal to it join them

  // the (round, wave) totals in k order, and their exclusive prefix sums
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const bool valid = tid + r * THREADS < K;
    const uint64_t bg = __ballot(valid && key[r] > tau), be = __ballot(valid && key[r] == tau);
    if (lane == 0) L.cnt[r * WAVES + wave] = ((uint32_t)__popcll(bg) << 16) | (uint32_t)__popcll(be);
  }
  __syncthreads();
  if (wave == 0) {
    uint32_t v[CH], own = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      v[c] = L.cnt[lane * CH + c];
      own += v[c];
    }
    uint32_t incl = own;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)incl, s);
      if (lane >= s) incl += u;
    }
    uint32_t run = incl - own;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      L.cnt[lane * CH + c] = run;
      run += v[c];
    }
  }
  __syncthreads();

  mine = 0;
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int k = tid + r * THREADS;
    const bool valid = k < K, gt = valid && key[r] > tau, eq = valid && key[r] == tau;
    const uint64_t bg = __ballot(gt), be = __ballot(eq);
    const uint32_t base = L.cnt[r * WAVES + wave];
    const uint32_t pg = (base >> 16) + (uint32_t)__popcll(bg & below), pe = (base & 0xFFFFu) + (uint32_t)__popcll(be & below);
    const uint32_t slot = gt ? pg : G + pe;
    if ((gt || (eq && pe < take)) && slot < (uint32_t)MAXE) {   // (slot < G + take <= E <= MAXE by construction; the bound keeps a caller's bad E inside the array)
      L.elite[slot] = (uint16_t)k;
      mine |= 1u << r;
    }
  }
  __syncthreads();
  return (int)(G + take);
}

}  // namespace earl
