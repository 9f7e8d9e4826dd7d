// wave_ballot.h — ballots, their population count and a wave's inclusive scan, shared by lovasz.hip and topk_ce.hip: the pieces a
// rank inside a tile is made of (no atomic decides an order).  The host checker has no ballot; it goes through its wave buffer.
#pragma once
#include "common.h"

typedef unsigned long long lv_mask_t;

// bit l = the predicate of lane l; every lane of the wave calls.  The host checker has no ballot: there the lanes exchange the
// predicate through its wave buffer (one wave barrier, as its shuffles do).
__device__ __forceinline__ lv_mask_t lv_ballot(bool p) {
#ifdef CENET_HOSTSIM_BUILD
  auto& s = hipsim::st();
  const int w = sim_wave(), l = sim_lane();
  auto xb = sim_xset();
  xb[w][l][0] = p ? 1 : 0;
  hipsim::wave_barrier();
  int nl = s.nthreads - w * 64;
  if (nl > 64) nl = 64;
  lv_mask_t m = 0;
  for (int j = 0; j < nl; ++j) m |= (lv_mask_t)(xb[w][j][0] & 1) << j;
  return m;
#else
  return __ballot(p);
#endif
}
__device__ __forceinline__ int lv_popc(lv_mask_t m) { return __builtin_popcountll(m); }

__device__ __forceinline__ int lv_wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl(v, lane >= o ? lane - o : lane);
    if (lane >= o) v += t;
  }
  return v;
}
