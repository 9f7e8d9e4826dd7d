// tile_rank.h — the tile toolkit of the sort (lovasz.hip) and the select (topk_ce.hip): S segments of n elements are cut into tiles
// of TILE_ELEMS, and an element's rank among those that satisfy a predicate = the count in earlier tiles (tile_count_kernel, then
// tile_rowscan_kernel over the tiles) + the count earlier in its own tile (tile_rank: ballots and the lane number).  No atomic
// decides an order.  The kernels are templates so that both translation units may hold them (as those of gemm_core.h).  The
// names here carry tile_ (TILE_ the macros); wave_ballot, wave_popc and wave_incl_scan stand beside common.h's wave_sum.
#pragma once
#include "common.h"
#include "../../include/cenet_hip.h"

#define TILE_IT 8  // elements a thread of a tile's workgroup takes
#define TILE_ELEMS (256 * TILE_IT)

static inline bool tile_seg_ok(long S, long n) { return S >= 1 && S <= 65535 && n >= 1 && n < (1L << 31); }
// B images of H W pixels cut into segments, `per` an image: per B segments of H W elements with per_image, else per of B H W
static inline bool tile_seg_shape_ok(int B, int H, int W, int per_image, long per, long* S, long* n) {
  if (B < 1 || H < 1 || W < 1) return false;
  const long HW = (long)H * W;
  if (HW >= (1L << 31)) return false;
  *S = per_image ? per * B : per;
  *n = per_image ? HW : HW * B;
  return tile_seg_ok(*S, *n);
}

// non-negative floats order as their bits: key = bits + 1, key 0 = an element that does not count, below every other
__device__ __forceinline__ unsigned tile_key(float x, bool valid) { return valid ? __float_as_uint(x) + 1u : 0u; }
__device__ __forceinline__ float tile_key_value(unsigned key) { return __uint_as_float(key - 1u); }

typedef unsigned long long wave_mask_t;

// bit l = the predicate of lane l; every lane of the wave calls.  The host checker has no ballot: there the lanes exchange the
// predicate through its wave buffer (one wave barrier, as its shuffles do).
__device__ __forceinline__ wave_mask_t wave_ballot(bool p) {
#ifdef CENET_HOSTSIM_BUILD
  auto& s = hipsim::st();
  const int w = sim_wave(), l = sim_lane();
  auto xb = sim_xset();
  xb[w][l][0] = p ? 1 : 0;
  hipsim::wave_barrier();
  int nl = s.nthreads - w * 64;
  if (nl > 64) nl = 64;
  wave_mask_t m = 0;
  for (int j = 0; j < nl; ++j) m |= (wave_mask_t)(xb[w][j][0] & 1) << j;
  return m;
#else
  return __ballot(p);
#endif
}
__device__ __forceinline__ int wave_popc(wave_mask_t m) { return __builtin_popcountll(m); }

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl(v, lane >= o ? lane - o : lane);
    if (lane >= o) v += t;
  }
  return v;
}

// grid (T, S): cnt[s T + tile] = elements of the tile whose word satisfies pred.  Pred: seg(s) = what the predicate compares with in
// segment s, read once; operator()(word, that).
template <typename Pred>
__global__ __launch_bounds__(256) void tile_count_kernel(const unsigned* __restrict__ words, Pred pred, int* __restrict__ cnt, int n,
                                                        int T) {
  __shared__ int wtot[4];
  const int tile = blockIdx.x, s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned* w0 = words + (long)s * n;
  const unsigned with = pred.seg(s);
  int c = 0;
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const unsigned i = (unsigned)tile * TILE_ELEMS + k * 256 + threadIdx.x;
    c += wave_popc(wave_ballot(i < (unsigned)n && pred(w0[i], with)));
  }
  if (lane == 0) wtot[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[(long)s * T + tile] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// Inside a tile of 256 threads (every thread calls): wave w owns elements [w 64 IT, (w + 1) 64 IT) of the tile, item k of lane l is
// element w 64 IT + 64 k + l, so the order of the elements is (wave, item, lane) and loads are coalesced.  flag(k): the predicate
// of this lane's item k.  rank[k] <- the flagged elements of this wave before item k (INCL: and itself); wtot[w] <- the count of
// wave w; returns the count of the waves before this one.
template <bool INCL, typename F>
__device__ __forceinline__ int tile_rank(F flag, int (&rank)[TILE_IT], int (&wtot)[4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const wave_mask_t mine = (wave_mask_t)1 << lane, before = (mine - 1) | (INCL ? mine : 0);
  int run = 0;
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const wave_mask_t bal = wave_ballot(flag(k));
    rank[k] = run + wave_popc(bal & before);
    run += wave_popc(bal);
  }
  if (lane == 0) wtot[wave] = run;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  return base;
}

// Exclusive scan of every row data[r T .. r T + T) in place, totals[r] = the row's sum (totals may be null).  A group of Wd lanes
// (tile_scan_width(T): the smallest power of two <= 64 that covers T) walks its row 4 Wd values at a time, four consecutive values a
// lane; 256 / Wd rows per workgroup, grid ceil(rows Wd / 256).  I is int in every launch: the parameter is there only so that the
// kernel may be defined in this header.
template <typename I>
__global__ __launch_bounds__(256) void tile_rowscan_kernel(I* __restrict__ data, I* __restrict__ totals, long rows, int T, int Wd) {
  const long r = ((long)blockIdx.x * 256 + threadIdx.x) / Wd;
  const int gl = threadIdx.x & (Wd - 1);
  const bool live = r < rows;
  I* row = data + (live ? r : 0) * T;
  I carry = 0;
  for (int base = 0; base < T; base += 4 * Wd) {  // (the same trip count for every thread: the shuffles stay convergent)
    const int i0 = base + 4 * gl;
    I v[4], tot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) tot += v[q] = (live && i0 + q < T) ? row[i0 + q] : 0;
    I inc = tot;
    for (int o = 1; o < Wd; o <<= 1) {
      const I t = __shfl(inc, gl >= o ? gl - o : gl, Wd);
      if (gl >= o) inc += t;
    }
    I at = carry + inc - tot;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (live && i0 + q < T) row[i0 + q] = at;
      at += v[q];
    }
    carry += __shfl(inc, Wd - 1, Wd);
  }
  if (live && gl == 0 && totals) totals[r] = carry;
}
static inline int tile_scan_width(int T) {
  int w = 1;
  while (4 * w < T && w < 64) w <<= 1;
  return w;
}
static inline int tile_rowscan(int* data, int* totals, long rows, int T, hipStream_t stream) {
  const int Wd = tile_scan_width(T);
  CENET_LAUNCH(tile_rowscan_kernel<int>, dim3(cdiv(rows * Wd, 256)), dim3(256), stream, data, totals, rows, T, Wd);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
