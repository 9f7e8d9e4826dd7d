// loss_pixel.h — what the per-pixel loss files (seg_loss_ex.hip, dist_loss.hip, lovasz.hip, topk_ce.hip) share: one pixel's K class
// values in registers (load, softmax), the launch by class bound, and the two halves of STORE-AND-SUM — a workgroup's
// partial sums stored as a row, the rows added by one workgroup in double.  The order of the additions written here is what
// makes those losses bitwise reproducible: it is written once.  loss_optim.hip includes it for CENET_LAUNCH_KM alone.
#pragma once
#include "common.h"

#define PX_MAXK 16

// KM: compile-time bound of the class loops (4 / 9 / 16); kernel<T, KM> is launched with the smallest that holds K
#define CENET_LAUNCH_KM(kernel, T, K, grid, block, stream, ...)                               \
  do {                                                                                         \
    if ((K) <= 4) CENET_LAUNCH((kernel<T, 4>), grid, block, stream, __VA_ARGS__);              \
    else if ((K) <= 9) CENET_LAUNCH((kernel<T, 9>), grid, block, stream, __VA_ARGS__);         \
    else CENET_LAUNCH((kernel<T, PX_MAXK>), grid, block, stream, __VA_ARGS__);                 \
  } while (0)

// pixel p of the K planes of HW elements at base: consecutive lanes on consecutive pixels of every plane
template <int KM, typename T>
__device__ __forceinline__ void px_load(float* v, const T* base, int HW, long p, int K) {
#pragma unroll
  for (int c = 0; c < KM; ++c)
    if (c < K) v[c] = ldf(base + (long)c * HW + p);
}

// softmax of one pixel's K logits, in place.  EXACT: libm's expf and an IEEE division a class, not v_exp_f32 and one v_rcp_f32 —
// where the order of near-equal keys follows the probabilities' last bits (lovasz.hip, topk_ce.hip)
template <int KM, bool EXACT>
__device__ __forceinline__ void px_softmax(float* v, int K) {
  float mx = -3.4e38f;
#pragma unroll
  for (int c = 0; c < KM; ++c)
    if (c < K) mx = fmaxf(mx, v[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < KM; ++c)
    if (c < K) {
      v[c] = EXACT ? expf(v[c] - mx) : fast_exp(v[c] - mx);
      s += v[c];
    }
  const float inv = EXACT ? 0.f : fast_rcp(s);
#pragma unroll
  for (int c = 0; c < KM; ++c)
    if (c < K) v[c] = EXACT ? v[c] / s : v[c] * inv;
}

// The NV partial sums of a workgroup of 256 threads (every thread calls): wave sums -> LDS -> the four waves added in a fixed
// order -> row[0 .. NV), one lane a value
template <int NV>
__device__ __forceinline__ void block_store_row(const float (&val)[NV], float (&wred)[4][NV], float* __restrict__ row) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float s = wave_sum(val[j]);
    if (lane == 0) wred[wave][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int j = threadIdx.x;
    row[j] = (wred[0][j] + wred[1][j]) + (wred[2][j] + wred[3][j]);
  }
}

// The finalize launch, one workgroup of 1024 threads (every thread calls): for each of the NV values of a row, thread t adds
// value(r, j) of the rows r = t, t + 1024, ... in double, then one tree over the threads takes the NV sums along.  sum[j]: for
// thread 0.
template <int NV, typename F>
__device__ __forceinline__ void rows_sum_f64(double (&acc)[NV][1024], long nrows, F value, double (&sum)[NV]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < NV; ++j) sum[j] = 0.0;
  for (long r = t; r < nrows; r += 1024) {
#pragma unroll
    for (int j = 0; j < NV; ++j) sum[j] += value(r, j);
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j][t] = sum[j];
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j][t] += acc[j][t + off];
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) sum[j] = acc[j][0];
}
