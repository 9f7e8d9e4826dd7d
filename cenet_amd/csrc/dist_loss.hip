// dist_loss.hip — the two distance-map losses on the boundary-distance maps of edt.hip (cenet_dist_maps_*), as one fused pair.
//   surface (boundary) loss, Kervadec et al. 2019:  softmax probability times the signed distance map of the ground truth
//   Hausdorff-DT loss, Karimi & Salcudean 2019, alpha = 2:  squared error times the squared distance maps of ground truth and
//                                                           thresholded prediction
// With N = B (K-1) H W, p = softmax(logits), g_c = [label == c], d2g / d2p the int32 maps of planes (b, c), c = 1 .. K-1:
//   phi_c  = +sqrt(d2g_c) outside class c,  -(sqrt(d2g_c) - 1) inside          L_surf = 1/N sum p_c phi_c
//   L_hd   = 1/N sum (p_c - g_c)^2 (d2g_c + d2p_c)                             loss = w[0] L_surf + w[1] L_hd
// w: two floats in DEVICE memory, read by every launch (a graph replay sees what was last written there).  A term that is not
// present is left out, not multiplied by 0; without the Hausdorff term d2p is never read.  The maps are constants: no gradient
// flows through the threshold.
// STORE-AND-SUM (loss_pixel.h): workgroup g of the forward stores its two partial sums as row g of the workspace, a
// one-workgroup launch adds the rows in a fixed order in double.  No float atomics: loss and gradient are bitwise reproducible.
// Backward, one launch: a_j = w[0] phi_j + 2 w[1] (p_j - g_j)(d2g_j + d2p_j), a_0 = 0;  dlogit_j = gout p_j (a_j - sum_c p_c a_c) / N.
#include "loss_pixel.h"
#include "../../include/cenet_hip.h"

enum { DL_SURFACE = 1, DL_HAUSDORFF = 2 };

static inline int dl_fwd_it(int K) { return K > 9 ? 4 : 8; }  // pixels per thread of the forward kernel
static inline long dl_rows(int B, int K, long HW) { return (long)cdiv(HW, 256 * dl_fwd_it(K)) * B; }
static inline bool dl_shape_ok(int B, int K, int H, int W) {
  return B > 0 && B <= 65535 && K >= 2 && K <= PX_MAXK && H >= 1 && W >= 1 && (long)H * W <= 0x7fffffffL - 256 * 8;
}

extern "C" long cenet_dist_loss_ws_floats(int B, int K, int H, int W) {
  if (!dl_shape_ok(B, K, H, W)) return 0;
  return 2 * dl_rows(B, K, (long)H * W);
}

__device__ __forceinline__ float dl_phi(int d2g, bool inside) {
  const float d = sqrtf((float)d2g);
  return inside ? 1.f - d : d;
}

// grid (ceil(HW / (256 IT)), B): a thread owns IT pixels of image blockIdx.y, consecutive lanes on consecutive pixels of every
// plane it reads (K logit planes, the labels, K - 1 planes of each map)
template <typename T, int KM>
__global__ __launch_bounds__(256) void dl_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ labels,
                                                    const int* __restrict__ d2g, const int* __restrict__ d2p,
                                                    float* __restrict__ rows, int K, int HW, int flags) {
  __shared__ float wred[4][2];
  constexpr int IT = KM > 9 ? 4 : 8;
  const bool surf = flags & DL_SURFACE, hd = flags & DL_HAUSDORFF;
  const int b = blockIdx.y;
  const T* lb0 = logits + (long)b * K * HW;
  const float* lab = labels + (long)b * HW;
  const int* g0 = d2g + (long)b * (K - 1) * HW;
  const int* p0 = hd ? d2p + (long)b * (K - 1) * HW : nullptr;
  float sum[2] = {0.f, 0.f};  // surface, Hausdorff
#pragma unroll 2
  for (int k = 0; k < IT; ++k) {
    const int p = (blockIdx.x * IT + k) * 256 + threadIdx.x;
    if (p >= HW) continue;
    float v[KM];
    int dg[KM], dp[KM];
#pragma unroll
    for (int c = 0; c < KM; ++c)  // (class by class, a logit between its two maps)
      if (c < K) {
        v[c] = ldf(lb0 + (long)c * HW + p);
        dg[c] = c ? g0[(long)(c - 1) * HW + p] : 0;
        dp[c] = (c && hd) ? p0[(long)(c - 1) * HW + p] : 0;
      }
    const float t = lab[p];
    px_softmax<KM, false>(v, K);
#pragma unroll
    for (int c = 1; c < KM; ++c)
      if (c < K) {
        const bool in = t == (float)c;
        if (surf) sum[0] += v[c] * dl_phi(dg[c], in);
        if (hd) {
          const float e = v[c] - (in ? 1.f : 0.f);
          sum[1] += e * e * ((float)dg[c] + (float)dp[c]);
        }
      }
  }
  block_store_row(sum, wred, rows + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

__global__ __launch_bounds__(1024) void dl_finalize_kernel(const float* __restrict__ rows, const float* __restrict__ w,
                                                          float* __restrict__ loss, long nrows, double inv_n, int flags) {
  __shared__ double acc[2][1024];
  double sum[2];  // surface, Hausdorff
  rows_sum_f64(acc, nrows, [&](long r, int j) { return (double)rows[2 * r + j]; }, sum);
  if (threadIdx.x == 0) {
    double l = 0.0;
    if (flags & DL_SURFACE) l += (double)w[0] * sum[0] * inv_n;
    if (flags & DL_HAUSDORFF) l += (double)w[1] * sum[1] * inv_n;
    loss[0] = (float)l;
  }
}

template <typename T, int KM>
__global__ __launch_bounds__(256) void dl_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ labels,
                                                    const int* __restrict__ d2g, const int* __restrict__ d2p,
                                                    const float* __restrict__ w, const float* __restrict__ gout,
                                                    T* __restrict__ dlogits, int K, int HW, float inv_n, int flags) {
  constexpr int IT = 4;  // grid (ceil(HW / (256 IT)), B)
  const bool surf = flags & DL_SURFACE, hd = flags & DL_HAUSDORFF;
  const float go = gout[0] * inv_n, ws = surf ? w[0] : 0.f, wh2 = hd ? 2.f * w[1] : 0.f;
  const int b = blockIdx.y;
  const T* lb0 = logits + (long)b * K * HW;
  T* db0 = dlogits + (long)b * K * HW;
  const float* lab = labels + (long)b * HW;
  const int* g0 = d2g + (long)b * (K - 1) * HW;
  const int* p0 = hd ? d2p + (long)b * (K - 1) * HW : nullptr;
#pragma unroll 2
  for (int k = 0; k < IT; ++k) {
    const int p = (blockIdx.x * IT + k) * 256 + threadIdx.x;
    if (p >= HW) continue;
    float v[KM], a[KM];
    int dg[KM], dp[KM];
#pragma unroll
    for (int c = 0; c < KM; ++c)  // (class by class, a logit between its two maps)
      if (c < K) {
        v[c] = ldf(lb0 + (long)c * HW + p);
        dg[c] = c ? g0[(long)(c - 1) * HW + p] : 0;
        dp[c] = (c && hd) ? p0[(long)(c - 1) * HW + p] : 0;
      }
    const float t = lab[p];
    px_softmax<KM, false>(v, K);
    float dot = 0.f;
    a[0] = 0.f;
#pragma unroll
    for (int c = 1; c < KM; ++c)
      if (c < K) {
        const bool in = t == (float)c;
        float ac = 0.f;
        if (surf) ac = ws * dl_phi(dg[c], in);
        if (hd) ac += wh2 * (v[c] - (in ? 1.f : 0.f)) * ((float)dg[c] + (float)dp[c]);
        a[c] = ac;
        dot += v[c] * ac;
      }
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) stf(db0 + (long)c * HW + p, go * v[c] * (a[c] - dot));
  }
}

static int dl_check(const void* logits, const float* labels, const int* d2g, const int* d2p, const float* w, int B, int K, int H,
                    int W, int surface, int hausdorff) {
  if (!dl_shape_ok(B, K, H, W) || (!surface && !hausdorff)) return CENET_EINVAL;
  if (!logits || !labels || !d2g || !w || (hausdorff && !d2p)) return CENET_EINVAL;
  return CENET_OK;
}

template <typename T>
static int dist_loss_fwd_impl(const T* logits, const float* labels, const int* d2g, const int* d2p, const float* w, float* ws,
                              long ws_floats, float* loss, int B, int K, int H, int W, int surface, int hausdorff,
                              hipStream_t stream) {
  const int rc = dl_check(logits, labels, d2g, d2p, w, B, K, H, W, surface, hausdorff);
  if (rc != CENET_OK) return rc;
  if (!ws || !loss || ws_floats < cenet_dist_loss_ws_floats(B, K, H, W)) return CENET_EINVAL;
  const int HW = H * W, flags = (surface ? DL_SURFACE : 0) | (hausdorff ? DL_HAUSDORFF : 0);
  const dim3 blocks(cdiv(HW, 256 * dl_fwd_it(K)), B);
  CENET_LAUNCH_KM(dl_fwd_kernel, T, K, blocks, dim3(256), stream, logits, labels, d2g, d2p, ws, K, HW, flags);
  CENET_CHECK_LAUNCH();
  const double inv_n = 1.0 / ((double)B * (K - 1) * HW);
  CENET_LAUNCH(dl_finalize_kernel, dim3(1), dim3(1024), stream, (const float*)ws, w, loss, dl_rows(B, K, HW), inv_n, flags);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(dist_loss_fwd, (const T* logits, const float* labels, const int* d2g, const int* d2p, const float* w, float* ws,
                           long ws_floats, float* loss, int B, int K, int H, int W, int surface, int hausdorff, hipStream_t stream),
           (logits, labels, d2g, d2p, w, ws, ws_floats, loss, B, K, H, W, surface, hausdorff, stream))

template <typename T>
static int dist_loss_bwd_impl(const T* logits, const float* labels, const int* d2g, const int* d2p, const float* w,
                              const float* gout, T* dlogits, int B, int K, int H, int W, int surface, int hausdorff,
                              hipStream_t stream) {
  const int rc = dl_check(logits, labels, d2g, d2p, w, B, K, H, W, surface, hausdorff);
  if (rc != CENET_OK) return rc;
  if (!gout || !dlogits) return CENET_EINVAL;
  const int HW = H * W, flags = (surface ? DL_SURFACE : 0) | (hausdorff ? DL_HAUSDORFF : 0);
  const dim3 blocks(cdiv(HW, 256 * 4), B);
  const float inv_n = (float)(1.0 / ((double)B * (K - 1) * HW));
  CENET_LAUNCH_KM(dl_bwd_kernel, T, K, blocks, dim3(256), stream, logits, labels, d2g, d2p, w, gout, dlogits, K, HW, inv_n, flags);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(dist_loss_bwd, (const T* logits, const float* labels, const int* d2g, const int* d2p, const float* w, const float* gout,
                           T* dlogits, int B, int K, int H, int W, int surface, int hausdorff, hipStream_t stream),
           (logits, labels, d2g, d2p, w, gout, dlogits, B, K, H, W, surface, hausdorff, stream))
