// augment_ops.hip — composable slice augmentation on the device: the operator family of the Synapse training pipeline
// (src/datasets/dataset_synapse.py:86-112: SomeOf((0, 4), [flips, noise, blur, contrast, four affine warps, a piecewise-affine
// mesh warp], random_order=True)) for a whole batch of device-resident slices.
//
// The reference runs imgaug on the host, one sample at a time; its random stream and its cv2 interpolation cannot be pinned
// without the library.  What is built here is the operator FAMILY, each operator specified by scipy (as ccl.hip and edt.hip are)
// and the DISTRIBUTION of the pipeline (cenet_amd/data.py SegAugmenter.draw) — not imgaug's numbers.
//
//   op            image                                                                  label
//   0 copy        v                                                                      same
//   1 flip_ud     a[H-1-i][j]                                                            same map
//   2 flip_lr     a[i][W-1-j]                                                            same map
//   3 affine      affine_transform(a64, M, offset, order=1, mode='constant', cval=0)     order=0
//   4 grid_warp   map_coordinates(order=1, mode='constant', cval=0) at (i + dY, j + dX)  order=0
//   5 blur        gaussian_filter(a64, sigma, mode='mirror', truncate=4), axis 0 then 1  unchanged
//   6 noise       v + scale * z(p), z from Philox4x32-10 + Box-Muller                    unchanged
//   7 contrast    c + alpha * (v - c)                                                    unchanged
//
// One launch per stage, grid (tiles, B): stage s of sample b executes op word tab[b][3 + s] with the parameter row dp[b][s],
// reading the pools (s = 0) or work buffer s & 1 and writing work buffer (s + 1) & 1, so the result of S stages is in buffer
// S & 1.  Every stage reads fp32 images, computes in fp64 WITHOUT fused multiply-adds (spline3.h's pragma) in scipy's operation
// order, from matrices / displacements / weights the host computed in fp64, and stores fp32; labels are uint8 throughout.  A
// workgroup owns an 8 x 32 tile of the output: the warps gather from a 2-D neighbourhood of the source, the blur keeps its
// axis-0 pass of the tile and its halo columns in LDS (fp64, as scipy's intermediate array is) and runs the axis-1 pass from
// there.  No atomics: two runs are bit-identical.
#include "common.h"
#include "../../include/cenet_hip.h"
#include "augment_ops.h"  // Philox, the tap order; fp contraction off from here on

#define AOP_MAX_GRID 16

enum { AOP_COPY = 0, AOP_FLIP_UD, AOP_FLIP_LR, AOP_AFFINE, AOP_GRID_WARP, AOP_BLUR, AOP_NOISE, AOP_CONTRAST, AOP_COUNT };

// one standard normal per pixel: counter (p, 0, 0, 0), Box-Muller on the first two output words
__device__ __forceinline__ double aop_normal(unsigned p, unsigned k0, unsigned k1) {
  unsigned c[4] = {p, 0u, 0u, 0u};
  aop_philox4x32_10(c, k0, k1);
  const double u1 = ((double)c[0] + 0.5) / 4294967296.0, u2 = ((double)c[1] + 0.5) / 4294967296.0;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
}

// scipy NI_GeometricTransform at (cy, cx), mode='constant', cval=0: outside [0, len - 1] -> 0 for image and label; the label reads
// floor(c + 0.5) (order 0), the image the four neighbours with weights (1 - f, f), rows outer, each tap value * wy * wx
__device__ __forceinline__ void aop_sample(const float* __restrict__ src, const unsigned char* __restrict__ srl, int H, int W, double cy,
                                           double cx, float& v, unsigned char& l) {
  if (cy < 0.0 || cy > (double)(H - 1) || cx < 0.0 || cx > (double)(W - 1)) {
    v = 0.f;
    l = 0;
    return;
  }
  l = srl[(long)(int)floor(cy + 0.5) * W + (int)floor(cx + 0.5)];
  const int y0 = (int)floor(cy), x0 = (int)floor(cx);
  const double fy = cy - (double)y0, fx = cx - (double)x0;
  const int y1 = y0 + 1 < H ? y0 + 1 : y0, x1 = x0 + 1 < W ? x0 + 1 : x0;  // (a tap past the edge has weight 0)
  const double wy[2] = {1.0 - fy, fy}, wx[2] = {1.0 - fx, fx};
  const float* r0 = src + (long)y0 * W;
  const float* r1 = src + (long)y1 * W;
  double t = 0.0;
  t += (double)r0[x0] * wy[0] * wx[0];
  t += (double)r0[x1] * wy[0] * wx[1];
  t += (double)r1[x0] * wy[1] * wx[0];
  t += (double)r1[x1] * wy[1] * wx[1];
  v = (float)t;
}

// bilinear sample of an R x C control grid D at (r0 + fy, c0 + fx)
__device__ __forceinline__ double aop_grid_at(const double* __restrict__ D, int C, int r0, int c0, double fy, double fx) {
  const double* a = D + r0 * C + c0;
  return (1.0 - fy) * ((1.0 - fx) * a[0] + fx * a[1]) + fy * ((1.0 - fx) * a[C] + fx * a[C + 1]);
}

// grid (tiles, B)
__global__ __launch_bounds__(256) void aug_ops_stage_kernel(const float* __restrict__ src_img, const unsigned char* __restrict__ src_lab,
                                                           int from_pool, const long* __restrict__ tab, const double* __restrict__ dp,
                                                           float* __restrict__ dst_img, unsigned char* __restrict__ dst_lab, long stride,
                                                           int S, int s) {
  __shared__ double col[AOP_TH][AOP_TW + 2 * AOP_MAX_RADIUS];
  const int b = blockIdx.y;
  const long* t = tab + (long)b * (3 + S);
  const int H = (int)t[1], W = (int)t[2];
  const long word = t[3 + s];
  const int op = (int)(word & 255);
  const long base = from_pool ? t[0] : (long)b * stride;
  const float* src = src_img + base;
  const unsigned char* srl = src_lab + base;
  float* di = dst_img + (long)b * stride;
  unsigned char* dl = dst_lab + (long)b * stride;
  const double* q = dp + ((long)b * S + s) * AOP_DP;
  const int ty = threadIdx.x / AOP_TW, tx = threadIdx.x % AOP_TW;
  const int tiles_x = (W + AOP_TW - 1) / AOP_TW, tiles = ((H + AOP_TH - 1) / AOP_TH) * tiles_x;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (the trip count is the same for every thread of the block)
    const int i0 = (tile / tiles_x) * AOP_TH, j0 = (tile % tiles_x) * AOP_TW;
    const int i = i0 + ty, j = j0 + tx;
    const bool live = i < H && j < W;
    const long p = (long)i * W + j;
    if (op == AOP_BLUR) {
      const int radius = (int)q[0];
      const double* w = q + 1;  // w[0] the centre weight, w[k] = the weight of both taps at distance k
      const int cols = AOP_TW + 2 * radius;
      for (int e = threadIdx.x; e < AOP_TH * cols; e += 256) {  // axis 0, for the tile's columns and `radius` more on either side
        const int ey = e / cols, ex = e - ey * cols;
        const int r = i0 + ey;
        double v = 0.0;
        if (r < H) {
          const float* a = src + aug_mirror(j0 + ex - radius, W);
#define AOP_AT0(k) (double)a[(long)aug_mirror(r + (k), H) * W]
          AOP_SYMMETRIC_TAPS(AOP_AT0)
#undef AOP_AT0
          v = acc;
        }
        col[ey][ex] = v;
      }
      __syncthreads();
      if (live) {  // axis 1, from the fp64 intermediate
        const double* a = &col[ty][tx + radius];
#define AOP_AT1(k) a[(k)]
        AOP_SYMMETRIC_TAPS(AOP_AT1)
#undef AOP_AT1
        di[p] = (float)acc;
        dl[p] = srl[p];
      }
      __syncthreads();  // the next tile overwrites col
      continue;
    }
    if (!live) continue;
    float v;
    unsigned char l;
    if (op == AOP_FLIP_UD || op == AOP_FLIP_LR) {
      const long sp = op == AOP_FLIP_UD ? (long)(H - 1 - i) * W + j : (long)i * W + (W - 1 - j);
      v = src[sp];
      l = srl[sp];
    } else if (op == AOP_AFFINE) {
      // scipy accumulates every coordinate component over the output axes, then adds the shift
      double cy = 0.0, cx = 0.0;
      cy += (double)i * q[0];
      cy += (double)j * q[1];
      cy += q[4];
      cx += (double)i * q[2];
      cx += (double)j * q[3];
      cx += q[5];
      aop_sample(src, srl, H, W, cy, cx, v, l);
    } else if (op == AOP_GRID_WARP) {
      const int R = (int)((word >> 8) & 255), C = (int)((word >> 16) & 255);
      const double gy = H > 1 ? (double)i * ((double)(R - 1) / (double)(H - 1)) : 0.0;
      const double gx = W > 1 ? (double)j * ((double)(C - 1) / (double)(W - 1)) : 0.0;
      int r0 = (int)floor(gy), c0 = (int)floor(gx);
      r0 = r0 < R - 2 ? r0 : R - 2;
      c0 = c0 < C - 2 ? c0 : C - 2;
      const double fy = gy - (double)r0, fx = gx - (double)c0;
      const double cy = (double)i + aop_grid_at(q, C, r0, c0, fy, fx);
      const double cx = (double)j + aop_grid_at(q + AOP_MAX_GRID, C, r0, c0, fy, fx);
      aop_sample(src, srl, H, W, cy, cx, v, l);
    } else {
      const double a = (double)src[p];
      l = srl[p];
      if (op == AOP_NOISE) v = (float)(a + q[0] * aop_normal((unsigned)p, (unsigned)q[1], (unsigned)q[2]));
      else if (op == AOP_CONTRAST) v = (float)(q[1] + q[0] * (a - q[1]));
      else v = src[p];
    }
    di[p] = v;
    dl[p] = l;
  }
}

// tab_host / dp_host: the tables as the host drew them, read here before anything is launched; tab / dp: their device copies
extern "C" int cenet_augment_ops(const float* pool_img, const unsigned char* pool_lab, const long* tab_host, const double* dp_host,
                                 const long* tab, const double* dp, float* work_img0, unsigned char* work_lab0, float* work_img1,
                                 unsigned char* work_lab1, long stride, int max_h, int max_w, int B, int S, hipStream_t stream) {
  if (!pool_img || !pool_lab || !tab_host || !dp_host || !tab || !dp || !work_img0 || !work_lab0 || !work_img1 || !work_lab1)
    return CENET_EINVAL;
  if (B <= 0 || B > 65535 || S < 1 || S > AOP_MAX_STAGES || max_h <= 0 || max_w <= 0 || stride <= 0) return CENET_EINVAL;
  if (work_img0 == work_img1 || work_lab0 == work_lab1) return CENET_EINVAL;
  for (int b = 0; b < B; ++b) {
    const long* t = tab_host + (long)b * (3 + S);
    if (t[0] < 0 || t[1] < 1 || t[2] < 1 || t[1] > max_h || t[2] > max_w || t[1] * t[2] > stride) return CENET_EINVAL;
    for (int s = 0; s < S; ++s) {
      const long word = t[3 + s];
      const long op = word & 255, R = (word >> 8) & 255, C = (word >> 16) & 255;
      const double* q = dp_host + ((long)b * S + s) * AOP_DP;
      if (word < 0 || op >= AOP_COUNT || (word >> 24) != 0) return CENET_EINVAL;
      if (op == AOP_GRID_WARP) {
        if (R < 2 || C < 2 || R * C > AOP_MAX_GRID) return CENET_EINVAL;
      } else if (word != op) {
        return CENET_EINVAL;
      }
      if (op == AOP_BLUR && !(q[0] >= 0.0 && q[0] <= (double)AOP_MAX_RADIUS && q[0] == (double)(int)q[0])) return CENET_EINVAL;
      if (op == AOP_NOISE && !(q[1] >= 0.0 && q[1] < 4294967296.0 && q[2] >= 0.0 && q[2] < 4294967296.0)) return CENET_EINVAL;
    }
  }
  float* wi[2] = {work_img0, work_img1};
  unsigned char* wl[2] = {work_lab0, work_lab1};
  const int tiles = cdiv(max_h, AOP_TH) * cdiv(max_w, AOP_TW);
  for (int s = 0; s < S; ++s) {
    const float* si = s == 0 ? pool_img : wi[s & 1];
    const unsigned char* sl = s == 0 ? pool_lab : wl[s & 1];
    CENET_LAUNCH(aug_ops_stage_kernel, dim3(tiles, B), dim3(256), stream, si, sl, (int)(s == 0), tab, dp, wi[(s + 1) & 1],
                 wl[(s + 1) & 1], stride, S, s);
  }
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

__global__ __launch_bounds__(256) void aug_philox_kernel(const long* __restrict__ ctr_key, long* __restrict__ out, int n) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const long* in = ctr_key + (long)r * 6;
  unsigned c[4] = {(unsigned)in[0], (unsigned)in[1], (unsigned)in[2], (unsigned)in[3]};
  aop_philox4x32_10(c, (unsigned)in[4], (unsigned)in[5]);
  for (int k = 0; k < 4; ++k) out[(long)r * 4 + k] = (long)c[k];
}

extern "C" int cenet_philox4x32_10(const long* ctr_key, long* out, int n, hipStream_t stream) {
  if (!ctr_key || !out || n <= 0) return CENET_EINVAL;
  CENET_LAUNCH(aug_philox_kernel, dim3(cdiv(n, 256)), dim3(256), stream, ctr_key, out, n);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// Normalize([mean], [std]) of the reference's norm_x_transform: (v - mean) / std in fp32, in place
__global__ __launch_bounds__(256) void aug_normalize_kernel(float* __restrict__ x, long n, float mean, float std) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)gridDim.x * 256) x[p] = (x[p] - mean) / std;
}

extern "C" int cenet_augment_normalize(float* x, long n, float mean, float std, hipStream_t stream) {
  if (!x || n <= 0 || !(std != 0.f)) return CENET_EINVAL;
  CENET_LAUNCH(aug_normalize_kernel, dim3(cdiv(n, 256 * 4)), dim3(256), stream, x, n, mean, std);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
