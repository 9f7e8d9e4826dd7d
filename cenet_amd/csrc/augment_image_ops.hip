// augment_image_ops.hip — composable augmentation of multi-channel images on the device: the operator family of the skin training
// pipeline (src/datasets/skin/dataset_ham.py:273-281, dataset_ph2.py:250-257: albumentations Compose([Rotate, HorizontalFlip,
// VerticalFlip, RandomBrightnessContrast, GaussianBlur, ElasticTransform]), then a per-sample min-max, :113) for a whole batch of
// device-resident samples of one size H x W with C planar channels and one uint8 label plane.
//
// The reference runs albumentations on the host, one sample at a time; its random stream, its cv2 interpolation and its uint8 LUT
// rounding cannot be pinned without the library.  What is built here is the operator FAMILY, each operator specified by scipy /
// numpy, and the DISTRIBUTION of the pipeline (cenet_amd/data.py ComposeAugmenter.draw) — not albumentations' numbers.
//
//   op                      image, every channel c (a64 = img[c] as float64)                                       label
//   0 copy                  v                                                                                      same
//   1 flip_ud               a[H-1-i][j]                                                                            same map
//   2 flip_lr               a[i][W-1-j]                                                                            same map
//   3 affine                affine_transform(a64, M, offset, order=1, mode=m, cval=0)                              order=0
//   4 blur                  correlate1d(correlate1d(a64, w, 0, mode='mirror'), w, 1, mode='mirror')                unchanged
//   5 brightness_contrast   np.clip(alpha * a64 + beta, lo, hi)                                                    unchanged
//   6 elastic               map_coordinates(a64, [i + alpha * g[0], j + alpha * g[1]], order=1, mode=m, cval=0)    order=0
// m = 'constant', or 'mirror' with bit 8 of the op word (AIMG_MIRROR; affine and elastic only).
//
// The elastic displacement field is made on the device from a Philox key, nothing dense is uploaded: with p = i * W + j,
//   u[f][i][j] = (philox4x32_10(counter (p, f, 0, 0), key)[0] + 0.5) / 2^31 - 1            f = 0 rows, 1 columns
//   g[f]       = correlate1d(correlate1d(u[f], w, 0, mode='constant', cval=0), w, 1, mode='constant', cval=0)
// with ONE symmetric kernel w per call (gaussian_filter1d's, radius <= 256).  Two launches before the stages, for the samples
// that carry an elastic stage: aimg_field_axis0_kernel generates u for a strip of AIMG_FS columns and all H rows straight into LDS
// (every Philox value is computed once and never stored to memory) and filters it along the rows into the fp64 scratch
// `field` [B, 2, H, W]; aimg_field_axis1_kernel takes one line of that into LDS and filters it in place.  A tap outside the image
// contributes 0 * w, which scipy adds and which leaves the sum as it is, so those taps are not read.
//
// Stages as in augment_ops.hip: one launch per stage, grid (tiles, B), all channels; stage s of sample b executes op word
// tab[b][1 + s] with the parameter row dp[b][s], reading the pools (s = 0, sample tab[b][0]) or work buffer s & 1 and writing
// work buffer (s + 1) & 1, so the result of S stages is in buffer S & 1.  fp32 in, fp64 arithmetic WITHOUT fused multiply-adds in
// scipy's operation order, fp32 out; labels uint8.  No atomics: two runs are bit-identical.
//
// cenet_augment_minmax: the per-sample (v - min) / ((max - min) + 1e-8f) of dataset_ham.py:113 in float32, two launches.
#include "common.h"
#include "../../include/cenet_hip.h"
#include "augment_ops.h"  // Philox, the tap order; fp contraction off from here on

#define AIMG_MAX_SIDE 1024
#define AIMG_MAX_FIELD_RADIUS 256
#define AIMG_MIRROR 256  // bit 8 of the op word
#define AIMG_FS 8        // columns per strip of the axis-0 field pass: 1024 x 8 doubles = 64 KB of LDS, two workgroups per CU;
                         // a wave reads 64 consecutive doubles per tap (both 32-lane halves of ds_read_b64 conflict-free) and
                         // stores 64-byte row segments

enum { AIMG_COPY = 0, AIMG_FLIP_UD, AIMG_FLIP_LR, AIMG_AFFINE, AIMG_BLUR, AIMG_BRIGHTNESS_CONTRAST, AIMG_ELASTIC, AIMG_COUNT };

// scipy map_coordinate(), NI_EXTEND_MIRROR, in its own arithmetic: a coordinate folded into [0, len).  A coordinate that lands in
// (len - 1, len) stays where it is (scipy folds from `>= len` on) and its taps are mirrored instead: for the order-1 image that is
// the same value to rounding, for the order-0 label it decides the tie at len - 1/2.
__device__ __forceinline__ double aimg_fold_mirror(double in, int len) {
  if (len <= 1) return 0.0;
  const long sz2 = 2 * (long)len - 2;
  if (in < 0.0) {
    in = (double)(sz2 * (long)(-in / (double)sz2)) + in;
    in = in <= (double)(1 - len) ? in + (double)sz2 : -in;
  } else if (in > (double)(len - 1)) {
    in -= (double)(sz2 * (long)(in / (double)sz2));
    if (in >= (double)len) in = (double)sz2 - in;
  }
  return in;
}

// scipy NI_GeometricTransform at (cy, cx) for C channels and the label.  mode='constant', cval=0: outside [0, len - 1] -> 0 for
// image and label; mode='mirror': the coordinate folded (above), every tap index mirrored.  The label reads floor(c + 0.5) (order
// 0), the image the four neighbours with weights (1 - f, f), rows outer, each tap value * wy * wx
__device__ __forceinline__ void aimg_sample(const float* __restrict__ src, const unsigned char* __restrict__ srl, int C, int H, int W,
                                            bool mirror, double cy, double cx, float* __restrict__ dst, long p, unsigned char& l) {
  const long HW = (long)H * W;
  if (mirror) {
    cy = aimg_fold_mirror(cy, H);
    cx = aimg_fold_mirror(cx, W);
  }
  const double ty = mirror ? (double)H : (double)(H - 1), tx = mirror ? (double)W : (double)(W - 1);
  if (!(cy >= 0.0 && cx >= 0.0 && (mirror ? cy < ty && cx < tx : cy <= ty && cx <= tx))) {  // (a NaN coordinate reads nothing either)
    for (int c = 0; c < C; ++c) dst[c * HW + p] = 0.f;
    l = 0;
    return;
  }
  l = srl[(long)aug_mirror((int)floor(cy + 0.5), H) * W + aug_mirror((int)floor(cx + 0.5), W)];
  const int y0 = (int)floor(cy), x0 = (int)floor(cx);  // (0 <= y0 <= H - 1, 0 <= x0 <= W - 1)
  const double fy = cy - (double)y0, fx = cx - (double)x0;
  const int y1 = aug_mirror(y0 + 1, H), x1 = aug_mirror(x0 + 1, W);  // (past the edge only with weight 0 when mode='constant')
  const double wy[2] = {1.0 - fy, fy}, wx[2] = {1.0 - fx, fx};
  for (int c = 0; c < C; ++c) {
    const float* r0 = src + c * HW + (long)y0 * W;
    const float* r1 = src + c * HW + (long)y1 * W;
    double t = 0.0;
    t += (double)r0[x0] * wy[0] * wx[0];
    t += (double)r0[x1] * wy[0] * wx[1];
    t += (double)r1[x0] * wy[1] * wx[0];
    t += (double)r1[x1] * wy[1] * wx[1];
    dst[c * HW + p] = (float)t;
  }
}

// the stage of sample b that is elastic, -1 without one
__device__ __forceinline__ int aimg_elastic_stage(const long* __restrict__ t, int S) {
  int at = -1;
  for (int s = 0; s < S; ++s)
    if ((int)(t[1 + s] & 255) == AIMG_ELASTIC) at = s;
  return at;
}

// grid (strips of AIMG_FS columns, 2, B): u[f] of the strip into LDS, axis-0 correlate1d(mode='constant') -> field[b][f]
__global__ __launch_bounds__(256) void aimg_field_axis0_kernel(const long* __restrict__ tab, const double* __restrict__ dp,
                                                              const double* __restrict__ w, int radius, double* __restrict__ field,
                                                              int H, int W, int S) {
  __shared__ double u[AIMG_MAX_SIDE * AIMG_FS];
  const int b = blockIdx.z, f = blockIdx.y, j0 = blockIdx.x * AIMG_FS;
  const int es = aimg_elastic_stage(tab + (long)b * (1 + S), S);
  if (es < 0) return;  // (the whole workgroup)
  const double* q = dp + ((long)b * S + es) * AOP_DP;
  const unsigned k0 = (unsigned)q[1], k1 = (unsigned)q[2];
  for (int e = threadIdx.x; e < H * AIMG_FS; e += 256) {
    const int i = e / AIMG_FS, j = j0 + e % AIMG_FS;
    double v = 0.0;
    if (j < W) {
      unsigned c[4] = {(unsigned)(i * W + j), (unsigned)f, 0u, 0u};
      aop_philox4x32_10(c, k0, k1);
      v = ((double)c[0] + 0.5) / 2147483648.0 - 1.0;
    }
    u[e] = v;
  }
  __syncthreads();
  if (radius > H - 1) radius = H - 1;  // (farther taps are outside for every row)
  double* g = field + ((long)b * 2 + f) * H * W;
  for (int e = threadIdx.x; e < H * AIMG_FS; e += 256) {
    const int i = e / AIMG_FS, j = j0 + e % AIMG_FS;
    if (j >= W) continue;
#define AIMG_AT0(k) (i + (k) >= 0 && i + (k) < H ? u[e + (k) * AIMG_FS] : 0.0)
    AOP_SYMMETRIC_TAPS(AIMG_AT0)
#undef AIMG_AT0
    g[(long)i * W + j] = acc;
  }
}

// grid (H, 2, B): one line of field[b][f] into LDS, axis-1 correlate1d(mode='constant'), in place
__global__ __launch_bounds__(256) void aimg_field_axis1_kernel(const long* __restrict__ tab, const double* __restrict__ w, int radius,
                                                              double* __restrict__ field, int H, int W, int S) {
  __shared__ double line[AIMG_MAX_SIDE];
  const int b = blockIdx.z, f = blockIdx.y, i = blockIdx.x;
  if (aimg_elastic_stage(tab + (long)b * (1 + S), S) < 0) return;
  double* g = field + (((long)b * 2 + f) * H + i) * W;
  for (int j = threadIdx.x; j < W; j += 256) line[j] = g[j];
  __syncthreads();
  if (radius > W - 1) radius = W - 1;
  for (int j = threadIdx.x; j < W; j += 256) {
#define AIMG_AT1(k) (j + (k) >= 0 && j + (k) < W ? line[j + (k)] : 0.0)
    AOP_SYMMETRIC_TAPS(AIMG_AT1)
#undef AIMG_AT1
    g[j] = acc;
  }
}

// grid (tiles, B); lab_f32: the label as float class ids too (the last stage, or null)
__global__ __launch_bounds__(256) void aimg_stage_kernel(const float* __restrict__ src_img, const unsigned char* __restrict__ src_lab,
                                                        int from_pool, const long* __restrict__ tab, const double* __restrict__ dp,
                                                        const double* __restrict__ field, float* __restrict__ dst_img,
                                                        unsigned char* __restrict__ dst_lab, float* __restrict__ lab_f32, int C, int H,
                                                        int W, int S, int s) {
  __shared__ double col[AOP_TH][AOP_TW + 2 * AOP_MAX_RADIUS];
  const int b = blockIdx.y;
  const long* t = tab + (long)b * (1 + S);
  const long word = t[1 + s];
  const int op = (int)(word & 255);
  const bool mirror = (word & AIMG_MIRROR) != 0;
  const long HW = (long)H * W;
  const long n = from_pool ? t[0] : (long)b;
  const float* src = src_img + n * C * HW;
  const unsigned char* srl = src_lab + n * HW;
  float* di = dst_img + (long)b * C * HW;
  unsigned char* dl = dst_lab + (long)b * HW;
  float* df = lab_f32 ? lab_f32 + (long)b * HW : nullptr;
  const double* q = dp + ((long)b * S + s) * AOP_DP;
  const int ty = threadIdx.x / AOP_TW, tx = threadIdx.x % AOP_TW;
  const int tiles_x = (W + AOP_TW - 1) / AOP_TW, tiles = ((H + AOP_TH - 1) / AOP_TH) * tiles_x;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (the trip count is the same for every thread of the block)
    const int i0 = (tile / tiles_x) * AOP_TH, j0 = (tile % tiles_x) * AOP_TW;
    const int i = i0 + ty, j = j0 + tx;
    const bool live = i < H && j < W;
    const long p = (long)i * W + j;
    if (op == AIMG_BLUR) {
      const int radius = (int)q[0];
      const double* w = q + 1;  // w[0] the centre weight, w[k] = the weight of both taps at distance k
      const int cols = AOP_TW + 2 * radius;
      for (int c = 0; c < C; ++c) {
        const float* sc = src + c * HW;
        for (int e = threadIdx.x; e < AOP_TH * cols; e += 256) {  // axis 0, for the tile's columns and `radius` more on either side
          const int ey = e / cols, ex = e - ey * cols;
          const int r = i0 + ey;
          double v = 0.0;
          if (r < H) {
            const float* a = sc + aug_mirror(j0 + ex - radius, W);
#define AIMG_AT0(k) (double)a[(long)aug_mirror(r + (k), H) * W]
            AOP_SYMMETRIC_TAPS(AIMG_AT0)
#undef AIMG_AT0
            v = acc;
          }
          col[ey][ex] = v;
        }
        __syncthreads();
        if (live) {  // axis 1, from the fp64 intermediate
          const double* a = &col[ty][tx + radius];
#define AIMG_AT1(k) a[(k)]
          AOP_SYMMETRIC_TAPS(AIMG_AT1)
#undef AIMG_AT1
          di[c * HW + p] = (float)acc;
        }
        __syncthreads();  // the next channel / tile overwrites col
      }
      if (live) {
        dl[p] = srl[p];
        if (df) df[p] = (float)srl[p];
      }
      continue;
    }
    if (!live) continue;
    unsigned char l;
    if (op == AIMG_AFFINE || op == AIMG_ELASTIC) {
      double cy, cx;
      if (op == AIMG_AFFINE) {  // scipy accumulates every coordinate component over the output axes, then adds the shift
        cy = 0.0, cx = 0.0;
        cy += (double)i * q[0];
        cy += (double)j * q[1];
        cy += q[4];
        cx += (double)i * q[2];
        cx += (double)j * q[3];
        cx += q[5];
      } else {
        const double* g = field + (long)b * 2 * HW;
        cy = (double)i + q[0] * g[p];
        cx = (double)j + q[0] * g[HW + p];
      }
      aimg_sample(src, srl, C, H, W, mirror, cy, cx, di, p, l);
    } else {
      const long sp = op == AIMG_FLIP_UD ? (long)(H - 1 - i) * W + j : op == AIMG_FLIP_LR ? (long)i * W + (W - 1 - j) : p;
      l = srl[sp];
      for (int c = 0; c < C; ++c) {
        float v = src[c * HW + sp];
        if (op == AIMG_BRIGHTNESS_CONTRAST) {
          double a = q[0] * (double)v;
          a = a + q[1];
          a = a < q[2] ? q[2] : a;  // np.clip = minimum(maximum(a, lo), hi)
          a = a > q[3] ? q[3] : a;
          v = (float)a;
        }
        di[c * HW + p] = v;
      }
    }
    dl[p] = l;
    if (df) df[p] = (float)l;
  }
}

// tab_host / dp_host / fw_host: the tables and the field kernel as the host made them, read here before anything is launched;
// tab / dp / fw: their device copies
extern "C" int cenet_augment_image_ops(const float* pool_img, const unsigned char* pool_lab, const long* tab_host, const double* dp_host,
                                       const long* tab, const double* dp, const double* fw_host, const double* fw, int field_radius,
                                       double* field, float* work_img0, unsigned char* work_lab0, float* work_img1,
                                       unsigned char* work_lab1, float* out_lab, int N, int C, int H, int W, int B, int S,
                                       hipStream_t stream) {
  if (!pool_img || !pool_lab || !tab_host || !dp_host || !tab || !dp || !work_img0 || !work_lab0 || !work_img1 || !work_lab1)
    return CENET_EINVAL;
  if (B <= 0 || B > 65535 || N <= 0 || S < 1 || S > AOP_MAX_STAGES || C < 1 || C > 4) return CENET_EINVAL;
  if (H < 1 || H > AIMG_MAX_SIDE || W < 1 || W > AIMG_MAX_SIDE) return CENET_EINVAL;
  if (work_img0 == work_img1 || work_lab0 == work_lab1) return CENET_EINVAL;
  bool any_elastic = false;
  for (int b = 0; b < B; ++b) {
    const long* t = tab_host + (long)b * (1 + S);
    if (t[0] < 0 || t[0] >= N) return CENET_EINVAL;
    int elastic = 0;
    for (int s = 0; s < S; ++s) {
      const long word = t[1 + s];
      const long op = word & 255;
      const double* q = dp_host + ((long)b * S + s) * AOP_DP;
      if (word < 0 || op >= AIMG_COUNT || (word & ~(long)(255 | AIMG_MIRROR)) != 0) return CENET_EINVAL;
      if ((word & AIMG_MIRROR) && op != AIMG_AFFINE && op != AIMG_ELASTIC) return CENET_EINVAL;
      if (op == AIMG_BLUR && !(q[0] >= 0.0 && q[0] <= (double)AOP_MAX_RADIUS && q[0] == (double)(int)q[0])) return CENET_EINVAL;
      if (op == AIMG_BRIGHTNESS_CONTRAST && !(q[2] <= q[3])) return CENET_EINVAL;
      if (op == AIMG_ELASTIC) {
        if (++elastic > 1) return CENET_EINVAL;
        if (!(q[1] >= 0.0 && q[1] < 4294967296.0 && q[2] >= 0.0 && q[2] < 4294967296.0)) return CENET_EINVAL;
        if (q[1] != (double)(unsigned)q[1] || q[2] != (double)(unsigned)q[2]) return CENET_EINVAL;
      }
    }
    any_elastic = any_elastic || elastic;
  }
  if (any_elastic && (!fw_host || !fw || !field || field_radius < 0 || field_radius > AIMG_MAX_FIELD_RADIUS)) return CENET_EINVAL;
  if (any_elastic) {
    CENET_LAUNCH(aimg_field_axis0_kernel, dim3(cdiv(W, AIMG_FS), 2, B), dim3(256), stream, tab, dp, fw, field_radius, field, H, W, S);
    CENET_LAUNCH(aimg_field_axis1_kernel, dim3(H, 2, B), dim3(256), stream, tab, fw, field_radius, field, H, W, S);
  }
  float* wi[2] = {work_img0, work_img1};
  unsigned char* wl[2] = {work_lab0, work_lab1};
  const int tiles = cdiv(H, AOP_TH) * cdiv(W, AOP_TW);
  for (int s = 0; s < S; ++s) {
    const float* si = s == 0 ? pool_img : wi[s & 1];
    const unsigned char* sl = s == 0 ? pool_lab : wl[s & 1];
    CENET_LAUNCH(aimg_stage_kernel, dim3(tiles, B), dim3(256), stream, si, sl, (int)(s == 0), tab, dp, (const double*)field,
                 wi[(s + 1) & 1], wl[(s + 1) & 1], s == S - 1 ? out_lab : (float*)nullptr, C, H, W, S, s);
  }
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// ---- per-sample min-max normalisation -------------------------------------------------------------------------------------------
#define AMM_MAX_PARTS 128  // workgroups per sample
#define AMM_PER_BLOCK 4096 // elements a workgroup takes at least (16 per thread)

__host__ __device__ __forceinline__ int amm_parts(long n) {
  const long g = (n + AMM_PER_BLOCK - 1) / AMM_PER_BLOCK;
  return (int)(g < AMM_MAX_PARTS ? g : AMM_MAX_PARTS);
}

// the minimum / maximum of 256 threads' values, in every thread
__device__ __forceinline__ void amm_block_minmax(float& mn, float& mx, float (*red)[256]) {
  red[0][threadIdx.x] = mn;
  red[1][threadIdx.x] = mx;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      red[0][threadIdx.x] = fminf(red[0][threadIdx.x], red[0][threadIdx.x + h]);
      red[1][threadIdx.x] = fmaxf(red[1][threadIdx.x], red[1][threadIdx.x + h]);
    }
    __syncthreads();
  }
  mn = red[0][0];
  mx = red[1][0];
  __syncthreads();
}

// grid (G, B): part[b][0][g], part[b][1][g] = min, max of workgroup g's share of sample b
__global__ __launch_bounds__(256) void amm_partial_kernel(const float* __restrict__ x, float* __restrict__ part, long n, int G) {
  __shared__ float red[2][256];
  const float* xb = x + (long)blockIdx.y * n;
  float mn = xb[0], mx = xb[0];
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)G * 256) {
    const float v = xb[p];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  amm_block_minmax(mn, mx, red);
  if (threadIdx.x == 0) {
    part[((long)blockIdx.y * 2 + 0) * AMM_MAX_PARTS + blockIdx.x] = mn;
    part[((long)blockIdx.y * 2 + 1) * AMM_MAX_PARTS + blockIdx.x] = mx;
  }
}

// grid (G, B): combine the sample's G partials, then y = (x - mn) / ((mx - mn) + 1e-8f) on the workgroup's share
__global__ __launch_bounds__(256) void amm_apply_kernel(const float* __restrict__ x, const float* __restrict__ part, float* __restrict__ y,
                                                       long n, int G) {
  __shared__ float red[2][256];
  const float* pb = part + (long)blockIdx.y * 2 * AMM_MAX_PARTS;
  float mn = pb[0], mx = pb[AMM_MAX_PARTS];
  if ((int)threadIdx.x < G) {
    mn = pb[threadIdx.x];
    mx = pb[AMM_MAX_PARTS + threadIdx.x];
  }
  amm_block_minmax(mn, mx, red);
  const float d = (mx - mn) + 1e-8f;
  const float* xb = x + (long)blockIdx.y * n;
  float* yb = y + (long)blockIdx.y * n;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)G * 256) yb[p] = (xb[p] - mn) / d;
}

extern "C" int cenet_augment_minmax(const float* x, float* y, float* part, int B, long n, hipStream_t stream) {
  if (!x || !y || !part || B <= 0 || B > 65535 || n <= 0) return CENET_EINVAL;
  const int G = amm_parts(n);
  CENET_LAUNCH(amm_partial_kernel, dim3(G, B), dim3(256), stream, x, part, n, G);
  CENET_LAUNCH(amm_apply_kernel, dim3(G, B), dim3(256), stream, (const float*)x, (const float*)part, y, n, G);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
