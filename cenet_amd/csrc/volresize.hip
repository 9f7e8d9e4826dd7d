// volresize.hip — the two resizes of the reference's test-time volume inference on the device (src/utils/metrics_eval.py:37-84,
// src/utils/utils_synapse.py:49-97): every slice of a test volume is resized to the network's input size with
// scipy.ndimage.zoom(order=3), classified, and the class map resized back with zoom(order=0).
//
//   cenet_vol_resize_cubic        n slices [H, W] fp32 -> [n, 1, PH, PW] fp32, optionally normalised
//     stage 1  vol_stage          fp32 -> fp64 copy of the chunk
//     stage 2  vol_prefilter      scipy's cubic B-spline prefilter (mirror boundary), axis 0 then axis 1, in place
//     stage 3  vol_zoom           zoom(order=3): output index o samples the input at o * ((H - 1) / (PH - 1)); a coordinate above
//                                 H - 1 (by one ulp is enough) gives cval = 0; taps mirror as in NI_ZoomShift
//   cenet_argmax_resize_counts    logits [n, K, PH, PW] -> class ids [n, H, W] (first maximum over K of the source pixel that
//                                 zoom(order=0) picks) and, with labels, the overlap counts of cenet_argmax_counts at [H, W].  The
//                                 class map at the network's resolution is never written.
//
// The spline arithmetic is augment.hip's (spline3.h): fp64, scipy's operation order, no fused multiply-adds, so the resized
// slices agree with scipy to the last float32 bit in practice (tests/test_volresize.py: 1e-6 and >= 99.9 % identical) and the
// class maps exactly (integer ids, scipy's fp64 coordinate arithmetic).
#include "common.h"
#include "../../include/cenet_hip.h"
#include "spline3.h"  // aug_prefilter_line, aug_cubic_at; fp contraction off from here on

#define VOL_MAXK 16  // classes (the counts live in LDS), as LOSS_MAXK of loss_optim.hip

__global__ __launch_bounds__(256) void vol_stage_kernel(const float* __restrict__ src, double* __restrict__ stage, long total) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) stage[e] = (double)src[e];
}

// AXIS 0: thread = one column (lines run down the rows, neighbouring threads touch neighbouring addresses); AXIS 1: thread = one
// row.  grid (chunks of 64 lines, n)
template <int AXIS>
__global__ __launch_bounds__(64) void vol_prefilter_kernel(double* __restrict__ stage, int H, int W, double zn) {
  double* c = stage + (long)blockIdx.y * H * W;
  const int line = blockIdx.x * 64 + threadIdx.x;
  if (AXIS == 0) {
    if (line < W) aug_prefilter_line(c + line, H, W, zn);
  } else {
    if (line < H) aug_prefilter_line(c + (long)line * W, W, 1, zn);
  }
}

// grid (chunks, n).  norm: out = (float(v) - mean) / std in fp32, in that order — what `(inp - 0.5) / 0.5` computes on the host after
// scipy has rounded its result to float32 (utils_synapse.py Normalize)
__global__ __launch_bounds__(256) void vol_zoom_kernel(const double* __restrict__ stage, float* __restrict__ out, int H, int W,
                                                      int PH, int PW, double zy, double zx, int norm, float mean, float std) {
  const double* c = stage + (long)blockIdx.y * H * W;
  float* o = out + (long)blockIdx.y * PH * PW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < PH * PW; p += gridDim.x * 256) {
    const int oy = p / PW, ox = p - oy * PW;
    const double cy = (double)oy * zy, cx = (double)ox * zx;
    // scipy map_coordinate(mode='constant'): outside [0, len - 1] -> cval = 0 (see aug_zoom_kernel)
    float v = 0.f;
    if (!(cy > (double)(H - 1) || cx > (double)(W - 1))) v = (float)aug_cubic_at(c, H, W, cy, cx);
    if (norm) v = (v - mean) / std;
    o[p] = v;
  }
}

extern "C" int cenet_vol_resize_cubic(const float* src, double* stage, float* out, int n, int H, int W, int PH, int PW,
                                      double zn_h, double zn_w, int normalize, float mean, float std, hipStream_t stream) {
  if (!src || !stage || !out) return CENET_EINVAL;
  if (n <= 0 || H < 2 || W < 2 || PH < 2 || PW < 2 || (normalize && std == 0.f)) return CENET_EINVAL;
  if ((long)H * W > 0x7FFFFFFFL || (long)PH * PW > 0x7FFFFFFFL || n > 65535) return CENET_EINVAL;
  const long total = (long)n * H * W;
  long blocks = (total + 1023) / 1024;
  if (blocks > 4096) blocks = 4096;
  CENET_LAUNCH(vol_stage_kernel, dim3((unsigned)blocks), dim3(256), stream, src, stage, total);
  CENET_LAUNCH(vol_prefilter_kernel<0>, dim3(cdiv(W, 64), n), dim3(64), stream, stage, H, W, zn_h);
  CENET_LAUNCH(vol_prefilter_kernel<1>, dim3(cdiv(H, 64), n), dim3(64), stream, stage, H, W, zn_w);
  // scipy zoom, grid_mode=False: input coordinate = output index * (in - 1) / (out - 1)
  const double zy = (double)(H - 1) / (double)(PH - 1), zx = (double)(W - 1) / (double)(PW - 1);
  CENET_LAUNCH(vol_zoom_kernel, dim3(cdiv((long)PH * PW, 256 * 4), n), dim3(256), stream, (const double*)stage, out, H, W, PH, PW, zy,
               zx, normalize, mean, std);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// pred[b, y, x] = argmax_c logits[b, c, sy, sx] with (sy, sx) the source pixel of scipy's zoom(order=0) from [PH, PW] to [H, W]:
// coordinate c = index * ((PH - 1) / (H - 1)) in fp64, outside [0, PH - 1] -> 0, otherwise floor(c + 0.5).  First maximum on ties.
// counts as in argmax_counts_kernel (loss_optim.hip), at the volume's resolution.
template <typename T>
__global__ __launch_bounds__(256) void argmax_resize_counts_kernel(const T* __restrict__ logits, const float* __restrict__ labels,
                                                                  float* __restrict__ pred, unsigned* __restrict__ counts, int K,
                                                                  int PH, int PW, int H, int W, double zy, double zx, long npix) {
  __shared__ unsigned sc[(VOL_MAXK + 1) * 3];
  for (int i = threadIdx.x; i < (K + 1) * 3; i += 256) sc[i] = 0u;
  __syncthreads();
  const long HW = (long)H * W, PHW = (long)PH * PW;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < npix; e += (long)gridDim.x * 256) {
    const long b = e / HW;
    const int p = (int)(e - b * HW);
    const int y = p / W, x = p - y * W;
    const double cy = (double)y * zy, cx = (double)x * zx;
    int arg = 0;
    if (!(cy > (double)(PH - 1) || cx > (double)(PW - 1))) {
      const int sy = (int)floor(cy + 0.5), sx = (int)floor(cx + 0.5);
      const T* lp = logits + b * (long)K * PHW + (long)sy * PW + sx;
      float best = ldf(lp);
      for (int c = 1; c < K; ++c) {
        const float v = ldf(lp + (long)c * PHW);
        if (v > best) {
          best = v;
          arg = c;
        }
      }
    }
    pred[e] = (float)arg;
    if (labels) {
      const int t = (int)labels[e];
      atomicAdd(&sc[arg * 3 + 1], 1u);
      if (t >= 0 && t < K) atomicAdd(&sc[t * 3 + 2], 1u);
      if (t == arg) atomicAdd(&sc[arg * 3], 1u);
      if (arg > 0) atomicAdd(&sc[K * 3 + 1], 1u);
      if (t > 0) atomicAdd(&sc[K * 3 + 2], 1u);
      if (arg > 0 && t > 0) atomicAdd(&sc[K * 3], 1u);
    }
  }
  __syncthreads();
  if (labels)
    for (int i = threadIdx.x; i < (K + 1) * 3; i += 256)
      if (sc[i]) atomicAdd(&counts[i], sc[i]);
}

template <typename T>
static int argmax_resize_counts_impl(const T* logits, const float* labels, float* pred, unsigned* counts, int n, int K, int PH,
                                     int PW, int H, int W, hipStream_t stream) {
  if (!logits || !pred || (labels && !counts)) return CENET_EINVAL;
  if (n <= 0 || K <= 0 || K > VOL_MAXK || H < 2 || W < 2 || PH < 2 || PW < 2) return CENET_EINVAL;
  if ((long)H * W > 0x7FFFFFFFL || (long)PH * PW > 0x7FFFFFFFL) return CENET_EINVAL;
  const long npix = (long)n * H * W;
  if (labels && cenet_zero_async((float*)counts, (K + 1) * 3L, stream) != CENET_OK) return CENET_EINVAL;
  long blocks = (npix + 2047) / 2048;
  if (blocks > 2048) blocks = 2048;
  const double zy = (double)(PH - 1) / (double)(H - 1), zx = (double)(PW - 1) / (double)(W - 1);
  CENET_LAUNCH((argmax_resize_counts_kernel<T>), dim3((unsigned)blocks), dim3(256), stream, logits, labels, pred, counts, K, PH, PW, H,
               W, zy, zx, npix);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(argmax_resize_counts, (const T* logits, const float* labels, float* pred, unsigned* counts, int n, int K, int PH, int PW,
                                  int H, int W, hipStream_t stream), (logits, labels, pred, counts, n, K, PH, PW, H, W, stream))
