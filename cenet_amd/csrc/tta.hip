// tta.hip — flip / rotate test-time augmentation of the device inference loop (evaluate.predict_volume(tta=...), tta_predict).  The
// recipe is the reference's tta_model (utils/utils.py:146-168: identity, horizontal flip, vertical flip), widened to the dihedral
// group D4 and averaging class probabilities instead of masks.
//
// A view is an element g of D4 as a bit field: bit 0 flip along W, bit 1 flip along H, bit 2 transpose H and W; forward
//   v = x;  if (g & 4) v = v^T;  if (g & 2) v = flip_H(v);  if (g & 1) v = flip_W(v)
// so view pixel (y, x) holds source pixel (a, b) with y' = g & 2 ? PH - 1 - y : y, x' = g & 1 ? PW - 1 - x : x and
// (a, b) = g & 4 ? (x', y') : (y', x').  The flips are involutions, hence source pixel (a, b) sits at view pixel
// (fy(a), fx(b)), or (fy(b), fx(a)) under a transpose.  A view set is an 8-bit mask, the views are taken in ascending code order
// (slot t = the t-th set bit), so the order of the float additions is fixed and two runs agree to the bit.  Views with bit 2 need
// PH == PW.
//
//   cenet_tta_views_f32                 src [n, C, PH, PW] -> out [T, n, C, PH, PW], all views in one launch.  A workgroup loads a
//                                       32 x 32 source tile into LDS once (rows of 33 floats: the transposed read walks a column
//                                       with stride 33, one bank per lane) and writes it into every view: lanes run along the
//                                       view's x in every case, so loads and stores are whole 128-byte rows.
//   cenet_tta_argmax_resize_counts_*    logits [T, n, K, PH, PW] -> pred / conf [n, H, W] and the overlap counts.  One thread per
//                                       OUTPUT voxel finds the order-0 zoom source pixel exactly as argmax_resize_counts_kernel
//                                       (volresize.hip) does, then per view reads that pixel's K logits at the view's position,
//                                       takes the max-subtracted fp32 softmax and adds it into K register accumulators; pred is
//                                       the first maximum of the sums under `>`, conf the winner's mean probability.  No
//                                       probability volume and no class map at [PH, PW] is written.  A workgroup owns a 32 x 32
//                                       output tile (lanes along x): the straight views read rows, the transposed ones columns
//                                       whose 128-byte lines the tile's other rows use up from the CU's cache.
// Non-finite logits are not special-cased: a NaN logit makes that pixel's sums NaN, and a NaN sum never wins under `>`, so
// such a voxel falls to the first class whose sum is a number (class 0 if none) — as argmax_resize_counts_kernel ignores them.
#include "common.h"
#include "../../include/cenet_hip.h"

// no fused multiply-adds: floor(index * zoom + 0.5) must round as scipy's (and volresize.hip's) two operations do
#pragma clang fp contract(off)

#define TTA_MAXK 16  // classes: VOL_MAXK of volresize.hip (register accumulators, counts in LDS)
#define TTA_TILE 32

static inline int tta_views_of(int view_mask) {
  int t = 0;
  for (int g = 0; g < 8; ++g) t += (view_mask >> g) & 1;
  return t;
}
// a mask in 1..255, and square patches for the transposed views
static inline bool tta_mask_ok(int view_mask, int PH, int PW) {
  return view_mask >= 1 && view_mask <= 255 && (!(view_mask & 0xF0) || PH == PW);
}

// grid-stride over (plane, tile); 256 threads = 32 lanes along x times 8 rows, four row groups per tile
__global__ __launch_bounds__(256) void tta_views_kernel(const float* __restrict__ src, float* __restrict__ out, long planes, int PH,
                                                       int PW, int tiles_x, int tiles_y, int view_mask, long ntiles) {
  __shared__ float tile[TTA_TILE][TTA_TILE + 1];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const long PHW = (long)PH * PW, tpp = (long)tiles_x * tiles_y;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long plane = t / tpp;
    const int tt = (int)(t - plane * tpp);
    const int ty0 = (tt / tiles_x) * TTA_TILE, tx0 = (tt % tiles_x) * TTA_TILE;
    const float* sp = src + plane * PHW;
    __syncthreads();  // the previous tile has been written out
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = ly + 8 * i;
      if (ty0 + r < PH && tx0 + lx < PW) tile[r][lx] = sp[(long)(ty0 + r) * PW + tx0 + lx];
    }
    __syncthreads();
    float* op = out + plane * PHW;
    for (int g = 0; g < 8; ++g) {
      if (!((view_mask >> g) & 1)) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = ly + 8 * i;
        // straight: lane = source column; transposed: lane = source row (the view's x runs along it)
        const int a = (g & 4) ? ty0 + lx : ty0 + r, b = (g & 4) ? tx0 + r : tx0 + lx;
        if (a < PH && b < PW) {
          const int p = (g & 4) ? b : a, q = (g & 4) ? a : b;  // the view pixel before the flips
          const int y = (g & 2) ? PH - 1 - p : p, x = (g & 1) ? PW - 1 - q : q;
          op[(long)y * PW + x] = (g & 4) ? tile[lx][r] : tile[r][lx];
        }
      }
      op += planes * PHW;
    }
  }
}

extern "C" int cenet_tta_views_f32(const float* src, float* out, int n, int C, int PH, int PW, int view_mask, hipStream_t stream) {
  if (!src || !out) return CENET_EINVAL;
  if (n <= 0 || C <= 0 || PH < 1 || PW < 1 || !tta_mask_ok(view_mask, PH, PW)) return CENET_EINVAL;
  if ((long)PH * PW > 0x7FFFFFFFL) return CENET_EINVAL;
  const int tiles_x = cdiv(PW, TTA_TILE), tiles_y = cdiv(PH, TTA_TILE);
  const long planes = (long)n * C, ntiles = planes * tiles_x * tiles_y;
  const long blocks = ntiles < 8192 ? ntiles : 8192;
  CENET_LAUNCH(tta_views_kernel, dim3((unsigned)blocks), dim3(256), stream, src, out, planes, PH, PW, tiles_x, tiles_y, view_mask,
               ntiles);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// The zoom rule is argmax_resize_counts_kernel's, to the letter: coordinate c = index * ((PH - 1) / (H - 1)) in fp64, c > PH - 1 -> class
// 0 (and conf 0), otherwise the source pixel floor(c + 0.5).  All loops over the classes have the fixed bound TTA_MAXK, so v[] and
// acc[] are registers.
template <typename T>
__global__ __launch_bounds__(256) void tta_argmax_resize_counts_kernel(const T* __restrict__ logits, const float* __restrict__ labels,
                                                                      float* __restrict__ pred, float* __restrict__ conf,
                                                                      unsigned* __restrict__ counts, int n, int K, int PH, int PW,
                                                                      int H, int W, double zy, double zx, int view_mask, float inv_t,
                                                                      int tiles_x, int tiles_y, long ntiles) {
  __shared__ unsigned sc[(TTA_MAXK + 1) * 3];
  for (int i = threadIdx.x; i < (K + 1) * 3; i += 256) sc[i] = 0u;
  __syncthreads();
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const long HW = (long)H * W, PHW = (long)PH * PW, tpp = (long)tiles_x * tiles_y;
  const long vstride = (long)n * K * PHW;  // one view's logit stack
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long b = t / tpp;
    const int tt = (int)(t - b * tpp);
    const int x = (tt % tiles_x) * TTA_TILE + lx, ty0 = (tt / tiles_x) * TTA_TILE;
    if (x >= W) continue;
    const double cx = (double)x * zx;
    for (int i = 0; i < 4; ++i) {
      const int y = ty0 + ly + 8 * i;
      if (y >= H) break;
      const double cy = (double)y * zy;
      int arg = 0;
      float cf = 0.f;
      if (!(cy > (double)(PH - 1) || cx > (double)(PW - 1))) {
        const int sy = (int)floor(cy + 0.5), sx = (int)floor(cx + 0.5);
        float acc[TTA_MAXK];
#pragma unroll
        for (int c = 0; c < TTA_MAXK; ++c) acc[c] = 0.f;
        const T* lb = logits + b * (long)K * PHW;
        for (int g = 0; g < 8; ++g) {
          if (!((view_mask >> g) & 1)) continue;
          const int p = (g & 4) ? sx : sy, q = (g & 4) ? sy : sx;
          const int yv = (g & 2) ? PH - 1 - p : p, xv = (g & 1) ? PW - 1 - q : q;
          const T* lp = lb + (long)yv * PW + xv;
          lb += vstride;
          float v[TTA_MAXK];
          float m = ldf(lp);
          v[0] = m;
#pragma unroll
          for (int c = 1; c < TTA_MAXK; ++c)
            if (c < K) {
              v[c] = ldf(lp + (long)c * PHW);
              m = v[c] > m ? v[c] : m;
            }
          float s = 0.f;
#pragma unroll
          for (int c = 0; c < TTA_MAXK; ++c)
            if (c < K) {
              v[c] = expf(v[c] - m);
              s += v[c];
            }
          const float inv = 1.f / s;
#pragma unroll
          for (int c = 0; c < TTA_MAXK; ++c)
            if (c < K) acc[c] += v[c] * inv;
        }
        float best = acc[0];
#pragma unroll
        for (int c = 1; c < TTA_MAXK; ++c)
          if (c < K && acc[c] > best) {
            best = acc[c];
            arg = c;
          }
        cf = best * inv_t;
      }
      const long e = b * HW + (long)y * W + x;
      pred[e] = (float)arg;
      if (conf) conf[e] = cf;
      if (labels) {
        const int tl = (int)labels[e];
        atomicAdd(&sc[arg * 3 + 1], 1u);
        if (tl >= 0 && tl < K) atomicAdd(&sc[tl * 3 + 2], 1u);
        if (tl == arg) atomicAdd(&sc[arg * 3], 1u);
        if (arg > 0) atomicAdd(&sc[K * 3 + 1], 1u);
        if (tl > 0) atomicAdd(&sc[K * 3 + 2], 1u);
        if (arg > 0 && tl > 0) atomicAdd(&sc[K * 3], 1u);
      }
    }
  }
  __syncthreads();
  if (labels)
    for (int i = threadIdx.x; i < (K + 1) * 3; i += 256)
      if (sc[i]) atomicAdd(&counts[i], sc[i]);
}

template <typename T>
static int tta_argmax_resize_counts_impl(const T* logits, const float* labels, float* pred, float* conf, unsigned* counts, int n, int K,
                                         int PH, int PW, int H, int W, int view_mask, hipStream_t stream) {
  if (!logits || !pred || (labels && !counts)) return CENET_EINVAL;
  if (n <= 0 || K <= 0 || K > TTA_MAXK || H < 2 || W < 2 || PH < 2 || PW < 2) return CENET_EINVAL;
  if (!tta_mask_ok(view_mask, PH, PW)) return CENET_EINVAL;
  if ((long)H * W > 0x7FFFFFFFL || (long)PH * PW > 0x7FFFFFFFL) return CENET_EINVAL;
  if (labels && cenet_zero_async((float*)counts, (K + 1) * 3L, stream) != CENET_OK) return CENET_EINVAL;
  const int tiles_x = cdiv(W, TTA_TILE), tiles_y = cdiv(H, TTA_TILE);
  const long ntiles = (long)n * tiles_x * tiles_y;
  const long blocks = ntiles < 4096 ? ntiles : 4096;
  const double zy = (double)(PH - 1) / (double)(H - 1), zx = (double)(PW - 1) / (double)(W - 1);
  CENET_LAUNCH((tta_argmax_resize_counts_kernel<T>), dim3((unsigned)blocks), dim3(256), stream, logits, labels, pred, conf, counts, n,
               K, PH, PW, H, W, zy, zx, view_mask, 1.0f / (float)tta_views_of(view_mask), tiles_x, tiles_y, ntiles);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(tta_argmax_resize_counts, (const T* logits, const float* labels, float* pred, float* conf, unsigned* counts, int n, int K,
                                      int PH, int PW, int H, int W, int view_mask, hipStream_t stream),
           (logits, labels, pred, conf, counts, n, K, PH, PW, H, W, view_mask, stream))
