// sliding_window.hip — sliding-window inference at the image's own resolution (evaluate.sliding_window_predict,
// evaluate.predict_volume(window_overlap=...)): the network runs on overlapping windows of its own input size, the windows' class
// probabilities are blended with a separable importance map (nnU-Net's window grid, MONAI's Gaussian map) and the argmax is taken.
// Nothing is resized.
//
// Window (b, iy, ix) of a slice is entry (b * nwy + iy) * nwx + ix of the network's batch and holds source pixel
// (oy[iy] + y, ox[ix] + x) at (y, x); an origin may be negative (a slice smaller than the window is centred in it).  The two origin
// tables are checked on the host (ascending, first <= 0, no gap, last + P >= L, at most 32 per axis: every output pixel is then
// covered by a window) and travel to the kernels BY VALUE in the kernel arguments: the values the kernels index with are the
// values that were checked, no upload and no synchronisation is needed, and a wave reads them through the scalar cache.
//
//   cenet_sw_windows_f32          src [n, C, H, W] -> out [n * nwy * nwx, C, PH, PW], all windows in one launch.  A wave owns one
//                                 window row (lanes along x: loads and stores are whole row segments); outside the slice it
//                                 stores pad_value as given, inside a bit copy or (x - mean) / std with a true division.
//   cenet_sw_merge_counts_*       logits [T, n * nwy * nwx, K, PH, PW] -> pred / conf [n, H, W] and the overlap counts, in the
//                                 gather form: one thread per OUTPUT pixel visits the windows that cover it in ascending (iy, ix)
//                                 and, inside a window, the views of view_mask in ascending code (tta.hip's D4 codes), reads
//                                 the pixel's K logits at its position in that view, takes tta.hip's max-subtracted fp32 softmax
//                                 and adds w * softmax into K register accumulators, w = wy[y - oy] * wx[x - ox].  pred is the
//                                 first maximum of the sums under `>`, conf = sum[pred] / (wsum * T).  No float atomic decides a
//                                 value, the order of the additions is fixed (two runs agree to the bit), and no probability
//                                 volume, weight-sum volume or per-window class map is written.  A workgroup owns a 32 x 32
//                                 output tile; the window range that can touch the tile is found once per tile from the scalar
//                                 tables, so the loops over the windows have wave-uniform bounds and only the tile's border
//                                 pixels mask a window out.  A window's padding maps onto no output pixel and is never read.
// Non-finite logits follow tta.hip's rule: a NaN sum never wins under `>`.
#include "common.h"
#include "../../include/cenet_hip.h"

// no fused multiply-adds: w * p and the running sums round as the two operations of the float32 restatement do
#pragma clang fp contract(off)

#define SW_MAXK 16  // classes: TTA_MAXK of tta.hip (register accumulators, counts in LDS)
#define SW_TILE 32
#define SW_MAXW 32  // windows per axis

struct SwTab {
  int oy[SW_MAXW];
  int ox[SW_MAXW];
};

// strictly ascending, first <= 0, consecutive windows leave no gap, the last one reaches the end
static bool sw_table_ok(const int* o, int nw, int P, int L) {
  if (!o || nw < 1 || nw > SW_MAXW) return false;
  if (o[0] > 0 || o[0] <= -P) return false;
  for (int i = 0; i + 1 < nw; ++i)
    if (o[i + 1] <= o[i] || (long)o[i + 1] > (long)o[i] + P) return false;
  return (long)o[nw - 1] + P >= L && o[nw - 1] < L;
}

static bool sw_tables(SwTab& tab, const int* oy_host, const int* ox_host, int nwy, int nwx, int PH, int PW, int H, int W) {
  if (!sw_table_ok(oy_host, nwy, PH, H) || !sw_table_ok(ox_host, nwx, PW, W)) return false;
  for (int i = 0; i < SW_MAXW; ++i) {
    tab.oy[i] = oy_host[i < nwy ? i : nwy - 1];
    tab.ox[i] = ox_host[i < nwx ? i : nwx - 1];
  }
  return true;
}

// one wave per window row, four rows per workgroup, grid-stride over the rows of all windows and channels
__global__ __launch_bounds__(256) void sw_windows_kernel(const float* __restrict__ src, float* __restrict__ out, SwTab tab, int C, int H,
                                                        int W, int PH, int PW, int nwy, int nwx, int normalize, float mean, float std,
                                                        float pad, long nrows) {
  const int lane = threadIdx.x & 63;
#ifdef CENET_HOSTSIM_BUILD
  const int wave = threadIdx.x >> 6;
#else
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the row's indices and table reads are scalar
#endif
  for (long r = (long)blockIdx.x * 4 + wave; r < nrows; r += (long)gridDim.x * 4) {
    const int y = (int)(r % PH);
    long q = r / PH;
    const int c = (int)(q % C);
    q /= C;
    const int ix = (int)(q % nwx);
    q /= nwx;
    const int iy = (int)(q % nwy);
    const long b = q / nwy;
    const int sy = tab.oy[iy] + y, x0 = tab.ox[ix];
    const bool row_in = sy >= 0 && sy < H;
    const float* sp = src + ((b * C + c) * H + (row_in ? sy : 0)) * (long)W;
    float* op = out + r * PW;
    for (int x = lane; x < PW; x += 64) {
      const int sx = x0 + x;
      float v = pad;
      if (row_in && sx >= 0 && sx < W) {
        v = sp[sx];
        if (normalize) v = (v - mean) / std;
      }
      op[x] = v;
    }
  }
}

extern "C" int cenet_sw_windows_f32(const float* src, float* out, const int* oy_host, const int* ox_host, int n, int C, int H, int W,
                                    int PH, int PW, int nwy, int nwx, int normalize, float mean, float std, float pad_value,
                                    hipStream_t stream) {
  if (!src || !out || !oy_host || !ox_host) return CENET_EINVAL;
  if (n <= 0 || C <= 0 || H < 1 || W < 1 || PH < 1 || PW < 1) return CENET_EINVAL;
  if ((long)H * W > 0x7FFFFFFFL || (long)PH * PW > 0x7FFFFFFFL) return CENET_EINVAL;
  SwTab tab;
  if (!sw_tables(tab, oy_host, ox_host, nwy, nwx, PH, PW, H, W)) return CENET_EINVAL;
  const long nrows = (long)n * nwy * nwx * C * PH;
  const long groups = (nrows + 3) / 4, blocks = groups < 8192 ? groups : 8192;
  CENET_LAUNCH(sw_windows_kernel, dim3((unsigned)blocks), dim3(256), stream, src, out, tab, C, H, W, PH, PW, nwy, nwx, normalize, mean,
               std, pad_value, nrows);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// All loops over the classes have the fixed bound SW_MAXK, so v[] and acc[] are registers (as in tta.hip).
template <typename T>
__global__ __launch_bounds__(256) void sw_merge_counts_kernel(const T* __restrict__ logits, const float* __restrict__ labels,
                                                             const float* __restrict__ wy, const float* __restrict__ wx,
                                                             float* __restrict__ pred, float* __restrict__ conf,
                                                             unsigned* __restrict__ counts, SwTab tab, int n, int K, int PH, int PW, int H,
                                                             int W, int nwy, int nwx, int view_mask, float tviews, int tiles_x,
                                                             int tiles_y, long ntiles) {
  __shared__ unsigned sc[(SW_MAXK + 1) * 3];
  for (int i = threadIdx.x; i < (K + 1) * 3; i += 256) sc[i] = 0u;
  __syncthreads();
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const long HW = (long)H * W, PHW = (long)PH * PW, tpp = (long)tiles_x * tiles_y;
  const long vstride = (long)n * nwy * nwx * K * PHW;  // one view's logit stack
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long b = t / tpp;
    const int tt = (int)(t - b * tpp);
    const int tx0 = (tt % tiles_x) * SW_TILE, ty0 = (tt / tiles_x) * SW_TILE;
    // the windows that can touch this tile: the same for every lane
    const int ty1 = (ty0 + SW_TILE < H ? ty0 + SW_TILE : H) - 1, tx1 = (tx0 + SW_TILE < W ? tx0 + SW_TILE : W) - 1;
    int iy0 = 0, iy1 = nwy - 1, ix0 = 0, ix1 = nwx - 1;
    while (iy0 < iy1 && tab.oy[iy0] + PH <= ty0) ++iy0;
    while (iy1 > iy0 && tab.oy[iy1] > ty1) --iy1;
    while (ix0 < ix1 && tab.ox[ix0] + PW <= tx0) ++ix0;
    while (ix1 > ix0 && tab.ox[ix1] > tx1) --ix1;
    const int x = tx0 + lx;
    if (x >= W) continue;
    for (int i = 0; i < 4; ++i) {
      const int y = ty0 + ly + 8 * i;
      if (y >= H) break;
      float acc[SW_MAXK];
#pragma unroll
      for (int c = 0; c < SW_MAXK; ++c) acc[c] = 0.f;
      float wsum = 0.f;
      for (int iy = iy0; iy <= iy1; ++iy) {
        const int py = y - tab.oy[iy];
        if (py < 0 || py >= PH) continue;
        const float wrow = wy[py];
        for (int ix = ix0; ix <= ix1; ++ix) {
          const int px = x - tab.ox[ix];
          if (px < 0 || px >= PW) continue;
          const float w = wrow * wx[px];
          const T* lb = logits + ((b * nwy + iy) * nwx + ix) * (long)K * PHW;
          for (int g = 0; g < 8; ++g) {
            if (!((view_mask >> g) & 1)) continue;
            const int p = (g & 4) ? px : py, q = (g & 4) ? py : px;
            const int yv = (g & 2) ? PH - 1 - p : p, xv = (g & 1) ? PW - 1 - q : q;
            const T* lp = lb + (long)yv * PW + xv;
            lb += vstride;
            float v[SW_MAXK];
            float m = ldf(lp);
            v[0] = m;
#pragma unroll
            for (int c = 1; c < SW_MAXK; ++c)
              if (c < K) {
                v[c] = ldf(lp + (long)c * PHW);
                m = v[c] > m ? v[c] : m;
              }
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < SW_MAXK; ++c)
              if (c < K) {
                v[c] = expf(v[c] - m);
                s += v[c];
              }
            const float inv = 1.f / s;
#pragma unroll
            for (int c = 0; c < SW_MAXK; ++c)
              if (c < K) acc[c] += w * (v[c] * inv);
          }
          wsum += w;
        }
      }
      int arg = 0;
      float best = acc[0];
#pragma unroll
      for (int c = 1; c < SW_MAXK; ++c)
        if (c < K && acc[c] > best) {
          best = acc[c];
          arg = c;
        }
      const long e = b * HW + (long)y * W + x;
      pred[e] = (float)arg;
      if (conf) conf[e] = best / (wsum * tviews);  // (wsum holds every covering window's w once, the sums once per view)
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
static int sw_merge_counts_impl(const T* logits, const float* labels, const float* wy, const float* wx, const int* oy_host,
                                const int* ox_host, float* pred, float* conf, unsigned* counts, int n, int K, int PH, int PW, int H, int W,
                                int nwy, int nwx, int view_mask, hipStream_t stream) {
  if (!logits || !pred || !wy || !wx || !oy_host || !ox_host || (labels && !counts)) return CENET_EINVAL;
  if (n <= 0 || K <= 0 || K > SW_MAXK || H < 1 || W < 1 || PH < 1 || PW < 1) return CENET_EINVAL;
  if (view_mask < 1 || view_mask > 255 || ((view_mask & 0xF0) && PH != PW)) return CENET_EINVAL;
  if ((long)H * W > 0x7FFFFFFFL || (long)PH * PW > 0x7FFFFFFFL) return CENET_EINVAL;
  SwTab tab;
  if (!sw_tables(tab, oy_host, ox_host, nwy, nwx, PH, PW, H, W)) return CENET_EINVAL;
  if (labels && cenet_zero_async((float*)counts, (K + 1) * 3L, stream) != CENET_OK) return CENET_EINVAL;
  int T_views = 0;
  for (int g = 0; g < 8; ++g) T_views += (view_mask >> g) & 1;
  const int tiles_x = cdiv(W, SW_TILE), tiles_y = cdiv(H, SW_TILE);
  const long ntiles = (long)n * tiles_x * tiles_y;
  const long blocks = ntiles < 4096 ? ntiles : 4096;
  CENET_LAUNCH((sw_merge_counts_kernel<T>), dim3((unsigned)blocks), dim3(256), stream, logits, labels, wy, wx, pred, conf, counts, tab,
               n, K, PH, PW, H, W, nwy, nwx, view_mask, (float)T_views, tiles_x, tiles_y, ntiles);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(sw_merge_counts, (const T* logits, const float* labels, const float* wy, const float* wx, const int* oy_host,
                             const int* ox_host, float* pred, float* conf, unsigned* counts, int n, int K, int PH, int PW, int H, int W,
                             int nwy, int nwx, int view_mask, hipStream_t stream),
           (logits, labels, wy, wx, oy_host, ox_host, pred, conf, counts, n, K, PH, PW, H, W, nwy, nwx, view_mask, stream))
