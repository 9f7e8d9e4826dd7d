// seg_loss_ex.hip — the fused segmentation loss with the options loss_optim.hip does not take: per-class weights for the Dice
// and cross-entropy terms, ignore_index, a Jaccard term and DiceLoss(softmax=False).
//   DiceLoss(weight, softmax)   utils/core.py:44-80        JaccardLoss(ignore_index, smooth)   utils/core.py:134-158
//   flatten(ignore_index)       utils/utils.py:39-50       CrossEntropyLoss(weight, ignore_index): torch, mean reduction
// loss = w_dice Dice + w_ce CE + w_bd BoundaryDoU + w_jac Jaccard from ONE pass over the logits.  With M = [label != ignore_index],
// t_c = [label == c] M and all sums over the whole batch:  I_c = sum M p_c t_c,  Z_c = sum M p_c^2,  Y_c = sum t_c,  S_c = sum M p_c,
// ceN = sum wc_t (-log p_t),  ceD = sum wc_t.
// STORE-AND-SUM, no float atomics: workgroup g of the forward kernel block-reduces its partials and stores them as row g of the
// workspace (ws[SEGX_HEAD + g * (5K+2) + value]); the finalize kernel — one workgroup, next launch on the same stream — folds
// the rows in a fixed order in double and writes the compact sums, the BoundaryDoU alpha and loss[0].  Every sum has one order of
// additions whatever the arrival order of the workgroups, so loss and gradient are bitwise reproducible.  Stream order is the
// only synchronisation.
#include "loss_pixel.h"
#include "../../include/cenet_hip.h"

// workspace head: [0..K) I, [K..2K) Z, [2K..3K) Y, [3K..4K) S, [4K..5K) boundary pixel counts, [5K] ceN, [5K+1] ceD,
// [5K+2..6K+2) BoundaryDoU alpha — what the backward kernel reads.  The rows of partials follow it.
#define SEGX_HEAD 128
enum { SEGX_BOUNDARY = 1, SEGX_IGNORE = 2, SEGX_PROBS = 4 };

static inline int segx_fwd_it(int K) { return K > 9 ? 4 : 8; }  // pixels per thread of the forward kernel
static inline long segx_rows(int B, int K, int HW) { return (long)cdiv(HW, 256 * segx_fwd_it(K)) * B; }

extern "C" long cenet_seg_loss_ex_ws_floats(int B, int K, int H, int W) {
  if (B <= 0 || K <= 0 || K > PX_MAXK || H <= 0 || W <= 0) return 0;
  return SEGX_HEAD + segx_rows(B, K, H * W) * (5 * K + 2);
}

// cw: [2K] class weights (Dice, then CE) or NULL.
template <typename T, int KM>
__global__ __launch_bounds__(256) void segx_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ labels,
                                                      const float* __restrict__ cw, float* __restrict__ rows, int K, int HW,
                                                      int W, int flags, int ignore_index) {
  constexpr int NVM = 5 * KM + 2;
  __shared__ float wred[4][NVM];
  float part[NVM];  // [0,KM) I, [KM,2KM) Z, [2KM,3KM) Y, [3KM,4KM) S, [4KM,5KM) boundary, [5KM] ceN, [5KM+1] ceD
#pragma unroll
  for (int i = 0; i < NVM; ++i) part[i] = 0.f;
  float wc[KM];
#pragma unroll
  for (int c = 0; c < KM; ++c) wc[c] = (cw && c < K) ? cw[K + c] : 1.f;
  const bool boundary = flags & SEGX_BOUNDARY, has_ignore = flags & SEGX_IGNORE, probs = flags & SEGX_PROBS;
  // grid (ceil(HW / (256 IT)), B): a thread owns IT pixels of image blockIdx.y, two at a time
  constexpr int IT = KM > 9 ? 4 : 8;
  const int H = HW / W, b = blockIdx.y;
  const T* lb0 = logits + (long)b * K * HW;
  const float* lab = labels + (long)b * HW;
#pragma unroll 1
  for (int k0 = 0; k0 < IT; k0 += 2) {
    float vv[2][KM], tl[2];
    int pp[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int p = (blockIdx.x * IT + k0 + k) * 256 + threadIdx.x;
      pp[k] = p < HW ? p : -1;
      const int q = p < HW ? p : 0;
      px_load<KM>(vv[k], lb0, HW, q, K);
      tl[k] = lab[q];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (pp[k] < 0) continue;
      const int p = pp[k];
      const int t = (int)tl[k];
      if (has_ignore && t == ignore_index) continue;  // M = 0: the pixel adds to no sum
      float* v = vv[k];
      if (!probs) px_softmax<KM, false>(v, K);
      bool edge = false;
      if (boundary) {  // a pixel of class t is a boundary pixel unless its four neighbours (zero padded) share t
        const int py = p / W, px = p - py * W;
        edge = !(py > 0 && (int)lab[p - W] == t && py + 1 < H && (int)lab[p + W] == t && px > 0 && (int)lab[p - 1] == t &&
                 px + 1 < W && (int)lab[p + 1] == t);
      }
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < K) {
          const float pc = v[c];
          part[KM + c] += pc * pc;
          part[3 * KM + c] += pc;
          if (c == t) {
            part[c] += pc;
            part[2 * KM + c] += 1.f;
            if (edge) part[4 * KM + c] += 1.f;
            if (!probs) {
              part[5 * KM] -= wc[c] * fast_log(fmaxf(pc, 1e-37f));
              part[5 * KM + 1] += wc[c];
            }
          }
        }
    }
  }
  // wave sums -> LDS -> the four waves added in a fixed order -> this workgroup's row, stored by 5K+2 lanes
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll  // static indices: part[] must stay in registers
  for (int i = 0; i < NVM; ++i) {
    if (!boundary && i >= 4 * KM && i < 5 * KM) continue;
    const float s = wave_sum(part[i]);
    if (lane == 0) wred[wave][i] = s;
  }
  __syncthreads();
  const int NV = 5 * K + 2, j = threadIdx.x;
  if (j < NV) {
    const int grp = j / K, m = grp < 5 ? grp * KM + (j - grp * K) : 5 * KM + (j - 5 * K);
    float s = 0.f;
    if (boundary || grp != 4) s = (wred[0][m] + wred[1][m]) + (wred[2][m] + wred[3][m]);
    rows[((long)blockIdx.y * gridDim.x + blockIdx.x) * NV + j] = s;
  }
}

// one workgroup of 1024 threads: thread (g, v) adds rows g, g + G, g + 2G, ... of value v, then thread v adds the G group sums
__global__ __launch_bounds__(1024) void segx_finalize_kernel(float* __restrict__ ws, float* __restrict__ loss,
                                                            const float* __restrict__ cw, long nrows, int K, float w_dice,
                                                            float w_ce, float w_bd, float w_jac, float smooth) {
  __shared__ double grp_sum[1024];
  __shared__ double tot[5 * PX_MAXK + 2];
  const int NV = 5 * K + 2, G = 1024 / NV, t = threadIdx.x;
  const float* rows = ws + SEGX_HEAD;
  if (t < G * NV) {
    const int v = t % NV, g = t / NV;
    double s = 0.0;
    for (long r = g; r < nrows; r += G) s += (double)rows[r * NV + v];
    grp_sum[t] = s;
  }
  __syncthreads();
  if (t < NV) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += grp_sum[g * NV + t];
    tot[t] = s;
    ws[t] = (float)s;
  }
  __syncthreads();
  if (t == 0) {
    double d = 0.0, bd = 0.0, jac = 0.0;
    for (int c = 0; c < K; ++c) {
      const double I = tot[c], z = tot[K + c], y = tot[2 * K + c], S = tot[3 * K + c];
      const double wd = cw ? (double)cw[c] : 1.0;
      d += wd * (1.0 - (2.0 * I + 1e-5) / (z + y + 1e-5));
      // BoundaryDoU (core.py:110-121): alpha from the boundary / area ratio of the class mask, truncated at 0.8
      double alpha = 2.0 * (1.0 - (tot[4 * K + c] + 1e-5) / (y + 1e-5)) - 1.0;
      if (alpha > 0.8) alpha = 0.8;
      ws[5 * K + 2 + c] = (float)alpha;
      bd += (z + y - 2.0 * I + 1e-5) / (z + y - (1.0 + alpha) * I + 1e-5);
      jac += 1.0 - (I + (double)smooth) / (S + y - I + (double)smooth);
    }
    double l = 0.0;  // a term with weight 0 is left out, not multiplied by 0: CE of an all-ignored batch is 0 / 0 = NaN (as torch's)
    if (w_dice != 0.f) l += (double)w_dice * d / K;
    if (w_ce != 0.f) l += (double)w_ce * tot[5 * K] / tot[5 * K + 1];
    if (w_bd != 0.f) l += (double)w_bd * bd / K;
    if (w_jac != 0.f) l += (double)w_jac * jac / K;
    loss[0] = (float)l;
  }
}

// dL/dp_c = M (A_c [t = c] + Bc_c p_c + Cc_c); through the softmax Jacobian unless the input already holds probabilities
template <typename T, int KM>
__global__ __launch_bounds__(256) void segx_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ labels,
                                                      const float* __restrict__ cw, const float* __restrict__ ws,
                                                      const float* __restrict__ gout, T* __restrict__ dlogits, int K, int HW,
                                                      float w_dice, float w_ce, float w_bd, float w_jac, float smooth, int flags,
                                                      int ignore_index) {
  const float go = gout[0];
  const bool has_ignore = flags & SEGX_IGNORE, probs = flags & SEGX_PROBS;
  float A[KM], Bc[KM], Cc[KM], wc[KM];
#pragma unroll
  for (int c = 0; c < KM; ++c)
    if (c < K) {
      const float I = ws[c], Y = ws[2 * K + c], zy = ws[K + c] + Y;
      const float D = zy + 1e-5f;
      const float num = 2.f * I + 1e-5f;
      const float wd = (cw ? cw[c] : 1.f) * w_dice / K;
      wc[c] = cw ? cw[K + c] : 1.f;
      A[c] = -wd * 2.f / D;
      Bc[c] = wd * num * 2.f / (D * D);
      Cc[c] = 0.f;
      if (w_bd != 0.f) {  // L_c = N / Db, N = z+y-2I+eps, Db = z+y-(1+alpha)I+eps ; dz/dp = 2p, dI/dp = t
        const float alpha = ws[5 * K + 2 + c];
        const float N = zy - 2.f * I + 1e-5f, Db = zy - (1.f + alpha) * I + 1e-5f;
        A[c] += w_bd / K * (N * (1.f + alpha) - 2.f * Db) / (Db * Db);
        Bc[c] += w_bd / K * 2.f * (Db - N) / (Db * Db);
      }
      if (w_jac != 0.f) {  // L_c = 1 - (I+s) / U, U = S+Y-I+s ; dI/dp = t, dS/dp = 1
        const float U = ws[3 * K + c] + Y - I + smooth, r = (I + smooth) / (U * U);
        A[c] -= w_jac / K * (1.f / U + r);
        Cc[c] = w_jac / K * r;
      }
    }
  const float cew = w_ce != 0.f ? w_ce / ws[5 * K + 1] : 0.f;
  constexpr int IT = 4;  // grid (ceil(HW / (256 IT)), B)
  const int b = blockIdx.y;
  const T* lb0 = logits + (long)b * K * HW;
  T* db0 = dlogits + (long)b * K * HW;
  const float* lab = labels + (long)b * HW;
  float vv[IT][KM], tl[IT];
  int pp[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int p = (blockIdx.x * IT + k) * 256 + threadIdx.x;
    pp[k] = p < HW ? p : -1;
    const int q = p < HW ? p : 0;
    px_load<KM>(vv[k], lb0, HW, q, K);
    tl[k] = lab[q];
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    if (pp[k] < 0) continue;
    const int t = (int)tl[k];
    float* v = vv[k];
    if (has_ignore && t == ignore_index) {  // exactly 0.0 in every class
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < K) stf(db0 + (long)c * HW + pp[k], 0.f);
      continue;
    }
    if (probs) {
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < K) stf(db0 + (long)c * HW + pp[k], go * (Bc[c] * v[c] + (c == t ? A[c] : 0.f) + Cc[c]));
      continue;
    }
    px_softmax<KM, false>(v, K);
    float gp[KM];
    float dot = 0.f, wt = 0.f;
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) {
        gp[c] = Bc[c] * v[c] + (c == t ? A[c] : 0.f) + Cc[c];
        dot += gp[c] * v[c];
        if (c == t) wt = wc[c];
      }
    const float cet = cew * wt;
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) stf(db0 + (long)c * HW + pp[k], go * (v[c] * (gp[c] - dot) + cet * (v[c] - (c == t ? 1.f : 0.f))));
  }
}

static int segx_check(int B, int K, int H, int W, float w_ce, float w_bd, float w_jac, int has_ignore, int from_probs) {
  if (B <= 0 || K <= 0 || K > PX_MAXK || H <= 0 || W <= 0) return CENET_EINVAL;
  if (B > 65535) return CENET_EUNSUPPORTED;
  if (from_probs && (w_ce != 0.f || w_bd != 0.f || w_jac != 0.f)) return CENET_EINVAL;  // DiceLoss(softmax=False) only
  if (has_ignore && w_bd != 0.f) return CENET_EUNSUPPORTED;  // a boundary count over a mask with holes is not defined
  return CENET_OK;
}

template <typename T>
static int seg_loss_ex_fwd_impl(const T* logits, const float* labels, const float* cw, float* ws, long ws_floats, float* loss,
                                int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac, float smooth,
                                int has_ignore, int ignore_index, int from_probs, hipStream_t stream) {
  const int rc = segx_check(B, K, H, W, w_ce, w_bd, w_jac, has_ignore, from_probs);
  if (rc != CENET_OK) return rc;
  if (!logits || !labels || !ws || !loss || ws_floats < cenet_seg_loss_ex_ws_floats(B, K, H, W)) return CENET_EINVAL;
  const int HW = H * W;
  const dim3 blocks(cdiv(HW, 256 * segx_fwd_it(K)), B);
  const int flags = (w_bd != 0.f ? SEGX_BOUNDARY : 0) | (has_ignore ? SEGX_IGNORE : 0) | (from_probs ? SEGX_PROBS : 0);
  float* rows = ws + SEGX_HEAD;
  CENET_LAUNCH_KM(segx_fwd_kernel, T, K, blocks, dim3(256), stream, logits, labels, cw, rows, K, HW, W, flags, ignore_index);
  CENET_LAUNCH(segx_finalize_kernel, dim3(1), dim3(1024), stream, ws, loss, cw, segx_rows(B, K, HW), K, w_dice, w_ce, w_bd, w_jac,
               smooth);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(seg_loss_ex_fwd, (const T* logits, const float* labels, const float* cw, float* ws, long ws_floats, float* loss, int B,
                             int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac, float smooth, int has_ignore,
                             int ignore_index, int from_probs, hipStream_t stream),
           (logits, labels, cw, ws, ws_floats, loss, B, K, H, W, w_dice, w_ce, w_bd, w_jac, smooth, has_ignore, ignore_index,
            from_probs, stream))

template <typename T>
static int seg_loss_ex_bwd_impl(const T* logits, const float* labels, const float* cw, const float* ws, const float* gout,
                                T* dlogits, int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac,
                                float smooth, int has_ignore, int ignore_index, int from_probs, hipStream_t stream) {
  const int rc = segx_check(B, K, H, W, w_ce, w_bd, w_jac, has_ignore, from_probs);
  if (rc != CENET_OK) return rc;
  if (!logits || !labels || !ws || !gout || !dlogits) return CENET_EINVAL;
  const int HW = H * W;
  const dim3 blocks(cdiv(HW, 256 * 4), B);
  const int flags = (has_ignore ? SEGX_IGNORE : 0) | (from_probs ? SEGX_PROBS : 0);
  CENET_LAUNCH_KM(segx_bwd_kernel, T, K, blocks, dim3(256), stream, logits, labels, cw, ws, gout, dlogits, K, HW, w_dice, w_ce, w_bd, w_jac, smooth,
                  flags, ignore_index);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(seg_loss_ex_bwd, (const T* logits, const float* labels, const float* cw, const float* ws, const float* gout, T* dlogits,
                             int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac, float smooth,
                             int has_ignore, int ignore_index, int from_probs, hipStream_t stream),
           (logits, labels, cw, ws, gout, dlogits, B, K, H, W, w_dice, w_ce, w_bd, w_jac, smooth, has_ignore, ignore_index,
            from_probs, stream))
