// chanloc.hip — CHANNEL-LOCAL fused chains of the decoder (round 5).
//
// BatchNorm couples the images of a batch, depthwise convs / nearest up-sampling / per-channel gates do not couple channels: a
// chain made of such steps only ever mixes the values of ONE channel.  One workgroup therefore owns one channel over the whole
// batch and runs the chain start to end — batch statistics are workgroup reductions (no second launch, no partial-sum round
// trip, no float atomics: the results do not depend on scheduling), intermediates live in LDS or are recomputed, and only the
// tensors the next channel-MIXING step (a 1x1 conv) needs are written.  At the 7x7 ... 28x28 decoder levels of a 224x224
// input a channel over a batch of 32 is 1.5 ... 25 K values: the launches this replaces were bound by their fill / drain
// latency, not by bytes (profiles/r04_*: ~120 dependent launches per level on <= 4 MB tensors).
//
//   eucb_{fwd,bwd}   blocks.py:297-321 EUCB up to its 1x1 conv: nearest x2 -> DW3x3 -> BatchNorm(train) -> LeakyReLU.
//                    The up-sampled tensor and the conv output are never stored (forward: 4 launches -> 1; backward: the
//                    BatchNorm backward, LeakyReLU mask, depthwise data + weight gradient and the x2 fold: 5 launches -> 1).
//
// Templates over the activation storage type T (float: parity mode, bf16_t: throughput mode); arithmetic in fp32.
#include "common.h"
#include <cstdlib>
#include "../../include/cenet_hip.h"

// elements of one channel over the batch (B * HW) up to which a workgroup owns a whole channel (28 x 28 planes at a batch of 32 and
// some headroom; beyond that the launch chains with partial sums over many workgroups win)
#define CENET_CHANLOC_MAX 32768

// (no anonymous namespace: the kernels keep plain names, as the profiler tools of tools/ key on them)

// sum over the workgroup of N values at once (one barrier pair for all of them); result in every thread.  red: >= 16 * N floats
template <int N>
__device__ __forceinline__ void block_sum_n(float (&v)[N], float* red) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum_dpp(v[k]);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (l == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[w * N + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i * N + k];
    v[k] = t;
  }
}

// Shift of a one-pass variance: BatchNorm's batch variance is formed as s2 / n - (s1 / n)^2 from sums of (x - K) and (x - K)^2,
// which is only as good as K is close to the mean.  K is the mean of the first min(HW, 64) values of image 0's plane (as
// norm.hip's bn_shift_block: NOT one sample, a single outlier there cost the variance 1e-3 of its value), one sample per
// lane, taken by EVERY wave for itself: no barrier, the same value in every thread.  v: the lane's sample; m: samples.
__device__ __forceinline__ float shift_mean(float v, int m) {
  return wave_sum_dpp(((int)threadIdx.x & 63) < m ? v : 0.f) / (float)m;
}

// Strided walks without a division per element: thread t visits e = t, t + NT, ... of a [B][HW] (or [B][H][W]) index space and
// keeps (b, p) / (b, i, j) up to date with adds and carries (an integer division by a run-time value is ~40 instructions: more
// than the arithmetic of any element here).
struct Walk2 {
  int b, p, dB, dP, HW;
  __device__ __forceinline__ Walk2(int e0, int stride, int HW_) : HW(HW_) {
    b = e0 / HW_;
    p = e0 - b * HW_;
    dB = stride / HW_;
    dP = stride - dB * HW_;
  }
  __device__ __forceinline__ void next() {
    p += dP;
    b += dB;
    if (p >= HW) {
      p -= HW;
      ++b;
    }
  }
};
struct Walk3 {
  int b, i, j, dB, dI, dJ, H, W;
  __device__ __forceinline__ Walk3(int e0, int stride, int H_, int W_) : H(H_), W(W_) {
    const int HW = H_ * W_;
    b = e0 / HW;
    int p = e0 - b * HW;
    i = p / W_;
    j = p - i * W_;
    dB = stride / HW;
    p = stride - dB * HW;
    dI = p / W_;
    dJ = p - dI * W_;
  }
  __device__ __forceinline__ void next() {
    j += dJ;
    i += dI;
    b += dB;
    if (j >= W) {
      j -= W;
      ++i;
    }
    if (i >= H) {
      i -= H;
      ++b;
    }
  }
};

struct EucbArgs {
  const void* x;   // [B, C, H, W] (batch stride sxb)
  long sxb;
  void* y;         // forward: [B, C, 2H, 2W] (batch stride syb)       backward: dx [B, C, H, W] (batch stride syb)
  long syb;
  const void* g;   // backward: gradient of the LeakyReLU output [B, C, 2H, 2W] (batch stride sgb)
  long sgb;
  const float* w;  // [C][9]
  const float *gamma, *beta;
  float eps, slope;
  float *mean, *var;             // forward: written; backward: read
  float *rmean, *rvar;           // forward: running statistics (may be null)
  float momentum;
  long* nbt;
  float *dw, *dgamma, *dbeta;    // backward: ADDED into (this workgroup is the only writer of its channel's entries)
  int B, H, W;
};

// The 2x2 output quad of source pixel (i, j) reads the 3x3 source neighbourhood S (zero outside the plane: the conv pads the
// UP-SAMPLED grid, whose border pixels are copies of the source border, so "outside" coincides):
//   up rows 2i-1, 2i, 2i+1 (output row 2i)   -> source rows i-1, i, i      up rows 2i, 2i+1, 2i+2 (row 2i+1) -> i, i, i+1
// so output parity py touches only S rows {py, py + 1} (S row 0 = i - 1), with the taps that fall on one source row summed:
//   u[py][px] = sum_{a2, c2 in {0, 1}} q[py][px][a2][c2] * S[py + a2][px + c2],
//   q = sum of w[ky][kx] over KY(py, a2) x KX(px, c2),   KY(0, 0) = {0}, KY(0, 1) = {1, 2}, KY(1, 0) = {0, 1}, KY(1, 1) = {2}
// 16 FMAs per quad instead of 36.  The planes sit in LDS with a one-pixel ZERO border ([H + 2][W + 2]): no bounds tests.
__device__ __forceinline__ int eucb_a2(int par, int k) { return par == 0 ? (k == 0 ? 0 : 1) : (k == 2 ? 1 : 0); }

__device__ __forceinline__ void eucb_combine(const float (&w)[9], float (&q)[2][2][2][2]) {
#pragma unroll
  for (int py = 0; py < 2; ++py)
#pragma unroll
    for (int px = 0; px < 2; ++px) {
#pragma unroll
      for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) q[py][px][a2][c2] = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) q[py][px][eucb_a2(py, ky)][eucb_a2(px, kx)] += w[ky * 3 + kx];
    }
}

// channel planes of the batch -> LDS [B][H + 2][W + 2] with a zero border, as FP32 whatever the tensor type: 2-byte LDS elements
// made the tap reads misaligned ds_read_b32 / ds_read_u16 pairs (SQ_WAIT_INST_LDS 39 % of the wave cycles, ~180 cycles per LDS
// instruction); aligned dwords, consecutive lanes on consecutive banks, read at full rate
template <typename T>
__device__ __forceinline__ void eucb_stage(const T* x, long sxb, float* xs, int B, int H, int W, int NT) {
  const int PW = W + 2, tot = B * (H + 2) * PW;
  Walk3 k(threadIdx.x, NT, H + 2, PW);
  // eight elements per trip, their loads issued together on clamped addresses (a branch around a load, or a trip per load,
  // puts one full memory round trip between consecutive loads: measured 3x on this loop)
  for (int e0 = threadIdx.x; e0 < tot; e0 += 8 * NT) {
    float v[8];
    bool in[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int yy = k.i - 1, xx = k.j - 1;
      in[u] = e0 + u * NT < tot && yy >= 0 && yy < H && xx >= 0 && xx < W;
      v[u] = ldf(x + (in[u] ? (long)k.b * sxb + yy * W + xx : 0));
      k.next();
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (e0 + u * NT < tot) xs[e0 + u * NT] = in[u] ? v[u] : 0.f;
  }
}
__device__ __forceinline__ void eucb_load_nb(const float* xs, int b, int i, int j, int H, int W, float (&S)[3][3]) {
  const float* p = xs + ((long)b * (H + 2) + i) * (W + 2) + j;  // padded row i = source row i - 1
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[a][c] = p[a * (W + 2) + c];
}
// the four conv outputs of the quad: u[py][px]
__device__ __forceinline__ void eucb_quad(const float (&S)[3][3], const float (&q)[2][2][2][2], float (&u)[2][2]) {
#pragma unroll
  for (int py = 0; py < 2; ++py)
#pragma unroll
    for (int px = 0; px < 2; ++px)
      u[py][px] = q[py][px][0][0] * S[py][px] + q[py][px][0][1] * S[py][px + 1] + q[py][px][1][0] * S[py + 1][px] +
                  q[py][px][1][1] * S[py + 1][px + 1];
}

// grid = C, NT threads, SM bytes of LDS holding the channel's padded source planes as T
template <typename T, int NT, int SM>
__global__ __launch_bounds__(NT) void eucb_fwd_kernel(EucbArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[SM];
  __shared__ float red[16 * 2];
  float* xs = (float*)smem;
  const int c = blockIdx.x, H = a.H, W = a.W, HW = H * W, items = a.B * HW;
  eucb_stage((const T*)a.x + (long)c * HW, a.sxb, xs, a.B, H, W, NT);
  float q[2][2][2][2];
  {
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = a.w[c * 9 + k];
    eucb_combine(w, q);
  }
  __syncthreads();
  // pass 1: batch statistics of the conv output (fp32 sums of squares, shifted by the mean of the quads of image 0's first
  // min(HW, 64) source pixels: shift_mean)
  float S[3][3], u[2][2];
  const int ms = HW < 64 ? HW : 64;
  {
    const int ps = ((int)threadIdx.x & 63) < ms ? ((int)threadIdx.x & 63) : 0;
    eucb_load_nb(xs, 0, ps / W, ps % W, H, W, S);
    eucb_quad(S, q, u);
  }
  const float K = shift_mean(0.25f * ((u[0][0] + u[0][1]) + (u[1][0] + u[1][1])), ms);
  float s[2] = {0.f, 0.f};
  Walk3 wk(threadIdx.x, NT, H, W);
  for (int e = threadIdx.x; e < items; e += NT, wk.next()) {
    eucb_load_nb(xs, wk.b, wk.i, wk.j, H, W, S);
    eucb_quad(S, q, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = u[k >> 1][k & 1] - K;
      s[0] += d;
      s[1] += d * d;
    }
  }
  block_sum_n<2>(s, red);
  const float n = 4.f * (float)items;
  const float m = s[0] / n;
  float var = s[1] / n - m * m;
  if (var < 0.f) var = 0.f;
  const float mu = K + m;
  if (threadIdx.x == 0) {
    a.mean[c] = mu;
    a.var[c] = var;
    if (a.rmean) {
      a.rmean[c] = (1.f - a.momentum) * a.rmean[c] + a.momentum * mu;
      a.rvar[c] = (1.f - a.momentum) * a.rvar[c] + a.momentum * var * (n / (n - 1.f));
    }
    if (a.nbt && c == 0) a.nbt[0] += 1;
  }
  const float sc = a.gamma[c] * rsqrtf(var + a.eps), sh = a.beta[c] - mu * sc;
  // pass 2: normalise + LeakyReLU + store (two pixels = one 4-byte / 8-byte store per output row)
  const int OW = 2 * W;
  T* y = (T*)a.y + (long)c * 4 * HW;
  wk = Walk3(threadIdx.x, NT, H, W);
  for (int e = threadIdx.x; e < items; e += NT, wk.next()) {
    eucb_load_nb(xs, wk.b, wk.i, wk.j, H, W, S);
    eucb_quad(S, q, u);
    T* yp = y + (long)wk.b * a.syb + (long)(2 * wk.i) * OW + 2 * wk.j;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      float v0 = u[py][0] * sc + sh, v1 = u[py][1] * sc + sh;
      v0 = v0 > 0.f ? v0 : v0 * a.slope;
      v1 = v1 > 0.f ? v1 : v1 * a.slope;
      if (sizeof(T) == 2) {
        const unsigned pk = cenet_pack_bf2(v0, v1);
        memcpy(yp + py * OW, &pk, 4);
      } else {
        const float pr[2] = {v0, v1};
        memcpy(yp + py * OW, pr, 8);
      }
    }
  }
}

// backward.  LDS: the padded source planes as T, then G zero-bordered planes [2H + 2][2W + 2] of fp32 conv-output gradients (one
// group of G images at a time: the depthwise data gradient needs the neighbours of an output pixel's gradient)
template <typename T, int NT, int SM>
__global__ __launch_bounds__(NT) void eucb_bwd_kernel(EucbArgs a, int G) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[SM];
  __shared__ float red[16 * 11];
  const int c = blockIdx.x, H = a.H, W = a.W, HW = H * W, items = a.B * HW, OW = 2 * W, OH = 2 * H;
  const int DW_ = OW + 2, DP = (OH + 2) * DW_;
  float* xs = (float*)smem;
  float* du = (float*)(smem + (((long)a.B * (H + 2) * (W + 2) * 4 + 15) & ~15L));
  eucb_stage((const T*)a.x + (long)c * HW, a.sxb, xs, a.B, H, W, NT);
  for (int e = threadIdx.x; e < G * DP; e += NT) du[e] = 0.f;  // (the borders stay zero: only interiors are rewritten)
  float w[9], q[2][2][2][2];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = a.w[c * 9 + k];
  eucb_combine(w, q);
  const float mu = a.mean[c], rs = rsqrtf(a.var[c] + a.eps), gm = a.gamma[c], bt = a.beta[c];
  __syncthreads();
  const T* g = (const T*)a.g + (long)c * 4 * HW;
  float S[3][3], u[2][2];
  // the two output rows of a quad's gradient as loaded (bf16: one packed pair per row; fp32: two floats per row)
  struct GRaw {
    float v[2][2];
  };
  auto load_g = [&](int b, int i, int j) __attribute__((always_inline)) -> GRaw {
    GRaw r;
    const T* gp = g + (long)b * a.sgb + (long)(2 * i) * OW + 2 * j;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      if (sizeof(T) == 2) {
        unsigned pk;
        memcpy(&pk, gp + py * OW, 4);
        r.v[py][0] = cenet_bf2f(pk & 0xFFFFu), r.v[py][1] = cenet_bf2f(pk >> 16);
      } else {
        float pr[2];
        memcpy(pr, gp + py * OW, 8);
        r.v[py][0] = pr[0], r.v[py][1] = pr[1];
      }
    }
    return r;
  };
  // gradient of the quad's four conv outputs through LeakyReLU, and their normalised values
  auto quad_g = [&](int b, int i, int j, const GRaw& gr, float (&gy)[2][2], float (&xh)[2][2]) __attribute__((always_inline)) {
    eucb_load_nb(xs, b, i, j, H, W, S);
    eucb_quad(S, q, u);
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        xh[py][px] = (u[py][px] - mu) * rs;
        gy[py][px] = (xh[py][px] * gm + bt > 0.f) ? gr.v[py][px] : gr.v[py][px] * a.slope;
      }
  };
  // pass 1: sum g, sum g * xhat.  Four quads per trip, their gradient loads issued together (clamped indices).
  float s[2] = {0.f, 0.f};
  float gy[2][2], xh[2][2];
  Walk3 wk(threadIdx.x, NT, H, W);
  for (int e0 = threadIdx.x; e0 < items; e0 += 4 * NT) {
    int qb[4], qi[4], qj[4];
    GRaw gr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bool v = e0 + t * NT < items;
      qb[t] = v ? wk.b : 0, qi[t] = v ? wk.i : 0, qj[t] = v ? wk.j : 0;
      gr[t] = load_g(qb[t], qi[t], qj[t]);
      wk.next();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (e0 + t * NT < items) {
        quad_g(qb[t], qi[t], qj[t], gr[t], gy, xh);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          s[0] += gy[k >> 1][k & 1];
          s[1] += gy[k >> 1][k & 1] * xh[k >> 1][k & 1];
        }
      }
  }
  block_sum_n<2>(s, red);
  const float n = 4.f * (float)items, m1 = s[0] / n, m2 = s[1] / n, k0 = gm * rs;
  // combined weights of the data gradient: dx(i, j) = sum_{r, t = -1..2} cw[r+1][t+1] du(2i + r, 2j + t), where
  // cw = sum of w[ky][kx] over KY(r) x KX(t), KY(-1) = {2}, KY(0) = {1, 2}, KY(1) = {0, 1}, KY(2) = {0}
  float cw[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float v = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const bool iny = (r == 0 && ky == 2) || (r == 1 && ky >= 1) || (r == 2 && ky <= 1) || (r == 3 && ky == 0);
          const bool inx = (t == 0 && kx == 2) || (t == 1 && kx >= 1) || (t == 2 && kx <= 1) || (t == 3 && kx == 0);
          if (iny && inx) v += w[ky * 3 + kx];
        }
      cw[r][t] = v;
    }
  // weight-gradient sums in the basis of the combined weights (16 FMAs per quad), expanded to the 9 taps at the end
  float A[2][2][2][2];
#pragma unroll
  for (int k = 0; k < 16; ++k) A[k >> 3][(k >> 2) & 1][(k >> 1) & 1][k & 1] = 0.f;
  T* dx = (T*)a.y + (long)c * HW;
  for (int b0 = 0; b0 < a.B; b0 += G) {
    const int nb = a.B - b0 < G ? a.B - b0 : G;
    // (a) conv-output gradients of images b0 .. b0 + nb into LDS
    wk = Walk3(threadIdx.x, NT, H, W);
    for (int e0 = threadIdx.x; e0 < nb * HW; e0 += 4 * NT) {
      int qb[4], qi[4], qj[4];
      GRaw gr[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bool v = e0 + t * NT < nb * HW;
        qb[t] = v ? wk.b : 0, qi[t] = v ? wk.i : 0, qj[t] = v ? wk.j : 0;
        gr[t] = load_g(b0 + qb[t], qi[t], qj[t]);
        wk.next();
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (e0 + t * NT < nb * HW) {
          const int bl = qb[t], i = qi[t], j = qj[t];
          quad_g(b0 + bl, i, j, gr[t], gy, xh);
          float* dp = du + (long)bl * DP + (2 * i + 1) * DW_ + 2 * j + 1;
#pragma unroll
          for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
              const float d = k0 * (gy[py][px] - m1 - xh[py][px] * m2);
              dp[py * DW_ + px] = d;
#pragma unroll
              for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) A[py][px][a2][c2] += d * S[py + a2][px + c2];
            }
        }
    }
    __syncthreads();
    // (b) data gradient of the group's source pixels: the 4x4 window of padded rows 2i .. 2i + 3
    wk = Walk3(threadIdx.x, NT, H, W);
    for (int e = threadIdx.x; e < nb * HW; e += NT, wk.next()) {
      const int bl = wk.b, i = wk.i, j = wk.j, p = i * W + j;
      const float* dp = du + (long)bl * DP + (2 * i) * DW_ + 2 * j;
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) t += cw[r][k] * dp[r * DW_ + k];
      stf(dx + (long)(b0 + bl) * a.syb + p, t);
    }
    __syncthreads();
  }
  float fin[11];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      float v = 0.f;
#pragma unroll
      for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px) v += A[py][px][eucb_a2(py, ky)][eucb_a2(px, kx)];
      fin[ky * 3 + kx] = v;
    }
  fin[9] = 0.f, fin[10] = 0.f;
  block_sum_n<11>(fin, red);
  if (threadIdx.x < 9) a.dw[c * 9 + threadIdx.x] += fin[threadIdx.x];
  if (threadIdx.x == 9) a.dgamma[c] += s[1];
  if (threadIdx.x == 10) a.dbeta[c] += s[0];
}

// ---- CFAM "mid" chain (cfam.py:365-374 around nlb.py:140-148) --------------------------------------------------------------------
//   p = BatchNorm_nl(p_raw)            (the Non-local block's output conv, nlb.py:141-142)
//   z = (1 - w) m + w p                (nlb.py:148; m = the block's input, w a scalar parameter)
//   x1 = x0 + ls1 * z                  (cfam.py:370: layer-scale residual; x0 = the CFAM block's input)
//   y2 = BatchNorm_2(x1)               (cfam.py:372 norm2, input of the Mlp; x1 also feeds the second residual)
// Channel-local: workgroup = channel over the batch, three passes each way (the tensors are L2-resident at the levels this is
// used for).  Forward 5 - 6 launches -> 1, backward 6 - 7 -> 1.  Element e of the channel = (image e / HW, pixel e % HW);
// V = elements per access (4 when HW % 4 == 0).
struct MidArgs {
  const void *p_raw, *m, *x0;  // [B, C, HW] contiguous
  void *x1, *y2;               // forward outputs; backward: x1 is read
  const void *g_y2, *g_x1;     // backward inputs (g_x1 may be null)
  void *d_p, *d_m, *d_x0;      // backward outputs
  const float *gp, *bp, *g2, *b2, *w, *ls;
  float epsp, eps2;
  float *meanp, *varp, *mean2, *var2;
  float *rmp, *rvp, *rm2, *rv2;
  float momp, mom2;
  long *nbtp, *nbt2;
  float *dgp, *dbp, *dg2, *db2, *dw, *dls;  // ADDED into (dw: one float atomic per channel)
  int B, C, HW;
};

__device__ __forceinline__ void bn_publish(float* mean, float* var, float* rm, float* rv, float mom, long* nbt, int c, float mu,
                                           float v, float n) {
  mean[c] = mu;
  var[c] = v;
  if (rm) {
    rm[c] = (1.f - mom) * rm[c] + mom * mu;
    rv[c] = (1.f - mom) * rv[c] + mom * v * (n / (n - 1.f));
  }
  if (nbt && c == 0) nbt[0] += 1;
}
template <typename T>
__device__ __forceinline__ float round_to(float v) {
  return sizeof(T) == 2 ? cenet_bf2f(cenet_f2bf(v)) : v;
}

// ---- register-resident element ownership ------------------------------------------------------------------------------------
// A pass over a channel that loads, reduces, loads again ... pays one memory round trip per loop ITERATION when the trip count
// is a run-time value (the loads of iteration i + 1 sit behind the uses of iteration i): measured 15 - 25 us for 1.5 K elements.
// Here a thread OWNS up to EPT elements of the channel for the whole kernel: every input is loaded once, all loads of the kernel
// in flight together, every pass runs on registers, and the outputs are stored at the end.  Ownership is wave-per-image — wave
// w holds images w, w + nw, ... (slot s), lane l the pixels l, l + 64, ... (row r) — so that per-image reductions are shuffle
// trees inside one wave and batch reductions one LDS round.  Element k of a thread = (slot k / Rr, row k % Rr), Rr = ceil(HW / 64);
// slot and row advance with scalar adds under full unrolling.  The host picks EPT >= slots * Rr.
struct Own {
  int lane, wave, nw, Rr, B, HW;
  __device__ __forceinline__ Own(int B_, int HW_) : B(B_), HW(HW_) {
    lane = threadIdx.x & 63;
#ifdef CENET_HOSTSIM_BUILD
    wave = threadIdx.x >> 6;
#else
    wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#endif
    nw = (int)blockDim.x >> 6;
    Rr = (HW_ + 63) >> 6;
  }
};
// for (k, b, p, ok) over the thread's elements; BODY sees them as locals
#define OWN_FOR(o, ...)                                                           \
  {                                                                               \
    int s__ = 0, r__ = 0;                                                         \
    _Pragma("unroll") for (int k = 0; k < EPT; ++k) {                             \
      const int b = (o).wave + s__ * (o).nw, p = r__ * 64 + (o).lane;             \
      const bool ok = b < (o).B && p < (o).HW;                                    \
      __VA_ARGS__                                                                 \
      if (++r__ == (o).Rr) {                                                      \
        r__ = 0;                                                                  \
        ++s__;                                                                    \
      }                                                                           \
    }                                                                             \
  }

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void cfam_mid_fwd_kernel(MidArgs a) {
  __shared__ float red[16 * 2];
  const int c = blockIdx.x, C = a.C, HW = a.HW;
  const Own o(a.B, HW);
  const long cb = (long)c * HW, sb = (long)C * HW;
  const T *pr = (const T*)a.p_raw + cb, *mm = (const T*)a.m + cb, *x0 = (const T*)a.x0 + cb;
  T *x1 = (T*)a.x1 + cb, *y2 = (T*)a.y2 + cb;
  float P[EPT], M[EPT], X[EPT];
  // (loads are UNCONDITIONAL on a clamped offset and masked afterwards: a branch per element would put every load in a basic
  // block of its own, each followed by its wait — straight-line code lets them all issue back to back)
  OWN_FOR(o, {
    const long q = ok ? b * sb + p : 0;
    P[k] = ldf(pr + q);
    M[k] = ldf(mm + q);
    X[k] = ldf(x0 + q);
  })
  // (shifts of the sums of squares, shift_mean: image 0's first min(HW, 64) elements, one per lane)
  const int ms = HW < 64 ? HW : 64, ls_ = o.lane < ms ? o.lane : 0;
  const float SP = ldf(pr + ls_), SM_ = ldf(mm + ls_), SX = ldf(x0 + ls_);
  const float KP = shift_mean(SP, ms);
  const float n = (float)a.B * (float)HW, wv = a.w[0], ls = a.ls[c];
  // (every per-channel scalar is fetched HERE, with the tensor loads: a load issued after a barrier is a cold miss on the
  // critical path between two passes)
  const float gp_ = a.gp[c], bp_ = a.bp[c], g2_ = a.g2[c], b2_ = a.b2[c];
  float s[2] = {0.f, 0.f};
  OWN_FOR(o, {
    const float d = ok ? P[k] - KP : 0.f;
    s[0] += d;
    s[1] += d * d;
  })
  block_sum_n<2>(s, red);
  float mloc = s[0] / n;
  float varp = s[1] / n - mloc * mloc;
  if (varp < 0.f) varp = 0.f;
  const float mup = KP + mloc;
  if (threadIdx.x == 0) bn_publish(a.meanp, a.varp, a.rmp, a.rvp, a.momp, a.nbtp, c, mup, varp, n);
  const float ap = gp_ * rsqrtf(varp + a.epsp), cp = bp_ - mup * ap;
  // x1 and its statistics (of the values as stored: the backward pass normalises what it reads)
  const float K2 = shift_mean(round_to<T>(SX + ls * ((1.f - wv) * SM_ + wv * (ap * SP + cp))), ms);
  s[0] = s[1] = 0.f;
  OWN_FOR(o, {
    X[k] = round_to<T>(X[k] + ls * ((1.f - wv) * M[k] + wv * (ap * P[k] + cp)));
    const float d = ok ? X[k] - K2 : 0.f;
    s[0] += d;
    s[1] += d * d;
  })
  block_sum_n<2>(s, red);
  mloc = s[0] / n;
  float var2 = s[1] / n - mloc * mloc;
  if (var2 < 0.f) var2 = 0.f;
  const float mu2 = K2 + mloc;
  if (threadIdx.x == 0) bn_publish(a.mean2, a.var2, a.rm2, a.rv2, a.mom2, a.nbt2, c, mu2, var2, n);
  const float a2 = g2_ * rsqrtf(var2 + a.eps2), c2 = b2_ - mu2 * a2;
  OWN_FOR(o, {
    if (ok) {
      stf(x1 + b * sb + p, X[k]);
      stf(y2 + b * sb + p, a2 * X[k] + c2);
    }
  })
}

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void cfam_mid_bwd_kernel(MidArgs a) {
  __shared__ float red[16 * 4];
  const int c = blockIdx.x, C = a.C, HW = a.HW;
  const Own o(a.B, HW);
  const long cb = (long)c * HW, sb = (long)C * HW;
  const T *pr = (const T*)a.p_raw + cb, *mm = (const T*)a.m + cb, *x1 = (const T*)a.x1 + cb, *gy = (const T*)a.g_y2 + cb;
  const T* gx = a.g_x1 ? (const T*)a.g_x1 + cb : nullptr;
  T *dp = (T*)a.d_p + cb, *dm = (T*)a.d_m + cb, *dx0 = (T*)a.d_x0 + cb;
  float G[EPT], X[EPT], P[EPT], M[EPT], D[EPT];
  const T* gxs = gx ? gx : gy;  // (no tap: any valid address; the value is dropped)
  OWN_FOR(o, {
    const long q = ok ? b * sb + p : 0;
    G[k] = ldf(gy + q);
    X[k] = ldf(x1 + q);
    P[k] = ldf(pr + q);
    M[k] = ldf(mm + q);
    D[k] = ldf(gxs + q);
  })
  OWN_FOR(o, {
    if (!ok) G[k] = 0.f;
    if (!ok || !gx) D[k] = 0.f;
  })
  const float n = (float)a.B * (float)HW, wv = a.w[0], ls = a.ls[c];
  const float mu2 = a.mean2[c], rs2 = rsqrtf(a.var2[c] + a.eps2), k2 = a.g2[c] * rs2;
  const float mup = a.meanp[c], rsp = rsqrtf(a.varp[c] + a.epsp), ap = a.gp[c] * rsp, cp = a.bp[c] - mup * ap;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  OWN_FOR(o, {
    X[k] = ok ? (X[k] - mu2) * rs2 : 0.f;  // xhat_2
    s[0] += G[k];
    s[1] += G[k] * X[k];
  })
  block_sum_n<4>(s, red);
  const float m1 = s[0] / n, m2 = s[1] / n;
  const float dg2 = s[1], db2 = s[0];
  s[0] = s[1] = s[2] = s[3] = 0.f;  // dls, dw, sum d p, sum d p * xhat_p
  OWN_FOR(o, {
    const float d = ok ? round_to<T>(k2 * (G[k] - m1 - X[k] * m2) + D[k]) : 0.f;  // d x1 = d x0 (as stored)
    D[k] = d;
    const float pn = ap * P[k] + cp, z = (1.f - wv) * M[k] + wv * pn, dz = d * ls, dpn = dz * wv;
    P[k] = (P[k] - mup) * rsp;  // xhat_p
    s[0] += d * z;
    s[1] += dz * (pn - M[k]);
    s[2] += dpn;
    s[3] += dpn * P[k];
  })
  block_sum_n<4>(s, red);
  const float t1 = s[2] / n, t2 = s[3] / n;
  if (threadIdx.x == 0) {
    a.dg2[c] += dg2;
    a.db2[c] += db2;
    a.dls[c] += s[0];
    a.dgp[c] += s[3];
    a.dbp[c] += s[2];
    atomicAdd(a.dw, s[1]);
  }
  OWN_FOR(o, {
    if (ok) {
      const long q = b * sb + p;
      const float dz = D[k] * ls, dpn = dz * wv;
      stf(dx0 + q, D[k]);
      stf(dm + q, dz * (1.f - wv));
      stf(dp + q, ap * (dpn - t1 - P[k] * t2));
    }
  })
}

// Threads per workgroup for a channel of B images x HW pixels: the FEWEST waves whose threads still own <= maxE elements each.
// These kernels are bound by vector-instruction ISSUE, not by bytes: every thread pays the fixed part of the kernel (reductions,
// scalars, index set-up: several hundred instructions) whatever it owns, so 16 waves holding 2 elements per thread cost four times
// the issue slots of 4 waves holding 8 (measured at 7x7, 512 channels: 19 -> 11 us).  Returns the elements per thread (0: too large).
static inline int own_pick(int B, int HW, int maxE, int* nt) {
  const int Rr = (HW + 63) / 64;
  for (int nw = 4; nw <= 16; nw *= 2) {
    const int need = ((B + nw - 1) / nw) * Rr;
    if (need <= maxE) {
      *nt = nw * 64;
      return need;
    }
  }
  return 0;
}

template <typename T>
static int cfam_mid_launch(const MidArgs& a, bool bwd, hipStream_t stream) {
  int nt = 0;
  const int need = own_pick(a.B, a.HW, 16, &nt);
  if ((long)a.B * a.HW < 2 || need == 0) return CENET_EUNSUPPORTED;
#define CENET_MID(E)                                                                                     \
  {                                                                                                      \
    if (bwd) CENET_LAUNCH((cfam_mid_bwd_kernel<T, E>), dim3(a.C), dim3(nt), stream, a);                  \
    else CENET_LAUNCH((cfam_mid_fwd_kernel<T, E>), dim3(a.C), dim3(nt), stream, a);                      \
  }
  if (need <= 2) CENET_MID(2)
  else if (need <= 4) CENET_MID(4)
  else if (need <= 8) CENET_MID(8)
  else CENET_MID(16)
#undef CENET_MID
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

template <typename T>
static int cfam_mid_fwd_impl(const T* p_raw, const T* m, const T* x0, T* x1, T* y2, const float* gp, const float* bp, float epsp,
                             float* meanp, float* varp, float* rmp, float* rvp, float momp, long* nbtp, const float* w,
                             const float* ls, const float* g2, const float* b2, float eps2, float* mean2, float* var2, float* rm2,
                             float* rv2, float mom2, long* nbt2, int B, int C, int HW, hipStream_t stream) {
  if (!p_raw || !m || !x0 || !x1 || !y2 || !gp || !bp || !meanp || !varp || !w || !ls || !g2 || !b2 || !mean2 || !var2 ||
      B <= 0 || C <= 0 || HW <= 0)
    return CENET_EINVAL;
  if ((((uintptr_t)p_raw | (uintptr_t)m | (uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)y2) & 15) != 0) return CENET_EUNSUPPORTED;
  MidArgs a;
  memset(&a, 0, sizeof(a));
  a.p_raw = p_raw; a.m = m; a.x0 = x0; a.x1 = x1; a.y2 = y2; a.gp = gp; a.bp = bp; a.epsp = epsp; a.meanp = meanp; a.varp = varp;
  a.rmp = rmp; a.rvp = rvp; a.momp = momp; a.nbtp = nbtp; a.w = w; a.ls = ls; a.g2 = g2; a.b2 = b2; a.eps2 = eps2;
  a.mean2 = mean2; a.var2 = var2; a.rm2 = rm2; a.rv2 = rv2; a.mom2 = mom2; a.nbt2 = nbt2; a.B = B; a.C = C; a.HW = HW;
  return cfam_mid_launch<T>(a, false, stream);
}
template <typename T>
static int cfam_mid_bwd_acc_impl(const T* g_y2, const T* g_x1, const T* p_raw, const T* m, const T* x1, T* d_p, T* d_m, T* d_x0,
                                 const float* gp, const float* bp, float epsp, const float* meanp, const float* varp,
                                 const float* w, const float* ls, const float* g2, float eps2, const float* mean2,
                                 const float* var2, float* dgp_acc, float* dbp_acc, float* dw_acc, float* dls_acc, float* dg2_acc,
                                 float* db2_acc, int B, int C, int HW, hipStream_t stream) {
  if (!g_y2 || !p_raw || !m || !x1 || !d_p || !d_m || !d_x0 || !gp || !bp || !meanp || !varp || !w || !ls || !g2 || !mean2 ||
      !var2 || !dgp_acc || !dbp_acc || !dw_acc || !dls_acc || !dg2_acc || !db2_acc || B <= 0 || C <= 0 || HW <= 0)
    return CENET_EINVAL;
  if ((((uintptr_t)g_y2 | (uintptr_t)g_x1 | (uintptr_t)p_raw | (uintptr_t)m | (uintptr_t)x1 | (uintptr_t)d_p | (uintptr_t)d_m |
        (uintptr_t)d_x0) & 15) != 0)
    return CENET_EUNSUPPORTED;
  MidArgs a;
  memset(&a, 0, sizeof(a));
  a.g_y2 = g_y2; a.g_x1 = g_x1; a.p_raw = p_raw; a.m = m; a.x1 = (void*)x1; a.d_p = d_p; a.d_m = d_m; a.d_x0 = d_x0; a.gp = gp;
  a.bp = bp; a.epsp = epsp; a.meanp = (float*)meanp; a.varp = (float*)varp; a.w = w; a.ls = ls; a.g2 = g2; a.eps2 = eps2;
  a.mean2 = (float*)mean2; a.var2 = (float*)var2; a.dgp = dgp_acc; a.dbp = dbp_acc; a.dw = dw_acc; a.dls = dls_acc;
  a.dg2 = dg2_acc; a.db2 = db2_acc; a.B = B; a.C = C; a.HW = HW;
  return cfam_mid_launch<T>(a, true, stream);
}

// ---- dilated depthwise branches of MultiOrderDWConv with their BatchNorm (cfam.py:227-241 over blocks.py:169-177) --------------
//   v[:, j*g + i] = ReLU(BatchNorm_train(DW3x3_{dil_j}(x[:, j*g + i])))   for the NB (<= 3) branches of g channels each,
//   rest = x[:, NB*g :]                                                   (the pooled branch's slice, copied)
// Forward: the conv output goes to v (rounded to the tensor type, as the launch chain stores it), its statistics are taken from
// those stored values, and after a barrier the workgroup normalises its own channel in place.  Backward recomputes the conv
// output from x (no saved copy), writes the conv-output gradient to an fp32 scratch plane set it alone reads back, and adds
// the OTHER gradients of x (g_add: the gate conv's data gradient; g_rest: the pooled branch's) while writing dx: the launch chain
// ran a depthwise kernel, a BatchNorm (2 launches), and backwards BatchNorm (2), depthwise data and weight gradients and a
// slice copy.  The channel's planes are staged in LDS when they fit (flat pointer either way).
struct DwBnArgs {
  const void* x;     // [B, Ctot, H, W] (batch stride sxb); the branch channels start at channel 0
  long sxb;
  void* y;           // forward: v [B, NB*g, H, W] (batch stride syb);  backward: dx [B, Ctot, H, W] (batch stride syb)
  long syb;
  void* rest;        // forward: [B, p, H, W] written;  backward: its gradient, read (batch stride srb)
  long srb;
  const void* g;     // backward: gradient of v (batch stride sgb)
  long sgb;
  const void* gadd;  // backward: other gradient of x [B, Ctot, H, W] (batch stride sab) or null
  long sab;
  const float* w[3];
  float* dw[3];
  int dil[3];
  int G, NB, P;      // channels per branch, branches, rest channels
  const float *gamma, *beta;
  float eps;
  float *mean, *var, *rmean, *rvar;
  float momentum;
  long* nbt;         // NB counters (one per branch) or null
  float *dgamma, *dbeta;
  int B, H, W;
};

// 3x3 taps of pixel (i, j) of one LDS plane (zero outside), their weighted sum
__device__ __forceinline__ float dw_tap9(const float* pl, int H, int W, int i, int j, int dil, const float (&w)[9], float (&tap)[9]) {
  float t = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = i + (ky - 1) * dil;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = j + (kx - 1) * dil;
      const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
      const float v = pl[in ? yy * W + xx : 0];
      tap[ky * 3 + kx] = in ? v : 0.f;
      t += w[ky * 3 + kx] * tap[ky * 3 + kx];
    }
  }
  return t;
}
// p -> (i, j) = (p / W, p % W) without an integer division (exact for p < 2^22)
__device__ __forceinline__ void pix_ij(int p, int W, float invW, int& i, int& j) {
  i = (int)(((float)p + 0.5f) * invW);
  j = p - i * W;
}

constexpr int DWBN_MAXE = 8192;  // elements of a channel over the batch (16 waves x 8 elements x 64 lanes)

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void dwbn_fwd_kernel(DwBnArgs a) {
  __shared__ float xs[DWBN_MAXE];  // (fp32 whatever T is: aligned dword reads, see eucb_stage)
  __shared__ float red[16 * 2];
  const int c = blockIdx.x, H = a.H, W = a.W, HW = H * W;
  const Own o(a.B, HW);
  if (c >= a.NB * a.G) {  // the pooled branch's slice: a copy
    const T* x = (const T*)a.x + (long)c * HW;
    T* r = (T*)a.rest + (long)(c - a.NB * a.G) * HW;
    T V[EPT];
    OWN_FOR(o, { V[k] = x[ok ? (long)b * a.sxb + p : 0]; })
    OWN_FOR(o, { if (ok) r[(long)b * a.srb + p] = V[k]; })
    return;
  }
  const int j = c / a.G, cl = c - j * a.G, dil = a.dil[j];
  const T* x = (const T*)a.x + (long)c * HW;
  {
    float V[EPT];
    OWN_FOR(o, { V[k] = ldf(x + (ok ? (long)b * a.sxb + p : 0)); })
    OWN_FOR(o, { if (ok) xs[b * HW + p] = V[k]; })
  }
  float w[9], tap[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = a.w[j][cl * 9 + k];
  const float gm = a.gamma[c], bt = a.beta[c], invW = 1.f / (float)W;
  __syncthreads();
  float K;  // (shift of the sums of squares, shift_mean: the stored conv output at image 0's first min(HW, 64) pixels)
  {
    const int ms = HW < 64 ? HW : 64;
    int pi, pj;
    pix_ij(o.lane < ms ? o.lane : 0, W, invW, pi, pj);
    K = shift_mean(round_to<T>(dw_tap9(xs, H, W, pi, pj, dil, w, tap)), ms);
  }
  float U[EPT];
  float s[2] = {0.f, 0.f};
  OWN_FOR(o, {
    int pi, pj;
    pix_ij(ok ? p : 0, W, invW, pi, pj);
    U[k] = round_to<T>(dw_tap9(xs + (ok ? b : 0) * HW, H, W, pi, pj, dil, w, tap));  // (rounded as the launch chain stores it)
    const float d = ok ? U[k] - K : 0.f;
    s[0] += d;
    s[1] += d * d;
  })
  block_sum_n<2>(s, red);
  const float n = (float)a.B * (float)HW, m = s[0] / n;
  float var = s[1] / n - m * m;
  if (var < 0.f) var = 0.f;
  const float mu = K + m;
  if (threadIdx.x == 0) {
    a.mean[c] = mu;
    a.var[c] = var;
    if (a.rmean) {
      a.rmean[c] = (1.f - a.momentum) * a.rmean[c] + a.momentum * mu;
      a.rvar[c] = (1.f - a.momentum) * a.rvar[c] + a.momentum * var * (n / (n - 1.f));
    }
    if (a.nbt && cl == 0) a.nbt[j] += 1;
  }
  const float sc = gm * rsqrtf(var + a.eps), sh = bt - mu * sc;
  T* y = (T*)a.y + (long)c * HW;
  OWN_FOR(o, {
    const float v = U[k] * sc + sh;
    if (ok) stf(y + (long)b * a.syb + p, v > 0.f ? v : 0.f);
  })
}

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void dwbn_bwd_kernel(DwBnArgs a) {
  __shared__ float xs[DWBN_MAXE];
  __shared__ float du[DWBN_MAXE];
  __shared__ float red[16 * 9];
  const int c = blockIdx.x, H = a.H, W = a.W, HW = H * W;
  const Own o(a.B, HW);
  T* dx = (T*)a.y + (long)c * HW;
  if (c >= a.NB * a.G) {  // pooled-branch channels: dx = g_rest (+ g_add)
    const T* r = (const T*)a.rest + (long)(c - a.NB * a.G) * HW;
    const T* ga = a.gadd ? (const T*)a.gadd + (long)c * HW : nullptr;
    float V[EPT];
    OWN_FOR(o, {
      V[k] = ldf(r + (ok ? (long)b * a.srb + p : 0));
      if (ga) V[k] += ldf(ga + (ok ? (long)b * a.sab + p : 0));
    })
    OWN_FOR(o, { if (ok) stf(dx + (long)b * a.syb + p, V[k]); })
    return;
  }
  const int j = c / a.G, cl = c - j * a.G, dil = a.dil[j];
  const T* x = (const T*)a.x + (long)c * HW;
  const T* g = (const T*)a.g + (long)c * HW;
  const T* ga = a.gadd ? (const T*)a.gadd + (long)c * HW : nullptr;
  float X[EPT], GY[EPT], GA[EPT];
  OWN_FOR(o, {
    X[k] = ldf(x + (ok ? (long)b * a.sxb + p : 0));
    GY[k] = ldf(g + (ok ? (long)b * a.sgb + p : 0));
    GA[k] = ga ? ldf(ga + (ok ? (long)b * a.sab + p : 0)) : 0.f;
  })
  OWN_FOR(o, { if (ok) xs[b * HW + p] = X[k]; })
  float w[9], tap[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = a.w[j][cl * 9 + k];
  const float mu = a.mean[c], rs = rsqrtf(a.var[c] + a.eps), gm = a.gamma[c], bt = a.beta[c], invW = 1.f / (float)W;
  __syncthreads();
  // pass 1: xhat of the recomputed conv output (rounded as the forward stored it), gradient through the ReLU mask, sums
  float XH[EPT];
  float s[2] = {0.f, 0.f};
  OWN_FOR(o, {
    int pi, pj;
    pix_ij(ok ? p : 0, W, invW, pi, pj);
    XH[k] = (round_to<T>(dw_tap9(xs + (ok ? b : 0) * HW, H, W, pi, pj, dil, w, tap)) - mu) * rs;
    GY[k] = (ok && XH[k] * gm + bt > 0.f) ? GY[k] : 0.f;
    s[0] += GY[k];
    s[1] += GY[k] * XH[k];
  })
  block_sum_n<2>(s, red);
  const float n = (float)a.B * (float)HW, m1 = s[0] / n, m2 = s[1] / n, k0 = gm * rs;
  // pass 2: conv-output gradient -> LDS
  OWN_FOR(o, { if (ok) du[b * HW + p] = k0 * (GY[k] - m1 - XH[k] * m2); })
  __syncthreads();
  // pass 3: one sweep over the 3x3 neighbourhood of the conv-output gradient gives BOTH remaining gradients:
  //   d x(p)  = sum_t w[t] du(p - delta_t)                       (correlation with the flipped taps)
  //   d w[t]  = sum_p du(p) x(p + delta_t) = sum_q x(q) du(q - delta_t)   (the same du(p - delta_t), times the centre value x(p))
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;
  OWN_FOR(o, {
    int pi, pj;
    pix_ij(ok ? p : 0, W, invW, pi, pj);
    const float* dp = du + (ok ? b : 0) * HW;
    const float xc = ok ? X[k] : 0.f;
    float t = GA[k];
_Pragma("unroll")
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = pi - (ky - 1) * dil;
_Pragma("unroll")
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = pj - (kx - 1) * dil;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        float v = dp[in ? yy * W + xx : 0];
        v = in ? v : 0.f;
        t += w[ky * 3 + kx] * v;
        acc[ky * 3 + kx] += xc * v;
      }
    }
    if (ok) stf(dx + (long)b * a.syb + p, t);
  })
  block_sum_n<9>(acc, red);
  if (threadIdx.x < 9) a.dw[j][cl * 9 + threadIdx.x] += acc[threadIdx.x];
  if (threadIdx.x == 9) a.dgamma[c] += s[1];
  if (threadIdx.x == 10) a.dbeta[c] += s[0];
}

// ---- depthwise 3x3 (+bias) + activation without a BatchNorm (cfam.py:150-151: the CFAM Mlp's 4C-channel conv + GELU) ----------
// Same ownership: the channel's planes in LDS (fp32), each thread's elements in registers.  Forward writes only the activated
// tensor (the launch chain also stored the pre-activation for the backward pass); backward recomputes the pre-activation from x,
// puts g * act'(u) into LDS and takes the data gradient, the weight gradient and the bias gradient from ONE sweep over its 3x3
// neighbourhood (the launch chain: activation backward, data-gradient conv, weight-gradient kernel: 3 launches, and at 7x7 —
// planes of 49 pixels, not a multiple of 4 — the scalar fallback kernels: 60 / 51 / 36 us for a 6 MB tensor).
struct DwActArgs {
  const void* x;   // [B, C, H, W] contiguous
  void* y;         // forward: act(conv(x) + bias);  backward: dx
  const void* g;   // backward: gradient of y
  const float *w, *bias;  // [C][9], [C] (may be null)
  float *dw, *db;         // backward: ADDED into (db may be null)
  int act, dil;
  float slope;
  int B, C, H, W;
};

// GELU / GELU' of the bf16 (throughput) instances: erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below a bf16 ulp) with the
// hardware exponential and reciprocal, as the tiled depthwise kernels of dwconv.hip use; the fp32 (parity) instances keep libm's erff.
template <typename T>
__device__ __forceinline__ float dwact_f(int act, float u, float slope) {
  if (sizeof(T) == 2 && act == ACT_GELU) return gelu_as(u);
  return act_fwd(act, u, slope);
}
template <typename T>
__device__ __forceinline__ float dwact_g(int act, float u, float slope) {
  if (sizeof(T) == 2 && act == ACT_GELU) return gelu_as_grad(u);  // Phi(u) + u phi(u): one exponential serves both terms
  return act_bwd(act, u, slope);
}

// Planes in LDS carry a zero border of one pixel when the bordered batch fits (dilation 1: B (H + 2)(W + 2) <= DWBN_MAXE — 14x14
// and 7x7 at B = 32): the nine taps are then unconditional reads at compile-time offsets from one base address, instead of nine
// bounds tests, selects and address computations per element and pass.
__device__ __forceinline__ bool dwact_bordered(const DwActArgs& a) {
  return a.dil == 1 && (long)a.B * (a.H + 2) * (a.W + 2) <= DWBN_MAXE;
}
__device__ __forceinline__ void dwact_zero(float* pl, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) pl[i] = 0.f;
}

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void dwact_fwd_kernel(DwActArgs a) {
  __shared__ float xs[DWBN_MAXE];
  const int c = blockIdx.x, H = a.H, W = a.W, HW = H * W;
  const Own o(a.B, HW);
  const long cb = (long)c * HW, sb = (long)a.C * HW;
  const T* x = (const T*)a.x + cb;
  T* y = (T*)a.y + cb;
  const bool bord = dwact_bordered(a);  // (workgroup-uniform)
  const int PW = W + 2, PS = (H + 2) * PW;
  const float invW = 1.f / (float)W;
  float w[9], tap[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = a.w[c * 9 + k];
  const float bias = a.bias ? a.bias[c] : 0.f;
  if (bord) {
    float V[EPT];
    OWN_FOR(o, { V[k] = ldf(x + (ok ? b * sb + p : 0)); })
    dwact_zero(xs, a.B * PS);
    __syncthreads();
    int base[EPT];  // element (i, j) of image b: xs[base + (ky) * PW + kx] is its tap (ky, kx)
    OWN_FOR(o, {
      int pi, pj;
      pix_ij(ok ? p : 0, W, invW, pi, pj);
      base[k] = (ok ? b : 0) * PS + pi * PW + pj;
      if (ok) xs[base[k] + PW + 1] = V[k];
    })
    __syncthreads();
    OWN_FOR(o, {
      const float* t0 = xs + base[k];
      float u = bias;
_Pragma("unroll")
      for (int ky = 0; ky < 3; ++ky)
_Pragma("unroll")
        for (int kx = 0; kx < 3; ++kx) u += w[ky * 3 + kx] * t0[ky * PW + kx];
      if (ok) stf(y + b * sb + p, dwact_f<T>(a.act, u, a.slope));
    })
    return;
  }
  {
    float V[EPT];
    OWN_FOR(o, { V[k] = ldf(x + (ok ? b * sb + p : 0)); })
    OWN_FOR(o, { if (ok) xs[b * HW + p] = V[k]; })
  }
  __syncthreads();
  OWN_FOR(o, {
    int pi, pj;
    pix_ij(ok ? p : 0, W, invW, pi, pj);
    const float u = dw_tap9(xs + (ok ? b : 0) * HW, H, W, pi, pj, a.dil, w, tap) + bias;
    if (ok) stf(y + b * sb + p, dwact_f<T>(a.act, u, a.slope));
  })
}

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void dwact_bwd_kernel(DwActArgs a) {
  __shared__ float xs[DWBN_MAXE];
  __shared__ float du[DWBN_MAXE];
  __shared__ float red[16 * 10];
  const int c = blockIdx.x, H = a.H, W = a.W, HW = H * W;
  const Own o(a.B, HW);
  const long cb = (long)c * HW, sb = (long)a.C * HW;
  const T* x = (const T*)a.x + cb;
  const T* g = (const T*)a.g + cb;
  T* dx = (T*)a.y + cb;
  const bool bord = dwact_bordered(a);  // (workgroup-uniform)
  const int PW = W + 2, PS = (H + 2) * PW;
  float X[EPT], G[EPT];
  OWN_FOR(o, {
    const long q = ok ? b * sb + p : 0;
    X[k] = ldf(x + q);
    G[k] = ldf(g + q);
  })
  float w[9], tap[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = a.w[c * 9 + k];
  const float bias = a.bias ? a.bias[c] : 0.f, invW = 1.f / (float)W;
  float acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.f;
  if (bord) {
    dwact_zero(xs, a.B * PS);
    dwact_zero(du, a.B * PS);
    __syncthreads();
    int base[EPT];
    OWN_FOR(o, {
      int pi, pj;
      pix_ij(ok ? p : 0, W, invW, pi, pj);
      base[k] = (ok ? b : 0) * PS + pi * PW + pj;
      if (ok) xs[base[k] + PW + 1] = X[k];
    })
    __syncthreads();
    OWN_FOR(o, {
      const float* t0 = xs + base[k];
      float u = bias;
_Pragma("unroll")
      for (int ky = 0; ky < 3; ++ky)
_Pragma("unroll")
        for (int kx = 0; kx < 3; ++kx) u += w[ky * 3 + kx] * t0[ky * PW + kx];
      const float d = ok ? G[k] * dwact_g<T>(a.act, u, a.slope) : 0.f;
      if (ok) du[base[k] + PW + 1] = d;
      acc[9] += d;
    })
    __syncthreads();
    OWN_FOR(o, {
      // dx(q) = sum_t w[t] du(q - d_t); dW[t] = sum_q x(q) du(q - d_t): tap (ky, kx) reads du at offset (2 - ky, 2 - kx) from base
      const float* t0 = du + base[k];
      const float xc = ok ? X[k] : 0.f;
      float t = 0.f;
_Pragma("unroll")
      for (int ky = 0; ky < 3; ++ky)
_Pragma("unroll")
        for (int kx = 0; kx < 3; ++kx) {
          const float v = t0[(2 - ky) * PW + (2 - kx)];
          t += w[ky * 3 + kx] * v;
          acc[ky * 3 + kx] += xc * v;
        }
      if (ok) stf(dx + b * sb + p, t);
    })
  } else {
    OWN_FOR(o, { if (ok) xs[b * HW + p] = X[k]; })
    __syncthreads();
    OWN_FOR(o, {
      int pi, pj;
      pix_ij(ok ? p : 0, W, invW, pi, pj);
      const float u = dw_tap9(xs + (ok ? b : 0) * HW, H, W, pi, pj, a.dil, w, tap) + bias;
      const float d = ok ? G[k] * dwact_g<T>(a.act, u, a.slope) : 0.f;
      if (ok) du[b * HW + p] = d;
      acc[9] += d;
    })
    __syncthreads();
    OWN_FOR(o, {
      int pi, pj;
      pix_ij(ok ? p : 0, W, invW, pi, pj);
      const float* dp = du + (ok ? b : 0) * HW;
      const float xc = ok ? X[k] : 0.f;
      float t = 0.f;
_Pragma("unroll")
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = pi - (ky - 1) * a.dil;
_Pragma("unroll")
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = pj - (kx - 1) * a.dil;
          const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
          float v = dp[in ? yy * W + xx : 0];
          v = in ? v : 0.f;
          t += w[ky * 3 + kx] * v;
          acc[ky * 3 + kx] += xc * v;
        }
      }
      if (ok) stf(dx + b * sb + p, t);
    })
  }
  block_sum_n<10>(acc, red);
  if (threadIdx.x < 9) a.dw[c * 9 + threadIdx.x] += acc[threadIdx.x];
  if (threadIdx.x == 9 && a.db) a.db[c] += acc[9];
}

template <typename T>
static int dwact_launch(const DwActArgs& a, bool bwd, hipStream_t stream) {
  const int HW = a.H * a.W;
  int nt = 0;
  const int need = own_pick(a.B, HW, 8, &nt);
  if ((long)a.B * HW < 1 || (long)a.B * HW > DWBN_MAXE || need == 0 || a.dil < 1) return CENET_EUNSUPPORTED;
#define CENET_DWACT(E)                                                                             \
  {                                                                                                \
    if (bwd) CENET_LAUNCH((dwact_bwd_kernel<T, E>), dim3(a.C), dim3(nt), stream, a);               \
    else CENET_LAUNCH((dwact_fwd_kernel<T, E>), dim3(a.C), dim3(nt), stream, a);                   \
  }
  if (need <= 2) CENET_DWACT(2)
  else if (need <= 4) CENET_DWACT(4)
  else CENET_DWACT(8)
#undef CENET_DWACT
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
template <typename T>
static int dwact_fwd_impl(const T* x, const float* w, const float* bias, T* y, int act, float slope, int dil, int B, int C, int H,
                          int W, hipStream_t stream) {
  if (!x || !w || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return CENET_EINVAL;
  DwActArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.w = w; a.bias = bias; a.act = act; a.slope = slope; a.dil = dil; a.B = B; a.C = C; a.H = H; a.W = W;
  return dwact_launch<T>(a, false, stream);
}
template <typename T>
static int dwact_bwd_acc_impl(const T* g, const T* x, const float* w, const float* bias, T* dx, float* dw_acc, float* dbias_acc,
                              int act, float slope, int dil, int B, int C, int H, int W, hipStream_t stream) {
  if (!g || !x || !w || !dx || !dw_acc || B <= 0 || C <= 0 || H <= 0 || W <= 0) return CENET_EINVAL;
  DwActArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.g = g; a.y = dx; a.w = w; a.bias = bias; a.dw = dw_acc; a.db = dbias_acc; a.act = act; a.slope = slope;
  a.dil = dil; a.B = B; a.C = C; a.H = H; a.W = W;
  return dwact_launch<T>(a, true, stream);
}

template <typename T>
static int dwbn_launch(const DwBnArgs& a, bool bwd, hipStream_t stream) {
  const int HW = a.H * a.W;
  int nt = 0;
  const int need = own_pick(a.B, HW, 8, &nt);
  if ((long)a.B * HW < 2 || (long)a.B * HW > DWBN_MAXE || need == 0 || a.NB < 1 || a.NB > 3 || a.G < 1 || a.P < 0)
    return CENET_EUNSUPPORTED;
  const int grid = a.NB * a.G + a.P;
#define CENET_DWBN(E)                                                                                \
  {                                                                                                  \
    if (bwd) CENET_LAUNCH((dwbn_bwd_kernel<T, E>), dim3(grid), dim3(nt), stream, a);                 \
    else CENET_LAUNCH((dwbn_fwd_kernel<T, E>), dim3(grid), dim3(nt), stream, a);                     \
  }
  if (need <= 2) CENET_DWBN(2)
  else if (need <= 4) CENET_DWBN(4)
  else CENET_DWBN(8)
#undef CENET_DWBN
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

template <typename T>
static int dwbn_fwd_impl(const T* x, long sxb, const float* const* w, const int* dil, int nb, int g, int p, T* v, long svb, T* rest,
                         long srb, const float* gamma, const float* beta, float eps, float* mean, float* var, float* rmean,
                         float* rvar, float momentum, long* nbt, int B, int H, int W, hipStream_t stream) {
  if (!x || !w || !dil || !v || !gamma || !beta || !mean || !var || (p > 0 && !rest) || B <= 0 || H <= 0 || W <= 0 || nb < 1 ||
      nb > 3)
    return CENET_EINVAL;
  DwBnArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.sxb = sxb; a.y = v; a.syb = svb; a.rest = rest; a.srb = srb;
  for (int j = 0; j < nb; ++j) {
    if (!w[j] || dil[j] < 1) return CENET_EINVAL;
    a.w[j] = w[j];
    a.dil[j] = dil[j];
  }
  a.G = g; a.NB = nb; a.P = p; a.gamma = gamma; a.beta = beta; a.eps = eps; a.mean = mean; a.var = var; a.rmean = rmean;
  a.rvar = rvar; a.momentum = momentum; a.nbt = nbt; a.B = B; a.H = H; a.W = W;
  return dwbn_launch<T>(a, false, stream);
}

template <typename T>
static int dwbn_bwd_acc_impl(const T* g_v, long sgb, const T* g_rest, long srb, const T* g_add, long sab, const T* x, long sxb,
                             const float* const* w, const int* dil, int nb, int g, int p, const float* gamma, const float* beta,
                             float eps, const float* mean, const float* var, T* dx, long sdb, float* const* dw_acc,
                             float* dgamma_acc, float* dbeta_acc, int B, int H, int W, hipStream_t stream) {
  if (!g_v || !x || !w || !dil || !gamma || !beta || !mean || !var || !dx || !dw_acc || !dgamma_acc || !dbeta_acc ||
      (p > 0 && !g_rest) || B <= 0 || H <= 0 || W <= 0 || nb < 1 || nb > 3)
    return CENET_EINVAL;
  DwBnArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.sxb = sxb; a.y = dx; a.syb = sdb; a.rest = (void*)g_rest; a.srb = srb; a.g = g_v; a.sgb = sgb; a.gadd = g_add;
  a.sab = sab;
  for (int j = 0; j < nb; ++j) {
    if (!w[j] || !dw_acc[j] || dil[j] < 1) return CENET_EINVAL;
    a.w[j] = w[j];
    a.dw[j] = dw_acc[j];
    a.dil[j] = dil[j];
  }
  a.G = g; a.NB = nb; a.P = p; a.gamma = gamma; a.beta = beta; a.eps = eps; a.mean = (float*)mean; a.var = (float*)var;
  a.dgamma = dgamma_acc; a.dbeta = dbeta_acc; a.B = B; a.H = H; a.W = W;
  return dwbn_launch<T>(a, true, stream);
}

// ---- CFAM front: norm1 + CCU (cfam.py:366 over cfam.py:251-264) -------------------------------------------------------------------
//   y1 = BatchNorm_1(x0)                                     (stored: the MCA shortcut and the CCU's input)
//   u_b = [max, mean, std_biased] of y1[b] over the plane;  z_b = fc2 . relu(fc1 u_b);  zn = BatchNorm1d_train(z) over the batch
//   (skipped for a batch of one);  xs = y1 * sigmoid(zn_b)
// Workgroup = channel; per-image statistics are taken by one WAVE per image (shuffle trees, no atomics, fixed order).  Forward
// 5 - 6 launches -> 1; backward (gate reduce, BatchNorm1d backward, CCU apply, BatchNorm backward: 5 launches) -> 1.
#define CCU_MAXB 256
struct FrontArgs {
  const void* x0;            // [B, C, HW]
  void *y1, *xs;             // forward outputs
  const void *g_xs, *g_y1, *g_tap;  // backward inputs (g_y1 / g_tap may be null)
  void* dx0;                 // backward output
  const float *g1, *b1;      // norm1
  float eps1;
  float *mean1, *var1, *rm1, *rv1;
  float mom1;
  long* nbt1;
  const float *fc1, *fc2;    // [C][3][3], [C][3]
  const float *gd, *bd;      // BatchNorm1d (null: no BatchNorm1d — batch of one)
  float epsd;
  float *meand, *vard, *rmd, *rvd;
  float momd;
  long* nbtd;
  float* u;                  // [B, C, 3]
  int* amax;                 // [B, C]
  float *z, *zn;             // [B, C]
  float *dg1, *db1, *dfc1, *dfc2, *dgd, *dbd;  // backward: ADDED into
  int B, C, HW;
};

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void cfam_front_fwd_kernel(FrontArgs a) {
  __shared__ float red[16 * 2];
  __shared__ float zs[CCU_MAXB];
  const int c = blockIdx.x, C = a.C, HW = a.HW, B = a.B;
  const Own o(B, HW);
  const long cb = (long)c * HW, sb = (long)C * HW;
  const T* x = (const T*)a.x0 + cb;
  T *y1 = (T*)a.y1 + cb, *xs = (T*)a.xs + cb;
  float X[EPT];
  OWN_FOR(o, { X[k] = ldf(x + (ok ? b * sb + p : 0)); })
  const int ms = HW < 64 ? HW : 64;
  const float K = shift_mean(ldf(x + (o.lane < ms ? o.lane : 0)), ms);  // (image 0's first min(HW, 64) elements)
  const float g1 = a.g1[c], b1 = a.b1[c];
  float w1[9], w2[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) w1[k] = a.fc1[c * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w2[k] = a.fc2[c * 3 + k];
  const float gd = a.gd ? a.gd[c] : 1.f, bd = a.gd ? a.bd[c] : 0.f;
  float s[2] = {0.f, 0.f};
  OWN_FOR(o, {
    const float d = ok ? X[k] - K : 0.f;
    s[0] += d;
    s[1] += d * d;
  })
  block_sum_n<2>(s, red);
  const float n = (float)B * (float)HW, m = s[0] / n;
  float var = s[1] / n - m * m;
  if (var < 0.f) var = 0.f;
  const float mu = K + m;
  if (threadIdx.x == 0) bn_publish(a.mean1, a.var1, a.rm1, a.rv1, a.mom1, a.nbt1, c, mu, var, n);
  const float a1 = g1 * rsqrtf(var + a.eps1), c1 = b1 - mu * a1;
  // y1 (as stored) and the per-image statistics of the stored values: an image's pixels all sit in ONE wave (rows r of a slot)
  float q1 = 0.f, q2 = 0.f, mx = -3.4e38f, Kb = 0.f;
  int mi = 0;
  OWN_FOR(o, {
    X[k] = round_to<T>(a1 * X[k] + c1);
    if (r__ == 0) {
      q1 = q2 = 0.f;
      mx = -3.4e38f;
      mi = 0;
      Kb = shift_mean(X[k], ms);  // (the image's first min(HW, 64) pixels: row 0 of the slot)
    }
    if (ok) {
      const float d = X[k] - Kb;
      q1 += d;
      q2 += d * d;
      if (X[k] > mx) {
        mx = X[k];
        mi = p;
      }
    }
    if (r__ == o.Rr - 1 && b < B) {  // (wave-uniform: b does not depend on the lane)
      q1 = wave_sum_dpp(q1);
      q2 = wave_sum_dpp(q2);
      const float wmx = wave_max_dpp(mx);
      mi = wave_min_i_dpp(mx == wmx ? mi : 0x7fffffff);  // (ties: the smallest pixel index, as aten::max)
      mx = wmx;
      if (o.lane == 0) {
        const float mb = q1 / HW;
        float vb = q2 / HW - mb * mb;
        if (vb < 0.f) vb = 0.f;
        const float mean = Kb + mb, sd = sqrtf(vb);
        const long bc = (long)b * C + c;
        a.u[bc * 3 + 0] = mx;
        a.u[bc * 3 + 1] = mean;
        a.u[bc * 3 + 2] = sd;
        a.amax[bc] = mi;
        float zz = 0.f;
_Pragma("unroll")
        for (int j = 0; j < 3; ++j) {
          const float hdn = w1[j * 3 + 0] * mx + w1[j * 3 + 1] * mean + w1[j * 3 + 2] * sd;
          if (hdn > 0.f) zz += w2[j] * hdn;
        }
        a.z[bc] = zz;
        zs[b] = zz;
      }
    }
  })
  __syncthreads();
  // BatchNorm1d over the batch (one value per image): every thread computes the same few sums
  float ad = 1.f, cd = 0.f;
  if (a.gd) {
    float t1 = 0.f;
    for (int b = 0; b < B; ++b) t1 += zs[b];
    const float mz = t1 / B;
    float t2 = 0.f;
    for (int b = 0; b < B; ++b) t2 += (zs[b] - mz) * (zs[b] - mz);
    const float vz = t2 / B;
    if (threadIdx.x == 0) bn_publish(a.meand, a.vard, a.rmd, a.rvd, a.momd, a.nbtd, c, mz, vz, (float)B);
    ad = gd * rsqrtf(vz + a.epsd);
    cd = bd - mz * ad;
  }
  float gate = 0.f;
  OWN_FOR(o, {
    if (r__ == 0) {
      const float zn = ad * zs[b < B ? b : 0] + cd;
      gate = sigmoid_f(zn);
      if (o.lane == 0 && b < B) a.zn[(long)b * C + c] = zn;
    }
    if (ok) {
      stf(y1 + b * sb + p, X[k]);
      stf(xs + b * sb + p, X[k] * gate);
    }
  })
}

// MAXT: the launch's thread count is at most this (512: eight waves, 256 registers per lane — the 16-element instance at the
// 1024-thread cap of 128 spilled 296 bytes per lane)
template <typename T, int EPT, int MAXT>
__global__ __launch_bounds__(MAXT) void cfam_front_bwd_kernel(FrontArgs a) {
  __shared__ float red[16 * 2];
  __shared__ float dzn_s[CCU_MAXB], gate_s[CCU_MAXB], dmean_s[CCU_MAXB], dstd_s[CCU_MAXB], dmax_s[CCU_MAXB], mean_s[CCU_MAXB];
  __shared__ int am_s[CCU_MAXB];
  const int c = blockIdx.x, C = a.C, HW = a.HW, B = a.B;
  const Own o(B, HW);
  const long cb = (long)c * HW, sb = (long)C * HW;
  const T* x = (const T*)a.x0 + cb;
  const T* gx = (const T*)a.g_xs + cb;
  const T* gy = a.g_y1 ? (const T*)a.g_y1 + cb : gx;   // (absent: any valid address, the value is dropped)
  const T* gt = a.g_tap ? (const T*)a.g_tap + cb : gx;
  T* dx = (T*)a.dx0 + cb;
  float X[EPT], GX[EPT], GY[EPT], GT[EPT];
  OWN_FOR(o, {
    const long q = ok ? b * sb + p : 0;
    X[k] = ldf(x + q);
    GX[k] = ldf(gx + q);
    GY[k] = ldf(gy + q);
    GT[k] = ldf(gt + q);
  })
  const float mu = a.mean1[c], rs = rsqrtf(a.var1[c] + a.eps1), a1 = a.g1[c] * rs, c1 = a.b1[c] - mu * a1;
  float w1[9], w2[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) w1[k] = a.fc1[c * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w2[k] = a.fc2[c * 3 + k];
  float kd = 1.f, mz = 0.f, rsd = 1.f;
  if (a.gd) {
    mz = a.meand[c];
    rsd = rsqrtf(a.vard[c] + a.epsd);
    kd = a.gd[c] * rsd;
  }
  // the wave-0 lanes own images for the tiny per-image algebra: their saved statistics now, with everything else
  float zb[(CCU_MAXB + 63) / 64], ub[(CCU_MAXB + 63) / 64][3];
  int ab[(CCU_MAXB + 63) / 64];
  if (o.wave == 0) {
#pragma unroll
    for (int i = 0; i < (CCU_MAXB + 63) / 64; ++i) {
      const int b = i * 64 + o.lane;
      const long bc = (long)(b < B ? b : 0) * C + c;
      zb[i] = a.z[bc];
      ub[i][0] = a.u[bc * 3];
      ub[i][1] = a.u[bc * 3 + 1];
      ub[i][2] = a.u[bc * 3 + 2];
      ab[i] = a.amax[bc];
    }
  }
  float ZN[EPT];  // zn of the element's image (one value per slot, kept per element for simplicity of the unrolled loops)
  OWN_FOR(o, { ZN[k] = a.zn[(long)(b < B ? b : 0) * C + c]; })
  // d gate_b = sum_p g_xs * y1 (the image's pixels sit in one wave) -> d zn_b
  float q = 0.f;
  OWN_FOR(o, {
    if (!ok) GX[k] = 0.f;
    if (!ok || !a.g_y1) GY[k] = 0.f;
    if (!ok || !a.g_tap) GT[k] = 0.f;
    if (r__ == 0) q = 0.f;
    q += GX[k] * round_to<T>(a1 * X[k] + c1);  // (y1 as the forward stored it)
    if (r__ == o.Rr - 1 && b < B) {
      q = wave_sum_dpp(q);
      if (o.lane == 0) {
        const float sg = sigmoid_f(ZN[k]);
        gate_s[b] = sg;
        dzn_s[b] = q * sg * (1.f - sg);
      }
    }
  })
  __syncthreads();
  // BatchNorm1d backward over the batch, then the gate MLP backward per image (lane = image in wave 0)
  if (o.wave == 0) {
    float md1 = 0.f, md2 = 0.f;
    if (a.gd) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int i = 0; i < (CCU_MAXB + 63) / 64; ++i) {
        const int b = i * 64 + o.lane;
        if (b < B) {
          t1 += dzn_s[b];
          t2 += dzn_s[b] * ((zb[i] - mz) * rsd);
        }
      }
      t1 = wave_sum_dpp(t1);
      t2 = wave_sum_dpp(t2);
      md1 = t1 / B;
      md2 = t2 / B;
      if (o.lane == 0) {
        a.dgd[c] += t2;
        a.dbd[c] += t1;
      }
    }
    float f1[9], f2[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) f1[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) f2[k] = 0.f;
#pragma unroll
    for (int i = 0; i < (CCU_MAXB + 63) / 64; ++i) {
      const int b = i * 64 + o.lane;
      if (b < B) {
        const float gz = a.gd ? kd * (dzn_s[b] - md1 - (zb[i] - mz) * rsd * md2) : dzn_s[b];
        const float mxv = ub[i][0], mean = ub[i][1], sd = ub[i][2];
        float du[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float hdn = w1[j * 3] * mxv + w1[j * 3 + 1] * mean + w1[j * 3 + 2] * sd;
          if (hdn > 0.f) {
            f2[j] += gz * hdn;
            const float gh = gz * w2[j];
            f1[j * 3 + 0] += gh * mxv;
            f1[j * 3 + 1] += gh * mean;
            f1[j * 3 + 2] += gh * sd;
            du[0] += gh * w1[j * 3];
            du[1] += gh * w1[j * 3 + 1];
            du[2] += gh * w1[j * 3 + 2];
          }
        }
        dmax_s[b] = du[0];
        dmean_s[b] = du[1] / HW;
        dstd_s[b] = sd > 0.f ? du[2] / (HW * sd) : 0.f;  // (aten::std_backward masks the 0/0 of a constant plane to 0)
        mean_s[b] = mean;
        am_s[b] = ab[i];
      }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) f1[k] = wave_sum_dpp(f1[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) f2[k] = wave_sum_dpp(f2[k]);
    if (o.lane < 9) {
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) v = o.lane == k ? f1[k] : v;
      a.dfc1[c * 9 + o.lane] += v;
    } else if (o.lane < 12) {
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) v = o.lane - 9 == k ? f2[k] : v;
      a.dfc2[c * 3 + o.lane - 9] += v;
    }
  }
  __syncthreads();
  // d y1 per element (in GX), xhat_1 (in X), BatchNorm_1 sums
  float s[2] = {0.f, 0.f};
  float cg = 0.f, cm = 0.f, cs = 0.f, cmean = 0.f, cmax = 0.f;
  int cam = -1;
  OWN_FOR(o, {
    if (r__ == 0) {
      const int bb = b < B ? b : 0;
      cg = gate_s[bb], cm = dmean_s[bb], cs = dstd_s[bb], cmean = mean_s[bb], cmax = dmax_s[bb], cam = am_s[bb];
    }
    float d = GX[k] * cg + cm + cs * (round_to<T>(a1 * X[k] + c1) - cmean) + GY[k];
    if (p == cam) d += cmax;
    if (!ok) d = 0.f;
    GX[k] = d;
    X[k] = ok ? (X[k] - mu) * rs : 0.f;  // xhat_1
    s[0] += d;
    s[1] += d * X[k];
  })
  block_sum_n<2>(s, red);
  const float n = (float)B * (float)HW, m1 = s[0] / n, m2 = s[1] / n;
  if (threadIdx.x == 0) {
    a.dg1[c] += s[1];
    a.db1[c] += s[0];
  }
  OWN_FOR(o, {
    if (ok) stf(dx + b * sb + p, a1 * (GX[k] - m1 - X[k] * m2) + GT[k]);
  })
}

template <typename T>
static int cfam_front_launch(const FrontArgs& a, bool bwd, hipStream_t stream) {
  int nt = 0;
  const int need = own_pick(a.B, a.HW, 16, &nt);
  if ((long)a.B * a.HW < 2 || need == 0 || a.B > CCU_MAXB) return CENET_EUNSUPPORTED;
#define CENET_FRONT(E)                                                                                   \
  {                                                                                                      \
    if (bwd && nt <= 512) CENET_LAUNCH((cfam_front_bwd_kernel<T, E, 512>), dim3(a.C), dim3(nt), stream, a); \
    else if (bwd) CENET_LAUNCH((cfam_front_bwd_kernel<T, E, 1024>), dim3(a.C), dim3(nt), stream, a);     \
    else CENET_LAUNCH((cfam_front_fwd_kernel<T, E>), dim3(a.C), dim3(nt), stream, a);                    \
  }
  if (need <= 2) CENET_FRONT(2)
  else if (need <= 4) CENET_FRONT(4)
  else if (need <= 8) CENET_FRONT(8)
  else CENET_FRONT(16)
#undef CENET_FRONT
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

template <typename T>
static int cfam_front_fwd_impl(const T* x0, T* y1, T* xs, const float* gamma1, const float* beta1, float eps1, float* mean1,
                               float* var1, float* rmean1, float* rvar1, float mom1, long* nbt1, const float* fc1, const float* fc2,
                               const float* gamma_d, const float* beta_d, float eps_d, float* mean_d, float* var_d, float* rmean_d,
                               float* rvar_d, float mom_d, long* nbt_d, float* u, int* amax, float* z, float* zn, int B, int C,
                               int HW, hipStream_t stream) {
  if (!x0 || !y1 || !xs || !gamma1 || !beta1 || !mean1 || !var1 || !fc1 || !fc2 || !u || !amax || !z || !zn || B <= 0 || C <= 0 ||
      HW <= 0 || (gamma_d && (!beta_d || !mean_d || !var_d)))
    return CENET_EINVAL;
  FrontArgs a;
  memset(&a, 0, sizeof(a));
  a.x0 = x0; a.y1 = y1; a.xs = xs; a.g1 = gamma1; a.b1 = beta1; a.eps1 = eps1; a.mean1 = mean1; a.var1 = var1; a.rm1 = rmean1;
  a.rv1 = rvar1; a.mom1 = mom1; a.nbt1 = nbt1; a.fc1 = fc1; a.fc2 = fc2; a.gd = gamma_d; a.bd = beta_d; a.epsd = eps_d;
  a.meand = mean_d; a.vard = var_d; a.rmd = rmean_d; a.rvd = rvar_d; a.momd = mom_d; a.nbtd = nbt_d; a.u = u; a.amax = amax;
  a.z = z; a.zn = zn; a.B = B; a.C = C; a.HW = HW;
  return cfam_front_launch<T>(a, false, stream);
}
template <typename T>
static int cfam_front_bwd_acc_impl(const T* g_xs, const T* g_y1, const T* g_tap, const T* x0, T* dx0, const float* gamma1,
                                   const float* beta1, float eps1, const float* mean1, const float* var1, const float* fc1,
                                   const float* fc2, const float* gamma_d, float eps_d, const float* mean_d, const float* var_d,
                                   const float* u, const int* amax, const float* z, const float* zn, float* dgamma1_acc,
                                   float* dbeta1_acc, float* dfc1_acc, float* dfc2_acc, float* dgamma_d_acc, float* dbeta_d_acc,
                                   int B, int C, int HW, hipStream_t stream) {
  if (!g_xs || !x0 || !dx0 || !gamma1 || !beta1 || !mean1 || !var1 || !fc1 || !fc2 || !u || !amax || !z || !zn || !dgamma1_acc ||
      !dbeta1_acc || !dfc1_acc || !dfc2_acc || B <= 0 || C <= 0 || HW <= 0 ||
      (gamma_d && (!mean_d || !var_d || !dgamma_d_acc || !dbeta_d_acc)))
    return CENET_EINVAL;
  FrontArgs a;
  memset(&a, 0, sizeof(a));
  a.g_xs = g_xs; a.g_y1 = g_y1; a.g_tap = g_tap; a.x0 = x0; a.dx0 = dx0; a.g1 = gamma1; a.b1 = beta1; a.eps1 = eps1;
  a.mean1 = (float*)mean1; a.var1 = (float*)var1; a.fc1 = fc1; a.fc2 = fc2; a.gd = gamma_d; a.epsd = eps_d;
  a.meand = (float*)mean_d; a.vard = (float*)var_d; a.u = (float*)u; a.amax = (int*)amax; a.z = (float*)z; a.zn = (float*)zn;
  a.dg1 = dgamma1_acc; a.db1 = dbeta1_acc; a.dfc1 = dfc1_acc; a.dfc2 = dfc2_acc; a.dgd = dgamma_d_acc; a.dbd = dbeta_d_acc;
  a.B = B; a.C = C; a.HW = HW;
  return cfam_front_launch<T>(a, true, stream);
}

// ---- pooled branch of MultiOrderDWConv (cfam.py:212-218,231-232) ------------------------------------------------------------------
//   pooled = AdaptiveAvgPool_7x7(x)   t = Conv1x1_{p x p}(pooled)   z = LeakyReLU_{0.01}(BatchNorm_train(t))
//   y = bilinear(bilinear(z, x7, align_corners) -> 49 x 49, size (H, W), align_corners = False)
// On [B, p, 7, 7] values (p = C / 16 = 4 ... 32) the launch chain — pool, conv, BatchNorm (2), two resamplings — ran six launches
// of pure fill / drain latency each way at EVERY decoder level.  Here: two launches each way.
//   mix   workgroup = image:   pool the image's p planes, mix the channels                      -> pooled, t  [B, p, 49] fp32
//   up    workgroup = channel: batch statistics of t[:, c], normalise, LeakyReLU, and BOTH resamplings as one separable linear map
//         y[b] = RH z[b] RW^T with RH = R_{49 -> H} R_{7 -> 49} ([H, 7], built on the host with the kernels' own coordinate rule)
// and mirrored backwards (up: RH^T g RW, LeakyReLU', BatchNorm backward, the conv weight gradient's row c; mix: W^T, un-pool).
#define POOLB 7
#define POOLK 49
struct PoolArgs {
  const void* x;      // mix fwd: [B, p, H, W] slice (batch stride sxb) ; up bwd: gradient of y (batch stride sxb)
  long sxb;
  void* y;            // up fwd: y slice (batch stride syb) ; mix bwd: dx [B, p, H, W] (batch stride syb)
  long syb;
  float *pooled, *t;  // [B, p, 49]
  float* dt;          // [B, p, 49]
  const float* wc;    // [p, p]
  float* dwc;         // ADDED into
  const float *gamma, *beta, *RH, *RW;  // RH [H, 7], RW [W, 7]
  float eps, slope;
  float *mean, *var, *rmean, *rvar;
  float momentum;
  long* nbt;
  float *dgamma, *dbeta;
  int B, P, H, W;
};
__device__ __forceinline__ int pool_lo(int o, int in) { return (o * in) / POOLB; }
__device__ __forceinline__ int pool_hi(int o, int in) { return ((o + 1) * in + POOLB - 1) / POOLB; }

template <typename T>
__global__ __launch_bounds__(256) void pool_mix_fwd_kernel(PoolArgs a) {
  __shared__ float pl[32 * POOLK];
  const int b = blockIdx.x, P = a.P, H = a.H, W = a.W;
  const T* x = (const T*)a.x + (long)b * a.sxb;
  for (int e = threadIdx.x; e < P * POOLK; e += 256) {
    const int ci = e / POOLK, k = e - ci * POOLK, oy = k / POOLB, ox = k - oy * POOLB;
    const int ys = pool_lo(oy, H), ye = pool_hi(oy, H), xs = pool_lo(ox, W), xe = pool_hi(ox, W);
    const T* xp = x + (long)ci * H * W;
    float sm = 0.f;
    for (int iy = ys; iy < ye; ++iy)
      for (int ix = xs; ix < xe; ++ix) sm += ldf(xp + iy * W + ix);
    sm /= (float)((ye - ys) * (xe - xs));
    pl[e] = sm;
    a.pooled[(long)b * P * POOLK + e] = sm;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < P * POOLK; e += 256) {
    const int co = e / POOLK, k = e - co * POOLK;
    float sm = 0.f;
    for (int ci = 0; ci < P; ++ci) sm += a.wc[co * P + ci] * pl[ci * POOLK + k];
    a.t[(long)b * P * POOLK + e] = sm;
  }
}

// mix, backward: workgroup = (image b, input channel ci) — the un-pooling writes H * W values per plane and is what takes the time at
// the large levels (one workgroup per IMAGE left 32 workgroups walking 12 K outputs each)
template <typename T>
__global__ __launch_bounds__(256) void pool_mix_bwd_kernel(PoolArgs a) {
  __shared__ float dpl[POOLK];
  const int b = blockIdx.x, ci = blockIdx.y, P = a.P, H = a.H, W = a.W, HW = H * W;
  if (threadIdx.x < POOLK) {
    const int k = threadIdx.x, oy = k / POOLB, ox = k - oy * POOLB;
    float sm = 0.f;
    for (int co = 0; co < P; ++co) sm += a.wc[co * P + ci] * a.dt[((long)b * P + co) * POOLK + k];
    dpl[k] = sm / (float)((pool_hi(oy, H) - pool_lo(oy, H)) * (pool_hi(ox, W) - pool_lo(ox, W)));
  }
  __syncthreads();
  T* dx = (T*)a.y + (long)b * a.syb + (long)ci * HW;
  for (int q = threadIdx.x; q < HW; q += 256) {
    const int iy = q / W, ix = q - iy * W;
    // the bins that hold row iy: pool_hi(oy) > iy <=> oy >= floor(7 iy / H), pool_lo(oy) <= iy <=> oy <= ceil(7 (iy + 1) / H) - 1
    // (two neighbours where H >= 7; below 7 the windows repeat pixels and a row sits in up to ceil(7 / H) + 1 bins)
    const int oy0 = (iy * POOLB) / H, oy1 = (POOLB * (iy + 1) + H - 1) / H - 1;
    const int ox0 = (ix * POOLB) / W, ox1 = (POOLB * (ix + 1) + W - 1) / W - 1;
    float sm = 0.f;
    for (int oy = oy0; oy <= oy1 && oy < POOLB; ++oy) {
      if (iy < pool_lo(oy, H) || iy >= pool_hi(oy, H)) continue;
      for (int ox = ox0; ox <= ox1 && ox < POOLB; ++ox)
        if (ix >= pool_lo(ox, W) && ix < pool_hi(ox, W)) sm += dpl[oy * POOLB + ox];
    }
    stf(dx + q, sm);
  }
}

// up, forward: workgroup = (channel c, image b).  The batch statistics of t[:, c] (B * 49 values) are recomputed by each of the
// channel's B workgroups — cheaper than a launch of their own — and image 0's workgroup publishes them.
template <typename T>
__global__ __launch_bounds__(256) void pool_up_fwd_kernel(PoolArgs a) {
  __shared__ float red[16 * 2];
  __shared__ float z[POOLK];
  __shared__ float tmp[POOLB * 64];
  const int c = blockIdx.x, b = blockIdx.y, B = a.B, P = a.P, H = a.H, W = a.W, n = B * POOLK;
  float s[2] = {0.f, 0.f};
  const float K = shift_mean(a.t[(long)c * POOLK + (((int)threadIdx.x & 63) < POOLK ? ((int)threadIdx.x & 63) : 0)], POOLK);  // (image 0's plane)
  for (int e = threadIdx.x; e < n; e += 256) {
    const int bb = e / POOLK, k = e - bb * POOLK;
    const float v = a.t[((long)bb * P + c) * POOLK + k] - K;
    s[0] += v;
    s[1] += v * v;
  }
  block_sum_n<2>(s, red);
  const float m = s[0] / n;
  float var = s[1] / n - m * m;
  if (var < 0.f) var = 0.f;
  const float mu = K + m;
  if (threadIdx.x == 0 && b == 0) {
    a.mean[c] = mu;
    a.var[c] = var;
    if (a.rmean) {
      a.rmean[c] = (1.f - a.momentum) * a.rmean[c] + a.momentum * mu;
      a.rvar[c] = (1.f - a.momentum) * a.rvar[c] + a.momentum * var * ((float)n / ((float)n - 1.f));
    }
    if (a.nbt && c == 0) a.nbt[0] += 1;
  }
  const float sc = a.gamma[c] * rsqrtf(var + a.eps), sh = a.beta[c] - mu * sc;
  if (threadIdx.x < POOLK) {
    const float v = a.t[((long)b * P + c) * POOLK + threadIdx.x] * sc + sh;
    z[threadIdx.x] = v > 0.f ? v : v * a.slope;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < POOLB * W; e += 256) {  // tmp[i][x] = sum_j z[i][j] RW[x][j]
    const int i = e / W, xx = e - i * W;
    float sm = 0.f;
#pragma unroll
    for (int j = 0; j < POOLB; ++j) sm += z[i * POOLB + j] * a.RW[xx * POOLB + j];
    tmp[i * 64 + xx] = sm;
  }
  __syncthreads();
  T* y = (T*)a.y + (long)b * a.syb + (long)c * H * W;
  for (int e = threadIdx.x; e < H * W; e += 256) {      // y[y][x] = sum_i RH[y][i] tmp[i][x]
    const int yy = e / W, xx = e - yy * W;
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < POOLB; ++i) sm += a.RH[yy * POOLB + i] * tmp[i * 64 + xx];
    stf(y + e, sm);
  }
}

// up, backward, per (channel, image): dzr[b, c] = RH^T g[b, c] RW   (the gradient plane goes through LDS: every element is read 7 times)
template <typename T>
__global__ __launch_bounds__(256) void pool_up_bwd_resample_kernel(PoolArgs a) {
  __shared__ float gl[64 * 64];
  __shared__ float tmp[POOLB * 64];
  const int c = blockIdx.x, b = blockIdx.y, P = a.P, H = a.H, W = a.W;
  const T* g = (const T*)a.x + (long)b * a.sxb + (long)c * H * W;
  for (int e0 = threadIdx.x; e0 < H * W; e0 += 4 * 256) {  // four loads in flight per thread
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ldf(g + (e0 + u * 256 < H * W ? e0 + u * 256 : 0));
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + u * 256 < H * W) gl[e0 + u * 256] = v[u];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < POOLB * W; e += 256) {  // tmp[i][x] = sum_y RH[y][i] g[y][x]
    const int i = e / W, xx = e - i * W;
    float sm = 0.f;
    for (int yy = 0; yy < H; ++yy) sm += a.RH[yy * POOLB + i] * gl[yy * W + xx];
    tmp[i * 64 + xx] = sm;
  }
  __syncthreads();
  if (threadIdx.x < POOLK) {                            // dzr[i][j] = sum_x tmp[i][x] RW[x][j]
    const int i = threadIdx.x / POOLB, j = threadIdx.x - i * POOLB;
    float sm = 0.f;
    for (int xx = 0; xx < W; ++xx) sm += tmp[i * 64 + xx] * a.RW[xx * POOLB + j];
    a.dt[((long)b * P + c) * POOLK + threadIdx.x] = sm;
  }
}

// up, backward, per channel: LeakyReLU', BatchNorm backward over the batch (in place in dt), row c of the conv weight gradient
__global__ __launch_bounds__(1024) void pool_up_bwd_bn_kernel(PoolArgs a) {
  __shared__ float red[16 * 2];
  __shared__ float z[64 * POOLK];  // B <= 64
  const int c = blockIdx.x, B = a.B, P = a.P, n = B * POOLK;
  const float mu = a.mean[c], rs = rsqrtf(a.var[c] + a.eps), gm = a.gamma[c], bt = a.beta[c];
  float s[2] = {0.f, 0.f};
  for (int e = threadIdx.x; e < n; e += 1024) {
    const int b = e / POOLK, k = e - b * POOLK;
    const long q = ((long)b * P + c) * POOLK + k;
    const float xh = (a.t[q] - mu) * rs, d = a.dt[q];
    const float gy = (xh * gm + bt > 0.f) ? d : d * a.slope;
    z[e] = gy;
    s[0] += gy;
    s[1] += gy * xh;
  }
  block_sum_n<2>(s, red);
  const float m1 = s[0] / n, m2 = s[1] / n, k0 = gm * rs;
  if (threadIdx.x == 0) {
    a.dgamma[c] += s[1];
    a.dbeta[c] += s[0];
  }
  for (int e = threadIdx.x; e < n; e += 1024) {
    const int b = e / POOLK, k = e - b * POOLK;
    const long q = ((long)b * P + c) * POOLK + k;
    const float d = k0 * (z[e] - m1 - (a.t[q] - mu) * rs * m2);
    z[e] = d;
    a.dt[q] = d;
  }
  __syncthreads();
  // dW[c][ci] = sum_{b, k} dt[b, c, k] pooled[b, ci, k]   (one wave per input channel in turn)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int ci = wave; ci < P; ci += 16) {
    float sm = 0.f;
    for (int e0 = lane; e0 < n; e0 += 8 * 64) {  // eight loads in flight per lane (clamped indices, masked products)
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u < n ? e0 + 64 * u : 0, b = e / POOLK, k = e - b * POOLK;
        v[u] = a.pooled[((long)b * P + ci) * POOLK + k];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (e0 + 64 * u < n) sm += z[e0 + 64 * u] * v[u];
    }
    sm = wave_sum(sm);
    if (lane == 0) a.dwc[c * P + ci] += sm;
  }
}

static inline bool pool_ok(int B, int P, int H, int W) {
  return B >= 1 && B <= 64 && P >= 1 && P <= 32 && H >= 1 && W >= 1 && W <= 64 && H <= 64 && (long)B * POOLK >= 2;
}

template <typename T>
static int pool_branch_fwd_impl(const T* x, long sxb, const float* wc, const float* gamma, const float* beta, float eps,
                                float slope, const float* RH, const float* RW, T* y, long syb, float* pooled, float* t, float* mean,
                                float* var, float* rmean, float* rvar, float momentum, long* nbt, int B, int P, int H, int W,
                                hipStream_t stream) {
  if (!x || !wc || !gamma || !beta || !RH || !RW || !y || !pooled || !t || !mean || !var) return CENET_EINVAL;
  if (!pool_ok(B, P, H, W)) return CENET_EUNSUPPORTED;
  PoolArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.sxb = sxb; a.y = y; a.syb = syb; a.pooled = pooled; a.t = t; a.wc = wc; a.gamma = gamma; a.beta = beta; a.RH = RH;
  a.RW = RW; a.eps = eps; a.slope = slope; a.mean = mean; a.var = var; a.rmean = rmean; a.rvar = rvar; a.momentum = momentum;
  a.nbt = nbt; a.B = B; a.P = P; a.H = H; a.W = W;
  CENET_LAUNCH((pool_mix_fwd_kernel<T>), dim3(B), dim3(256), stream, a);
  CENET_LAUNCH((pool_up_fwd_kernel<T>), dim3(P, B), dim3(256), stream, a);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
template <typename T>
static int pool_branch_bwd_acc_impl(const T* g, long sgb, const float* wc, const float* gamma, const float* beta, float eps,
                                    float slope, const float* RH, const float* RW, const float* pooled, const float* t,
                                    const float* mean, const float* var, float* dt_ws, T* dx, long sdb, float* dwc_acc,
                                    float* dgamma_acc, float* dbeta_acc, int B, int P, int H, int W, hipStream_t stream) {
  if (!g || !wc || !gamma || !beta || !RH || !RW || !pooled || !t || !mean || !var || !dt_ws || !dx || !dwc_acc || !dgamma_acc ||
      !dbeta_acc)
    return CENET_EINVAL;
  if (!pool_ok(B, P, H, W)) return CENET_EUNSUPPORTED;
  PoolArgs a;
  memset(&a, 0, sizeof(a));
  a.x = g; a.sxb = sgb; a.y = dx; a.syb = sdb; a.pooled = (float*)pooled; a.t = (float*)t; a.dt = dt_ws; a.wc = wc; a.dwc = dwc_acc;
  a.gamma = gamma; a.beta = beta; a.RH = RH; a.RW = RW; a.eps = eps; a.slope = slope; a.mean = (float*)mean; a.var = (float*)var;
  a.dgamma = dgamma_acc; a.dbeta = dbeta_acc; a.B = B; a.P = P; a.H = H; a.W = W;
  CENET_LAUNCH((pool_up_bwd_resample_kernel<T>), dim3(P, B), dim3(256), stream, a);
  CENET_LAUNCH(pool_up_bwd_bn_kernel, dim3(P), dim3(1024), stream, a);
  CENET_LAUNCH((pool_mix_bwd_kernel<T>), dim3(B, P), dim3(256), stream, a);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

constexpr int EUCB_SM_SMALL = 48 * 1024, EUCB_SM_LARGE = 152 * 1024;

// images per group of the backward's LDS gradient planes (0: does not fit)
template <typename T>
static inline int eucb_bwd_group(int B, int H, int W, int sm) {
  const long xs = (((long)B * (H + 2) * (W + 2) * 4) + 15) & ~15L;  // (LDS planes are fp32 for every tensor type)
  const long plane = 4L * (2 * H + 2) * (2 * W + 2);
  long G = (sm - xs) / plane;
  if (G > B) G = B;
  return G < 1 ? 0 : (int)G;
}

template <typename T>
static int eucb_fwd_impl(const T* x, long sxb, const float* w, const float* gamma, const float* beta, float eps, float slope,
                         T* y, long syb, float* mean, float* var, float* rmean, float* rvar, float momentum, long* nbt, int B,
                         int C, int H, int W, hipStream_t stream) {
  if (!x || !w || !gamma || !beta || !y || !mean || !var || B <= 0 || C <= 0 || H <= 0 || W <= 0) return CENET_EINVAL;
  const long need = (long)B * (H + 2) * (W + 2) * 4;
  if (need > EUCB_SM_LARGE || (syb & 1) || (((uintptr_t)y) & 7)) return CENET_EUNSUPPORTED;
  EucbArgs a;
  a.x = x; a.sxb = sxb; a.y = y; a.syb = syb; a.g = nullptr; a.sgb = 0; a.w = w; a.gamma = gamma; a.beta = beta; a.eps = eps;
  a.slope = slope; a.mean = mean; a.var = var; a.rmean = rmean; a.rvar = rvar; a.momentum = momentum; a.nbt = nbt;
  a.dw = a.dgamma = a.dbeta = nullptr; a.B = B; a.H = H; a.W = W;
  if (need <= EUCB_SM_SMALL) CENET_LAUNCH((eucb_fwd_kernel<T, 512, EUCB_SM_SMALL>), dim3(C), dim3(512), stream, a);
  else CENET_LAUNCH((eucb_fwd_kernel<T, 1024, EUCB_SM_LARGE>), dim3(C), dim3(1024), stream, a);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

template <typename T>
static int eucb_bwd_acc_impl(const T* g, long sgb, const T* x, long sxb, const float* w, const float* gamma, const float* beta,
                             float eps, float slope, const float* mean, const float* var, T* dx, long sdb, float* dw_acc,
                             float* dgamma_acc, float* dbeta_acc, int B, int C, int H, int W, hipStream_t stream) {
  if (!g || !x || !w || !gamma || !beta || !mean || !var || !dx || !dw_acc || !dgamma_acc || !dbeta_acc || B <= 0 || C <= 0 ||
      H <= 0 || W <= 0)
    return CENET_EINVAL;
  if ((sgb & 1) || (((uintptr_t)g) & 7)) return CENET_EUNSUPPORTED;
  EucbArgs a;
  a.x = x; a.sxb = sxb; a.y = dx; a.syb = sdb; a.g = g; a.sgb = sgb; a.w = w; a.gamma = gamma; a.beta = beta; a.eps = eps;
  a.slope = slope; a.mean = (float*)mean; a.var = (float*)var; a.rmean = a.rvar = nullptr; a.momentum = 0.f; a.nbt = nullptr;
  a.dw = dw_acc; a.dgamma = dgamma_acc; a.dbeta = dbeta_acc; a.B = B; a.H = H; a.W = W;
  int G = eucb_bwd_group<T>(B, H, W, EUCB_SM_SMALL);
  if (G >= 4 || G == B) {
    CENET_LAUNCH((eucb_bwd_kernel<T, 512, EUCB_SM_SMALL>), dim3(C), dim3(512), stream, a, G);
  } else {
    G = eucb_bwd_group<T>(B, H, W, EUCB_SM_LARGE);
    if (G < 1) return CENET_EUNSUPPORTED;
    CENET_LAUNCH((eucb_bwd_kernel<T, 1024, EUCB_SM_LARGE>), dim3(C), dim3(1024), stream, a, G);
  }
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}


/* does the fused EUCB front (forward AND backward) take this shape?  esize = 2 (bf16) / 4 (fp32) */
extern "C" int cenet_eucb_supported(int B, int H, int W, int esize) {
  if (B <= 0 || H <= 0 || W <= 0 || H * W < 16 || (esize != 2 && esize != 4)) return 0;
  const long need = (long)B * (H + 2) * (W + 2) * 4;
  if (need > EUCB_SM_LARGE) return 0;
  return (esize == 2 ? eucb_bwd_group<bf16_t>(B, H, W, EUCB_SM_LARGE) : eucb_bwd_group<float>(B, H, W, EUCB_SM_LARGE)) >= 1;
}

CENET_TWIN(eucb_fwd, (const T* x, long sxb, const float* w, const float* gamma, const float* beta, float eps, float slope, T* y,
                      long syb, float* mean, float* var, float* running_mean, float* running_var, float momentum,
                      long* num_batches_tracked, int B, int C, int H, int W, hipStream_t stream),
           (x, sxb, w, gamma, beta, eps, slope, y, syb, mean, var, running_mean, running_var, momentum, num_batches_tracked, B, C,
            H, W, stream))
CENET_TWIN(eucb_bwd_acc, (const T* g, long sgb, const T* x, long sxb, const float* w, const float* gamma, const float* beta,
                          float eps, float slope, const float* mean, const float* var, T* dx, long sdb, float* dw_acc,
                          float* dgamma_acc, float* dbeta_acc, int B, int C, int H, int W, hipStream_t stream),
           (g, sgb, x, sxb, w, gamma, beta, eps, slope, mean, var, dx, sdb, dw_acc, dgamma_acc, dbeta_acc, B, C, H, W, stream))

/* a channel over the batch (B * HW elements) is small enough for the channel-local chains */
extern "C" int cenet_chanloc_supported(int B, int HW) {
  int nt = 0;
  // (planes below 4 x 4 keep the launch chains: BatchNorm over a handful of values is ill-conditioned there and the chains'
  // two-pass statistics are what the small-shape tests are calibrated on; no real level is that small)
  return B > 0 && HW >= 16 && (long)B * HW <= 8192 && own_pick(B, HW, 8, &nt) > 0;
}

CENET_TWIN(cfam_mid_fwd, (const T* p_raw, const T* m, const T* x0, T* x1, T* y2, const float* gamma_p, const float* beta_p,
                          float eps_p, float* mean_p, float* var_p, float* rmean_p, float* rvar_p, float mom_p, long* nbt_p,
                          const float* w, const float* ls, const float* gamma_2, const float* beta_2, float eps_2, float* mean_2,
                          float* var_2, float* rmean_2, float* rvar_2, float mom_2, long* nbt_2, int B, int C, int HW,
                          hipStream_t stream),
           (p_raw, m, x0, x1, y2, gamma_p, beta_p, eps_p, mean_p, var_p, rmean_p, rvar_p, mom_p, nbt_p, w, ls, gamma_2, beta_2,
            eps_2, mean_2, var_2, rmean_2, rvar_2, mom_2, nbt_2, B, C, HW, stream))
CENET_TWIN(cfam_mid_bwd_acc, (const T* g_y2, const T* g_x1, const T* p_raw, const T* m, const T* x1, T* d_p_raw, T* d_m, T* d_x0,
                              const float* gamma_p, const float* beta_p, float eps_p, const float* mean_p, const float* var_p,
                              const float* w, const float* ls, const float* gamma_2, float eps_2, const float* mean_2,
                              const float* var_2, float* dgamma_p_acc, float* dbeta_p_acc, float* dw_acc, float* dls_acc,
                              float* dgamma_2_acc, float* dbeta_2_acc, int B, int C, int HW, hipStream_t stream),
           (g_y2, g_x1, p_raw, m, x1, d_p_raw, d_m, d_x0, gamma_p, beta_p, eps_p, mean_p, var_p, w, ls, gamma_2, eps_2, mean_2,
            var_2, dgamma_p_acc, dbeta_p_acc, dw_acc, dls_acc, dgamma_2_acc, dbeta_2_acc, B, C, HW, stream))

CENET_TWIN(dwbn_fwd, (const T* x, long sxb, const float* const* w, const int* dil, int nb, int g, int p, T* v, long svb, T* rest,
                      long srb, const float* gamma, const float* beta, float eps, float* mean, float* var, float* running_mean,
                      float* running_var, float momentum, long* num_batches_tracked, int B, int H, int W, hipStream_t stream),
           (x, sxb, w, dil, nb, g, p, v, svb, rest, srb, gamma, beta, eps, mean, var, running_mean, running_var, momentum,
            num_batches_tracked, B, H, W, stream))
CENET_TWIN(dwbn_bwd_acc, (const T* g_v, long sgb, const T* g_rest, long srb, const T* g_add, long sab, const T* x, long sxb,
                          const float* const* w, const int* dil, int nb, int g, int p, const float* gamma, const float* beta,
                          float eps, const float* mean, const float* var, T* dx, long sdb, float* const* dw_acc,
                          float* dgamma_acc, float* dbeta_acc, int B, int H, int W, hipStream_t stream),
           (g_v, sgb, g_rest, srb, g_add, sab, x, sxb, w, dil, nb, g, p, gamma, beta, eps, mean, var, dx, sdb, dw_acc,
            dgamma_acc, dbeta_acc, B, H, W, stream))

CENET_TWIN(cfam_front_fwd, (const T* x0, T* y1, T* xs, const float* gamma1, const float* beta1, float eps1, float* mean1,
                            float* var1, float* rmean1, float* rvar1, float mom1, long* nbt1, const float* fc1, const float* fc2,
                            const float* gamma_d, const float* beta_d, float eps_d, float* mean_d, float* var_d, float* rmean_d,
                            float* rvar_d, float mom_d, long* nbt_d, float* u, int* amax, float* z, float* zn, int B, int C, int HW,
                            hipStream_t stream),
           (x0, y1, xs, gamma1, beta1, eps1, mean1, var1, rmean1, rvar1, mom1, nbt1, fc1, fc2, gamma_d, beta_d, eps_d, mean_d,
            var_d, rmean_d, rvar_d, mom_d, nbt_d, u, amax, z, zn, B, C, HW, stream))
CENET_TWIN(cfam_front_bwd_acc, (const T* g_xs, const T* g_y1, const T* g_tap, const T* x0, T* dx0, const float* gamma1,
                                const float* beta1, float eps1, const float* mean1, const float* var1, const float* fc1,
                                const float* fc2, const float* gamma_d, float eps_d, const float* mean_d, const float* var_d,
                                const float* u, const int* amax, const float* z, const float* zn, float* dgamma1_acc,
                                float* dbeta1_acc, float* dfc1_acc, float* dfc2_acc, float* dgamma_d_acc, float* dbeta_d_acc, int B,
                                int C, int HW, hipStream_t stream),
           (g_xs, g_y1, g_tap, x0, dx0, gamma1, beta1, eps1, mean1, var1, fc1, fc2, gamma_d, eps_d, mean_d, var_d, u, amax, z, zn,
            dgamma1_acc, dbeta1_acc, dfc1_acc, dfc2_acc, dgamma_d_acc, dbeta_d_acc, B, C, HW, stream))

CENET_TWIN(dwact_fwd, (const T* x, const float* w, const float* bias, T* y, int act, float slope, int dil, int B, int C, int H,
                       int W, hipStream_t stream), (x, w, bias, y, act, slope, dil, B, C, H, W, stream))
CENET_TWIN(dwact_bwd_acc, (const T* g, const T* x, const float* w, const float* bias, T* dx, float* dw_acc, float* dbias_acc,
                           int act, float slope, int dil, int B, int C, int H, int W, hipStream_t stream),
           (g, x, w, bias, dx, dw_acc, dbias_acc, act, slope, dil, B, C, H, W, stream))

CENET_TWIN(pool_branch_fwd, (const T* x, long sxb, const float* wc, const float* gamma, const float* beta, float eps, float slope,
                             const float* RH, const float* RW, T* y, long syb, float* pooled, float* t, float* mean, float* var,
                             float* running_mean, float* running_var, float momentum, long* num_batches_tracked, int B, int P,
                             int H, int W, hipStream_t stream),
           (x, sxb, wc, gamma, beta, eps, slope, RH, RW, y, syb, pooled, t, mean, var, running_mean, running_var, momentum,
            num_batches_tracked, B, P, H, W, stream))
CENET_TWIN(pool_branch_bwd_acc, (const T* g, long sgb, const float* wc, const float* gamma, const float* beta, float eps,
                                 float slope, const float* RH, const float* RW, const float* pooled, const float* t,
                                 const float* mean, const float* var, float* dt_ws, T* dx, long sdb, float* dwc_acc,
                                 float* dgamma_acc, float* dbeta_acc, int B, int P, int H, int W, hipStream_t stream),
           (g, sgb, wc, gamma, beta, eps, slope, RH, RW, pooled, t, mean, var, dt_ws, dx, sdb, dwc_acc, dgamma_acc, dbeta_acc, B,
            P, H, W, stream))

// ---- self-test of the DPP wave reductions of common.h (tests/test_kern_misc.py): wave w of the launch reduces x[64 w .. 64 w + 64);
// sums / maxs / mins hold 2 nwaves entries ----
__global__ __launch_bounds__(256) void wave_reduce_selftest_kernel(const float* __restrict__ x, float* __restrict__ sums,
                                                                  float* __restrict__ maxs, int* __restrict__ mins, int nwaves) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= nwaves) return;  // (wave-uniform)
  const float v = x[(long)w * 64 + lane];
  const float s = wave_sum_dpp(v), m = wave_max_dpp(v);
  const int mi = wave_min_i_dpp((int)(v * 1024.f) + lane);
  // every lane must hold the result (the reductions broadcast): lane 0 writes row w, lane 37 row nwaves + w
  if (lane == 0 || lane == 37) {
    const int o = lane ? nwaves + w : w;
    sums[o] = s;
    maxs[o] = m;
    mins[o] = mi;
  }
}
extern "C" int cenet_selftest_wave_reduce(const float* x, float* sums, float* maxs, int* mins, int nwaves, hipStream_t stream) {
  if (!x || !sums || !maxs || !mins || nwaves <= 0) return CENET_EINVAL;
  CENET_LAUNCH(wave_reduce_selftest_kernel, dim3(cdiv(nwaves, 4)), dim3(256), stream, x, sums, maxs, mins, nwaves);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
