// adam.hip — the fused Adam / AdamW update over the flat parameter arena.
//   Adam / AdamW(lr, betas, eps, weight_decay)   utils/core.py:13-18 (torch.optim.Adam / AdamW, amsgrad off, maximize off)
// Per element, torch's single-tensor Adam with the gradient pre-multiplied by grad_scale:
//   g = grad * gscale
//   Adam:  g += wd * p                   AdamW: p *= 1 - lr * wd
//   m = lerp(m, g, 1 - beta1)            (torch's lerp: m + w (g - m) for w < 0.5, g - (g - m)(1 - w) otherwise)
//   v = v * beta2 + (1 - beta2) * g * g
//   p += -step_size * (m / (sqrt(v) / bc2_sqrt + eps)),  step_size = lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t)
// The bias corrections and the products of hyper-parameters are computed on the host in double (as torch computes them in
// Python) and read from a device buffer, so a captured step picks up the next step's values from FusedAdam.prepare().
// IEEE sqrtf and division (hipcc's default for fp32): parity with torch is the point of this kernel.
// A pure stream: 16 B read + 12 B written per parameter (+2 B for the bf16 shadow), in 16-byte accesses.
#include "common.h"
#include "../../include/cenet_hip.h"

// hyper (device, fp32): [0] lr, [1] beta1, [2] beta2, [3] eps, [4] weight_decay, [5] grad_scale, [6] step_size,
// [7] bc2_sqrt, [8] decoupled (AdamW) flag, [9] 1 - beta1, [10] 1 - beta2, [11] 1 - lr * weight_decay

struct adam_hp {
  float b2, eps, wd, gs, nss, bc2s, w1, omw1, omb2, decay;
  bool dec, coupled;
};

__device__ __forceinline__ adam_hp adam_load_hyper(const float* __restrict__ h) {
  adam_hp r;
  r.b2 = h[2], r.eps = h[3], r.wd = h[4], r.gs = h[5], r.nss = -h[6], r.bc2s = h[7];
  r.dec = h[8] != 0.f;
  r.w1 = h[9], r.omw1 = 1.f - h[9], r.omb2 = h[10], r.decay = h[11];
  r.coupled = !r.dec && r.wd != 0.f;  // torch applies the coupled decay only when weight_decay != 0
  return r;
}

__device__ __forceinline__ float adam_elem(const adam_hp& h, float p, float gr, float& m, float& v) {
  float g = gr * h.gs;
  if (h.dec) p = p * h.decay;
  else if (h.coupled) g = g + h.wd * p;
  m = h.w1 < 0.5f ? m + h.w1 * (g - m) : g - (g - m) * h.omw1;
  v = v * h.b2 + h.omb2 * g * g;
  const float denom = sqrtf(v) / h.bc2s + h.eps;
  return p + h.nss * (m / denom);
}

// grid-stride over quads [0, nq); the scalar tail [4 nq, n) (an arena is a multiple of 64 elements: empty there) by the first
// threads of the grid
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, const float* __restrict__ hyper, long n, long nq,
                                                  bf16_t* __restrict__ shadow) {
  const adam_hp h = adam_load_hyper(hyper);
  const long stride = (long)gridDim.x * 256;
  const long t0 = (long)blockIdx.x * 256 + threadIdx.x;
  for (long q = t0; q < nq; q += stride) {
    const long i = 4 * q;
    f4 pv = ld4(p + i), mv = ld4(m + i), vv = ld4(v + i);
    const f4 gv = ld4(g + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) pv.v[e] = adam_elem(h, pv.v[e], gv.v[e], mv.v[e], vv.v[e]);
    st4(p + i, pv);
    st4(m + i, mv);
    st4(v + i, vv);
    if (shadow) st4(shadow + i, pv);
  }
  for (long i = 4 * nq + t0; i < n; i += stride) {
    float mm = m[i], vv = v[i];
    const float pn = adam_elem(h, p[i], g[i], mm, vv);
    p[i] = pn;
    m[i] = mm;
    v[i] = vv;
    if (shadow) shadow[i] = (bf16_t)cenet_f2bf(pn);
  }
}

static int adam_launch(float* p, const float* g, float* m, float* v, const float* hyper, long n, bf16_t* shadow,
                       hipStream_t stream) {
  if (n <= 0) return CENET_EINVAL;
  // 16-byte accesses need every stream quad-aligned (the arena's buffers are fresh allocations); otherwise all elements take
  // the scalar loop
  const bool quads = quad_aligned<float>(p) && quad_aligned<float>(g) && quad_aligned<float>(m) && quad_aligned<float>(v) &&
                     (shadow == nullptr || quad_aligned<bf16_t>(shadow));
  const long nq = quads ? n / 4 : 0;
  // 256 CUs x 8 workgroups of 4 waves: 32 waves per CU in flight, each thread walks ~16 quads of a 33 M-parameter arena
  long blocks = ((nq > 0 ? nq : n) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  CENET_LAUNCH(adam_kernel, dim3((unsigned)blocks), dim3(256), stream, p, g, m, v, hyper, n, nq, shadow);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_adam_step_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, const float* hyper12, long n,
                                   hipStream_t stream) {
  return adam_launch(p, g, exp_avg, exp_avg_sq, hyper12, n, nullptr, stream);
}
extern "C" int cenet_adam_step_shadow_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, const float* hyper12,
                                          long n, unsigned short* shadow_bf16, hipStream_t stream) {
  return adam_launch(p, g, exp_avg, exp_avg_sq, hyper12, n, shadow_bf16, stream);
}
