/* cenet_hip.h — C ABI of libcenet_hip.so, the MI355X (gfx950) kernel library behind cenet_amd.networks.CENet.
 *
 * The reference (xmindflow/cenet) is pure PyTorch: its "FFI" for this path is the ATen operator set its
 * nn.Modules call.  Each entry point below replaces the ATen op group cited next to it (file:line relative to
 * /root/reference/src/); cenet_amd/ops.py binds them with ctypes and wraps them in torch.autograd.Functions,
 * and cenet_amd/networks mirrors the reference's nn.Module tree on top.
 *
 * Conventions: raw device pointers; no allocation, no ownership transfer and no host synchronisation inside;
 * workspaces are passed in; every call takes the HIP stream to launch on and is re-entrant (called from the
 * autograd worker thread); return 0 on success, non-zero error code otherwise (the Python wrapper raises).
 * Tensors are fp32 ("_f32" entry points: the parity mode) or, for activations, bf16 ("_bf16" twins at the end of this header:
 * the throughput mode).  "NCHW" tensors are addressed as ptr[b*sb + c*HW + y*W + x] so that a
 * channel slice of a larger tensor is (ptr + lo*HW, sb = Ctotal*HW).  "TOK" tensors are [B, N, C] contiguous.
 * Functions whose name ends in _acc ADD into their gradient outputs (the flat gradient arena is zeroed once
 * per step), using float atomics where several workgroups share a destination.
 */
#ifndef CENET_HIP_H
#define CENET_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CENET_HOSTSIM_BUILD
typedef struct ihipStream_t* cenet_stream_t;
#else
typedef void* cenet_stream_t;
#endif

/* ---- GEMM / implicit-GEMM convolution (gemm.hip) ------------------------------------------------------- */
/* Logical matrix operand. mode 0: elem(r,c) = ptr[b*sb + kb*skb + r*sr + c*sc].
 * mode 1: on-the-fly im2col view of an image tensor: with patch index e=(ci,ky,kx) and pixel index p=(py,px)
 *   (e,p) = patch_is_row ? (r,c) : (c,r);
 *   !transposed: iy = py*stride - pad + ky*dil           (conv forward / weight-gradient gather)
 *    transposed: iy = (py + pad - ky*dil)/stride if divisible   (data-gradient gather)
 *   elem = in-range ? ptr[b*sb + kb*skb + ci*sci + iy*sy + ix*sx] : 0.
 * kfast: 1 if consecutive k are adjacent in memory (picks the coalesced staging pattern). */
typedef struct {
  const void* ptr;           /* fp32 or bf16 elements (the `dtype` argument of cenet_gemm); strides count ELEMENTS */
  long sb, sb2, skb, sr, sc; /* batch z -> (z / nb_inner, z % nb_inner): offset = (z/nb_inner)*sb + (z%nb_inner)*sb2 */
  long sk_outer;             /* mode 0 with kinner > 0: k -> (k / kinner)*sk_outer + (k % kinner)*(sc or sr) */
  int kinner;
  int mode, kfast;
  int patch_is_row, transposed;
  int KH, KW, Pw, Hs, Ws, stride, pad, dil;
  long sci, sy, sx;
} cenet_mat_t;

/* Epilogue: v = alpha*acc; atomic ? C += v : C = bscale[b]*act(v + bias) + R.  C and R have the operands' element type,
 * except that an ATOMIC epilogue (split-K, scatter-add) always adds into an fp32 C; bias / bscale are always fp32. */
typedef struct {
  void* C;
  long scb, scb2, scr, scc;
  const float* bias;
  int bias_on_row;
  int act;
  float slope;
  const float* bscale;
  const void* R;
  long srb, srb2, srr, src;
  int atomic;
  float alpha;
  /* cmode 1: col2im scatter — row = patch index (ci,ky,kx), col = output pixel (py,px);
   * C address = b*scb + ci*csci + (py*cstride - cpad + ky)*csy + (px*cstride - cpad + kx)*csx, skipped when out of
   * [0,cHs)x[0,cWs). Used for the data-gradient of strided convolutions (atomic when patches overlap). */
  int cmode, cKH, cKW, cPw, cHs, cWs, cstride, cpad;
  long csci, csy, csx;
  /* > 0: bscale is indexed by (row / bscale_rows) instead of by batch -- a [B, n, K] activation run as ONE flat GEMM of
   * B*n rows with the per-sample DropPath scale of pvtv2.py:117-118 still applied per sample (bscale_rows = n). */
  int bscale_rows;
  /* atomic (weight-gradient) contractions only: asum[m] += sum_k A[m, k] over the whole reduction (all k-batches) -- the
   * bias gradient that goes with the weight gradient dW = dY^T X (A = dY^T), folded into the pass that already reads dY
   * instead of a second sweep (aten::sum of the linear / 1x1-convolution backward).  fp32, may be NULL. */
  float* asum;
} cenet_epi_t;

/* Replaces aten::addmm/mm/bmm/convolution(+_backward) — pvtv2.py:41,45,90,98,106,164; cfam.py:149,158,299,302;
 * nlb.py:106-115,142; blocks.py:178,211,320; dseb.py:164; unet.py:156-197; multihead_diffattn.py:79-81,126. */
int cenet_gemm_f32(const cenet_mat_t* A, const cenet_mat_t* B, const cenet_epi_t* E, int M, int N, int K,
                   int nbatch, int nb_inner, int nkb, int splits, cenet_stream_t stream);
/* The same contraction on bf16 tensors (throughput mode): A, B (and C / R unless E->atomic) hold bf16 elements, products
 * run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; weights are passed as their bf16 shadow copy (cenet_sgd_step_shadow_f32
 * / cenet_cast_f32_to_bf16). */
int cenet_gemm_bf16(const cenet_mat_t* A, const cenet_mat_t* B, const cenet_epi_t* E, int M, int N, int K,
                    int nbatch, int nb_inner, int nkb, int splits, cenet_stream_t stream);
/* Measurement aid: the kernel instance the last cenet_gemm_* call on this thread launched, spelled as rocprofv3 prints it
 * ("gemm_ring_kernel<false, false, 64, 64, 4, false>").  bench.py groups its live per-launch timings by this name. */
const char* cenet_gemm_last_kernel(void);

/* GROUPED weight gradients (gemm_group.hip): the parameter gradients that autograd computes one aten::mm / aten::convolution_
 * backward at a time for every Linear (pvtv2.py:41,45,60-63,90,98,106; multihead_diffattn.py:57-60) and 1x1 convolution
 * (cfam.py:128-144,283-288; nlb.py:66-92; blocks.py:303-311; dseb.py:111) of a backward segment, as ONE launch per <= 56
 * problems.  Problem i:  C_i[m, n] += sum over kb < nkb, k < K of A_i(m, k) * B_i(k, n)   and   asum_i[m] += sum of A_i(m, k)
 * (the bias gradient; may be NULL), with  A(m, k) = akf ? A[kb*skbA + m*lda + k] : A[kb*skbA + k*lda + m],
 * B(k, n) = bkf ? B[kb*skbB + n*ldb + k] : B[kb*skbB + k*ldb + n];  A, B bf16 (dY and the layer input), C fp32 row-major
 * [M, N] (a slot of the gradient arena), strides in elements.  akf == bkf is required (token-major Linear: both 0; NCHW 1x1
 * convolution: both 1), else CENET_EUNSUPPORTED.  Long reductions are cut into K slices whose partial tiles go to `ws`
 * (cenet_wgrad_group_ws_floats(p, n) floats, may be 0) and are summed in slice order by a second launch: no float atomics
 * unless two problems of a call share a C, results independent of scheduling. */
typedef struct {
  const void* A;
  const void* B;
  float* C;
  float* asum;
  long lda, ldb, skbA, skbB;
  int M, N, K, nkb;
  int akf, bkf;
} cenet_wgrad_prob_t;
long cenet_wgrad_group_ws_floats(const cenet_wgrad_prob_t* p, int n);
int cenet_wgrad_group_bf16(const cenet_wgrad_prob_t* p, int n, float* ws, long ws_floats, cenet_stream_t stream);
/* Measurement aid: the same reduction issued in two calls — phase 1 launches the K-slice kernels only, phase 2 the fold
 * kernels only (phase 0 = cenet_wgrad_group_bf16) — so that bench.py can bracket the two kernel symbols with HIP events. */
/* the partition cenet_wgrad_group_bf16 makes of its problems: launch[i] = index of the grouped launch problem i goes to (issue
 * order), bm / bn / ns [i] = that launch's tile and ring depth (gemm_group_kernel<akf, akf, bm, bn, ns>) */
int cenet_wgrad_group_plan(const cenet_wgrad_prob_t* p, int n, int* launch, int* bm, int* bn, int* ns);
int cenet_wgrad_group_phase_bf16(const cenet_wgrad_prob_t* p, int n, float* ws, long ws_floats, int phase, cenet_stream_t stream);

/* Direct ("LDS halo") stride-1 same-padded convolution on bf16 tensors (throughput mode, conv_direct.hip): replaces
 * aten::convolution(+ data-gradient) for out.py:41-49,59 (5x5 32->32, 3x3 64->64, 3x3 64->32 and their dgrads).
 * x, y: bf16; w: the fp32 master weight.  dgrad = 1: x is dY [B,Cin,H,W], w is the ORIGINAL forward weight [Cin,Cout,k,k],
 * y is dX [B,Cout,H,W]. */
int cenet_conv_direct_supported(int Cin, int Cout, int k, int stride, int pad);
int cenet_conv_direct_bf16(const unsigned short* x, const float* w, unsigned short* y, int B, int Cin, int Cout, int H, int W,
                           int k, int dgrad, cenet_stream_t stream);
/* Weight gradient of the same convolutions in the same mode (replaces the implicit-GEMM wgrad of unet.py:156-197,
 * blocks.py:211, out.py:41-49 for 5x5 32->32 and 3x3 64->64 / 64->32): dw_acc[Cout,Cin,k,k] += dY (*) X.
 * ws: cenet_conv_wgrad_direct_ws_floats(Cin, Cout, k) floats of scratch (per-workgroup partial sums). */
/* One-channel input (the network image) into Cout <= 32 channels, stride 1, pad k/2, k in {1, 3, 5}, bf16 tensors
 * (conv_c1.hip): the residual block of the output head that reads x (out.py:41-44; unet.py:156-197 conv1 / conv3).
 * Forward y = w (*) x and the weight gradient dw_acc += dy (*) x; the image itself needs no gradient. */
int cenet_conv_c1_supported(int Cin, int Cout, int k, int stride, int pad);
/* `groups` independent square bias-free 1x1 convolutions over G <= 40 channels each (conv_c1.hip, bf16): y[b, j*G + o, p] =
 * sum_i W[j][o][i] x[b, j*G + i, p]  (transpose != 0: W[j][i][o], the data gradient).  The pointwise convs of the dilated
 * SepConvBN branches and the pooled-branch conv of cfam.py:208-219 at channel counts where a GEMM tile is mostly padding. */
/* 1x1 convolution from 64 channels to Cout <= 16 channels with bias, bf16 tensors (conv_c1.hip): the last layer of the
 * segmentation head (unet.py:200-217 UnetOutBlock, out.py:49).  x [B,64,HW], W bf16 [Cout,64] (shadow of the fp32 weight),
 * y / dy [B,Cout,HW]; the weight-gradient entry adds into fp32 dW [Cout,64] and dbias [Cout] (Cout in {2, 4, 9}). */
int cenet_pw_fewout_supported(int Cin, int Cout);
int cenet_pw_fewout_wgrad_supported(int Cin, int Cout);
int cenet_pw_fewout_fwd_bf16(const unsigned short* x, const unsigned short* W, const float* bias, unsigned short* y, int B, int Cin,
    int Cout, long HW, cenet_stream_t stream);
int cenet_pw_fewout_dgrad_bf16(const unsigned short* dy, const unsigned short* W, unsigned short* dx, int B, int Cin, int Cout,
    long HW, cenet_stream_t stream);
int cenet_pw_fewout_wgrad_bf16(const unsigned short* x, const unsigned short* dy, float* dW_acc, float* dbias_acc, int B, int Cin,
    int Cout, long HW, cenet_stream_t stream);
int cenet_pw_small_supported(int G);
int cenet_pw_small_bf16(const unsigned short* x, const unsigned short* W, unsigned short* y, int B, int groups, int G, long HW,
    int transpose, cenet_stream_t stream);
int cenet_conv_c1_fwd_bf16(const unsigned short* x, const float* w, unsigned short* y, int B, int Cout, int H, int W, int k,
    cenet_stream_t stream);
int cenet_conv_c1_wgrad_bf16(const unsigned short* x, const unsigned short* dy, float* dw_acc, int B, int Cout, int H, int W,
    int k, cenet_stream_t stream);
int cenet_conv_wgrad_direct_supported(int Cin, int Cout, int k, int stride, int pad);
long cenet_conv_wgrad_direct_ws_floats(int Cin, int Cout, int k);
int cenet_conv_wgrad_direct_bf16(const unsigned short* x, const unsigned short* dy, float* dw_acc, float* ws, int B, int Cin,
                                 int Cout, int H, int W, int k, cenet_stream_t stream);
/* Test and measurement aid: what the last call on this thread into conv_direct.hip, conv_c1.hip or dwconv.hip launched — the kernel
 * with its template arguments, then the run-time numbers that select a code path inside it ("conv_direct_bf16_kernel<32, 32, 5, 4>
 * dgrad=0 grid=5 ntiles=24", "dw3x3_nchw_plane_kernel<ACT_GELU> ppw=4").  Written by the host dispatchers only. */
const char* cenet_conv_last_kernel(void);

/* ---- attention (attn.hip) -------------------------------------------------------------------------------- */
/* Element (b,h,i,d) of Q = q[b*qsb + h*qsh + i*qsi + d*qsd]; same for K (Nk rows), V (head h / v_head_div,
 * width Dv) and O / dO (strides os*).  lse, delta: [B,H,Nq] fp32.  q, k, v, o, dout, dq, dk, dv are fp32 (`_f32` entry points)
 * or bf16 (`_bf16`).  When v_head_div > 1 the backward ADDS into dv with atomics (caller zero-fills dv); with bf16 tensors
 * atomic accumulation needs `dkv_f32`: dk and dv then point to fp32 buffers laid out like k and v. */
typedef struct {
  const void *q, *k, *v;
  void* o;
  float* lse;
  const void* dout;
  void *dq, *dk, *dv;
  float* delta;
  long qsb, qsh, qsi, qsd, ksb, ksh, ksi, ksd, vsb, vsh, vsi, vsd, osb, osh, osi, osd;
  int B, H, Nq, Nk, D, Dv, v_head_div;
  float scale;
  int dkv_zeroed; /* backward only: caller guarantees dk / dv are zero-filled, so the library may slice the query range
                     over workgroups and accumulate dK / dV atomically (few keys under many queries) */
  int dkv_f32;    /* bf16 entry points only: dk / dv are fp32 accumulators */
  int finite_scores; /* fp32 entry points only (multihead_diffattn.py:95-106): q is scaled BEFORE the product (`q *= self.scaling`)
                        and the scores pass through torch.nan_to_num (NaN -> 0, +-inf -> +-FLT_MAX) before the softmax, so a q.k
                        product that overflows fp32 gives the reference's finite output; the backward rebuilds the scores the
                        same way and sets dS = 0 where the raw score was not finite (nan_to_num's backward).  The bf16 entry
                        points ignore it (overflowing scores are outside the supported domain there: INTEGRATION.md) */
} cenet_attn_t;
/* Replaces q@k^T -> softmax -> @v (pvtv2.py:101-105; nlb.py:117-138; multihead_diffattn.py:96-116) and backward.
 * Supported head dims: D<=64 with Dv<=128 (cenet_flash_attn_supported). */
int cenet_flash_attn_supported(int D, int Dv);
int cenet_flash_attn_fwd_f32(const cenet_attn_t* p, cenet_stream_t stream);
int cenet_flash_attn_bwd_f32(const cenet_attn_t* p, cenet_stream_t stream);
int cenet_flash_attn_fwd_bf16(const cenet_attn_t* p, cenet_stream_t stream);
int cenet_flash_attn_bwd_bf16(const cenet_attn_t* p, cenet_stream_t stream);
/* Differential attention of the DSEB skip blocks on bf16 tensors (attn_diff.hip; multihead_diffattn.py:83-109): softmax head
 * 2h+s (s = 0, 1) attends with q_{2h+s}, k_{2h+s} over the SHARED value head h; U[b, 2h+s] = softmax(q k^T * scale) v_h.
 * q, k [B, N, 2H*hd], v [B, N, H*2hd] (token-major, as the projections produce them), U, dU [B, 2H, N, 2hd], lse [B, 2H, N]
 * fp32; dq, dk, dv laid out like q, k, v.  ws: cenet_diffattn_heads_ws_bytes(B, H, N) bytes of scratch the backward uses to
 * pass the softmax statistics between its two kernels.  hd in {8, 16, 32}; all pointers 16-byte aligned. */
typedef struct {
  const void *q, *k, *v;
  void* U;
  float* lse;
  const void* dU;
  void *dq, *dk, *dv;
  void* ws;
  int B, H, N, hd;
  float scale;
  int batch_mul; /* 0 / 1: dense tensors.  m > 1: q / k / v (and dq / dk / dv) of image b start m rows-blocks apart, i.e. at
                  * element b * m * N * row_len of their pointers — q | k | v stacked per image as [B, 3, N, C] (the Non-local
                  * block's merged theta / phi / g projection, nlb.py:117-119, m = 3) are read and written in place */
} cenet_diffattn_t;
int cenet_diffattn_heads_supported(int hd, int N);
long cenet_diffattn_heads_ws_bytes(int B, int H, int N);
int cenet_diffattn_heads_fwd_bf16(const cenet_diffattn_t* p, cenet_stream_t stream);
int cenet_diffattn_heads_bwd_bf16(const cenet_diffattn_t* p, cenet_stream_t stream);
/* Plain self-attention with head dimension 64 or 128 on bf16 tensors through the same tiles (one softmax over both hd/2-column
 * halves): q, k, v [B, N, H*hd] token-major, U / dU [B, H, N, hd], lse [B, H, N], hd = 64 | 128, ws of cenet_attn64_ws_bytes.
 * Replaces the score / softmax / value products of the Non-local block at the 56x56 (C = 64) and 28x28 (C = 128) decoder
 * levels (nlb.py:117-138). */
long cenet_attn64_ws_bytes(int B, int H, int N);
int cenet_attn64_fwd_bf16(const cenet_diffattn_t* p, cenet_stream_t stream);
int cenet_attn64_bwd_bf16(const cenet_diffattn_t* p, cenet_stream_t stream);
/* Spatial-reduction attention backward (pvtv2.py:88-109) on bf16 tensors in ONE kernel: head dimension 64, Nk <= 64 keys
 * resident in LDS.  q, o, dout, dq [B, Nq, 64 H]; kv [B, Nk, 128 H] (k | v); lse [B, H, Nq] as the forward kernel left it;
 * dkv [B, Nk, 128 H] fp32, ZERO-FILLED by the caller (workgroups add their partial sums atomically). */
int cenet_sra_attn_bwd_supported(int hd, int Nk);
/* 64 < Nk <= 256 keys of head dimension 64 (pvtv2.py:92-105 at 512x512 inputs): cenet_sra_attn_bwd_bf16 then runs as two
 * launches — dQ with all keys resident, dK / dV per 64-key block (the saved lse makes key blocks independent). */
int cenet_sra_attn_bwd_blocks_supported(int hd, int Nk);
/* The forward of the same problem class (head dimension 64, Nk <= 64, cenet_sra_attn_bwd_supported) with the keys / values
 * resident: o [B, Nq, 64 H], lse [B, H, Nq] (natural log, as the backward entries expect). */
int cenet_sra_attn_fwd_bf16(const unsigned short* q, const unsigned short* kv, unsigned short* o, float* lse, int B, int H, int Nq,
    int Nk, float scale, cenet_stream_t stream);
int cenet_sra_attn_bwd_bf16(const unsigned short* q, const unsigned short* kv, const unsigned short* o,
    const unsigned short* dout, const float* lse, unsigned short* dq, float* dkv, int B, int H, int Nq, int Nk, float scale,
    cenet_stream_t stream);
/* The same kernel where its launch puts all queries of a (batch, head) in ONE workgroup (cenet_sra_attn_bwd_direct_supported:
 * the 14x14 and 7x7 stages at B = 32): dkv [B, Nk, 128 H] is written as bf16 directly — no zero fill, no atomics, no cast. */
int cenet_sra_attn_bwd_direct_supported(int B, int H, int Nq, int Nk);
/* 32-query tiles a wave of the Nk <= 64 backward launch walks through (workgroup = 4 waves = 128 * tiles queries). */
int cenet_sra_attn_bwd_tiles(int B, int H, int Nq);
int cenet_sra_attn_bwd_direct_bf16(const unsigned short* q, const unsigned short* kv, const unsigned short* o,
    const unsigned short* dout, const float* lse, unsigned short* dq, unsigned short* dkv, int B, int H, int Nq, int Nk,
    float scale, cenet_stream_t stream);
/* Row softmax for the materialised path (head dims > 128): aten::_softmax(+_backward_data).  Scores x and score gradients
 * dy are fp32 in both forms; the probabilities y and dx have the storage type of the entry point. */
int cenet_softmax_rows_fwd_f32(const float* x, float* y, long rows, int n, cenet_stream_t stream);
int cenet_softmax_rows_bwd_f32(const float* y, const float* dy, float* dx, long rows, int n, cenet_stream_t stream);
int cenet_softmax_rows_fwd_bf16(const float* x, unsigned short* y, long rows, int n, cenet_stream_t stream);
int cenet_softmax_rows_bwd_bf16(const unsigned short* y, const float* dy, unsigned short* dx, long rows, int n,
                                cenet_stream_t stream);
/* fp32 parity mode with non-finite scores (cenet_attn_t.finite_scores on the materialised path, multihead_diffattn.py:106): the
 * forward reads every score x through torch.nan_to_num; the backward takes the raw scores x as well and writes dx = 0 wherever
 * x is not finite (nan_to_num's backward is grad * isfinite(x)). */
int cenet_softmax_rows_finite_fwd_f32(const float* x, float* y, long rows, int n, cenet_stream_t stream);
int cenet_softmax_rows_finite_bwd_f32(const float* y, const float* dy, const float* x, float* dx, long rows, int n,
                                      cenet_stream_t stream);

/* ---- normalisation (norm.hip) ----------------------------------------------------------------------------- */
/* aten::native_layer_norm(+_backward) — pvtv2.py:117,124,166,69,221-245. x,y [rows,C]. */
int cenet_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int rows, int C, float eps, cenet_stream_t stream);
int cenet_layernorm_bwd_acc_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                float* dx, float* dgamma_acc, float* dbeta_acc, int rows, int C, cenet_stream_t stream);
/* the same with dx = LN-backward(dy) + dx_add: the gradient of a residual connection that by-passed the LayerNorm
 * (x + f(LN(x)), pvtv2.py:141-142) is folded in here instead of a separate aten::add; dx_add may be NULL. */
int cenet_layernorm_bwd_add_acc_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                    const float* dx_add, float* dx, float* dgamma_acc, float* dbeta_acc, int rows, int C,
                                    cenet_stream_t stream);
/* aten::native_batch_norm(+_backward), training mode — cfam.py:22-32,92,250; blocks.py:151,161,212,307; nlb.py:81;
 * unet.py:175-197.  ws: CENET_BN_WS_FLOATS(C) floats of scratch (per-split partial sums, no zero-fill needed).
 * stats writes batch mean / biased var and updates the running
 * buffers (momentum, unbiased var) and num_batches_tracked when given. */
/* Contract of the batch statistics: for ANY data the batch mean is accurate to 2^-24 sqrt(n) E|x| and the biased batch variance to
 * 2^-24 sqrt(n) (var + (2^-24 sqrt(n) E|x|)^2), n = B HW, times a small constant (tests/norm_ref.py), independent of the value of any
 * single element: where a kernel sums in one pass, the shift of its sums is a mean over the first min(HW, 64) elements of image 0's
 * plane, not one element.  ws holds at most 255 partial-sum slots per channel and moment, followed by the C shifts. */
#define CENET_BN_WS_FLOATS(C) (2L * (C) * 256)
int cenet_bn_stats_f32(const float* x, long sb, int B, int C, int HW, float* ws, float* mean, float* var,
                       float* running_mean, float* running_var, float momentum, long* num_batches_tracked,
                       cenet_stream_t stream);
int cenet_bn_apply_f32(const float* x, long sxb, float* y, long syb, const float* mean, const float* var, float eps,
                       const float* gamma, const float* beta, int act, float slope, int B, int C, int HW,
                       cenet_stream_t stream);
/* Train-mode BatchNorm forward in one call (two launches): statistics + normalisation (+ activation); writes y, the batch
 * mean / var the backward pass needs, and the running statistics (nn.BatchNorm2d.forward in training mode). */
int cenet_bn_train_fwd_f32(const float* x, long sxb, float* y, long syb, float* ws, float* mean, float* var,
    float* running_mean, float* running_var, float momentum, long* num_batches_tracked, float eps, const float* gamma,
    const float* beta, int act, float slope, int B, int C, int HW, int nbt_count, cenet_stream_t stream);
/* nbt_count (1 <= nbt_count <= C): the launch covers the channels of that many nn.BatchNorm2d modules whose parameters and
 * buffers lie back to back (the three dilated SepConvBN branches of cfam.py:208-212 in one launch); num_batches_tracked[0 ..
 * nbt_count) are each incremented.  1 for a single module. */
int cenet_bn_bwd_acc_f32(const float* dy, long sgb, const float* x, long sxb, float* dx, long sdb, const float* mean,
                         const float* var, float eps, const float* gamma, const float* beta, int act, float slope, int B,
                         int C, int HW, float* ws, float* dgamma_acc, float* dbeta_acc, cenet_stream_t stream);
/* ... + dx_add (batch stride sab, may be NULL): dx = BatchNormBackward(dy) + dx_add — the gradient of the residual connection
 * around the normalised branch (cfam.py:365-374) added by the kernel that writes dx (round 4) */
int cenet_bn_bwd_add_acc_f32(const float* dy, long sgb, const float* x, long sxb, float* dx, long sdb, const float* dx_add,
                             long sab, const float* mean, const float* var, float eps, const float* gamma, const float* beta,
                             int act, float slope, int B, int C, int HW, float* ws, float* dgamma_acc, float* dbeta_acc,
                             cenet_stream_t stream);

/* BatchNorm1d on a [B, C] fp32 matrix with 2 <= B <= 64 (the CCU gate, cfam.py:251-264: one value per image and channel), training
 * mode, forward and backward in ONE launch each (a thread owns a channel; round 4).  Forward: zn, batch mean / biased variance, running
 * statistics (unbiased variance) and the batch counter (NULL: not wanted); backward: dz written, dgamma / dbeta ADDED into. */
int cenet_bn1d_supported(int B);
int cenet_bn1d_train_fwd_f32(const float* z, float* zn, float* mean, float* var, float* running_mean, float* running_var,
                             float momentum, long* num_batches_tracked, float eps, const float* gamma, const float* beta, int B,
                             int C, cenet_stream_t stream);
int cenet_bn1d_bwd_acc_f32(const float* dy, const float* z, float* dz, const float* mean, const float* var, float eps,
                           const float* gamma, float* dgamma_acc, float* dbeta_acc, int B, int C, cenet_stream_t stream);

/* Test and measurement aid: what the last call on this thread into norm.hip launched, kernels with their template arguments and
 * the run-time numbers that select a code path, joined by '+' where a call launches several ("bn_partial_v4_kernel<float> S=2+
 * bn_finalize_kernel<float>+bn_apply_v4_kernel<float> fin=0 threads=64 chunks=1").  Written by the host dispatchers only. */
const char* cenet_norm_last_kernel(void);

/* ---- depthwise 3x3 conv (dwconv.hip) — aten::convolution(groups=C)(+_backward) ------------------------------ */
/* pvtv2.py:359-370 (token layout), cfam.py:132-140, blocks.py:142-150,305 (NCHW). y = conv(x)+bias; a = act(y) if a. */
int cenet_dwconv3x3_nchw_f32(const float* x, long sxb, const float* w, const float* bias, float* y, long syb, float* a,
                             long sab, int B, int C, int H, int W, int dil, int flip, int act, float slope,
                             cenet_stream_t stream);
int cenet_dwconv3x3_tok_f32(const float* x, const float* w, const float* bias, float* y, float* a, int B, int C, int H, int W,
                            int flip, int act, float slope, cenet_stream_t stream);
int cenet_dwconv3x3_wgrad_nchw_acc_f32(const float* x, long sxb, const float* dy, long sgb, float* dw_acc, float* dbias_acc,
                                       int B, int C, int H, int W, int dil, cenet_stream_t stream);
int cenet_dwconv3x3_wgrad_tok_acc_f32(const float* x, const float* dy, float* dw_acc, float* dbias_acc, int B, int C, int H,
                                      int W, cenet_stream_t stream);

/* LayerNorm backward on bf16 rows with DEFERRED affine gradients (round 4): instead of 2 C float atomics per workgroup, each
 * workgroup writes one row of part[cenet_layernorm_bwd_part_rows(rows, C)][2 C]; cenet_ln_fold_group adds the column sums of up to
 * any number of such buffers (all LayerNorms of a backward segment) into their dgamma / dbeta with one launch per 48. */
int cenet_layernorm_bwd_part_rows(int rows, int C);
int cenet_layernorm_bwd_add_part_bf16(const unsigned short* dy, const unsigned short* x, const float* gamma, const float* mean,
                                      const float* rstd, const unsigned short* dx_add, unsigned short* dx, float* part, int rows,
                                      int C, cenet_stream_t stream);
/* the same, also writing dxs = bscale[row / rows_per_sample] * dx: the gradient the DropPath-scaled branch upstream wants
 * (pvtv2.py:141-149) comes out of the kernel that produces dx instead of a scale pass (both NULL: plain) */
int cenet_layernorm_bwd_add_part_scaled_bf16(const unsigned short* dy, const unsigned short* x, const float* gamma,
                                             const float* mean, const float* rstd, const unsigned short* dx_add,
                                             unsigned short* dx, float* part, const float* bscale, int rows_per_sample,
                                             unsigned short* dxs, int rows, int C, cenet_stream_t stream);
int cenet_ln_fold_group(const void* const* part, float* const* dgamma_acc, float* const* dbeta_acc, const int* nrows, const int* C,
                        int n, cenet_stream_t stream);

/* ---- fused PVTv2 MLP half (pvt_mlp.hip) — pvtv2.py:40-47,145-149,364-370 on bf16 tokens [B, H*W, C] --------------------- */
/* y = x + s_b (fc2(GELU(DW3x3(fc1(LayerNorm(x))) + bd)) + b2) in ONE launch: replaces aten::native_layer_norm + addmm +
 * convolution(groups) + gelu + addmm + mul + add.  w1 [HD, C] / w2 [C, HD] are bf16, everything else fp32; bscale [B] (DropPath
 * keep / keep_prob per sample) may be NULL.  xn_out / mean_out / rstd_out / h_out / a_out (all or none): the LayerNorm output
 * and statistics, the fc1 output and s_b * the GELU output, stored for the backward kernels.  CENET_EUNSUPPORTED unless
 * cenet_pvt_mlp_supported(C, HD, H, W) (C in {64, 128}, HD % 64 == 0, W % 14 == 0, H % 7 == 0 or H % 8 == 0). */
int cenet_pvt_mlp_supported(int C, int HD, int H, int W);
int cenet_pvt_mlp_fwd_bf16(const unsigned short* x, const float* ln_g, const float* ln_b, float eps, const unsigned short* w1,
                           const float* b1, const float* wd, const float* bd, const unsigned short* w2, const float* b2,
                           const float* bscale, unsigned short* y, unsigned short* xn_out, float* mean_out, float* rstd_out,
                           unsigned short* h_out, unsigned short* a_out, int B, int H, int W, int C, int HD, cenet_stream_t stream);

/* backward of cenet_pvt_mlp_fwd_bf16 from its saved tensors in two launches (+ a fold of the LayerNorm affine gradients): replaces
 * mul (DropPath scale) + mm (fc2 data gradient) + gelu_backward + convolution_backward(groups) + mm (fc1 data gradient) +
 * native_layer_norm_backward + add (residual).  gu, dh [B, H*W, HD]: the gradient of the depthwise conv's output (scratch) and of
 * fc1's output (operand of the fc1 weight gradient dW1 = dh^T xn; the fc2 weight gradient is dW2 = g^T a with the forward's saved a,
 * which already carries s_b); dx = g + LayerNormBackward(dh . W1); dwd / dbd / dln_g / dln_b and db2 (fc2 bias gradient =
 * column sums of s_b g; may be NULL) are ADDED into.
 * Where the backward rounds: gu = bf16(da * GELU'(DW3x3(h) + bd)) with da = bf16(s_b (g . W2)) — the product with W2 is rounded to
 * bf16 once (s_b applied in fp32 before that rounding) BEFORE the multiply by GELU'.  dwd / dbd accumulate the fp32 product
 * da * GELU' (against the h windows; dbd: its plain sum) BEFORE gu is rounded to bf16, in fp32 and in no fixed order.  dh and dx
 * are computed from gu and dh AS STORED.  GELU' is the bf16 form stated at cenet_dwact_* (the forward's GELU likewise).
 * With up_scale [B] and dxs (both or neither: CENET_EINVAL otherwise), dxs = bf16(up_scale_b * float(dx as stored)).
 * ws: cenet_pvt_mlp_bwd_ws_floats(B, H, W, C) floats. */
long cenet_pvt_mlp_bwd_ws_floats(int B, int H, int W, int C);
/* The tiling both entry points launch with, for tests that pin which code path a shape takes: tile_rows = rows of the 14-column
 * token tile of the forward kernel and of the second backward kernel (dh, dx); k1_tile_rows = rows of the first backward kernel's
 * (gu, dwd, dbd) tile; a workgroup of that kernel walks a run of at most k1_tiles_per_run consecutive tiles of one image and one
 * 64-channel slab, k1_runs runs per image (the last one may be shorter).  Any output pointer may be NULL.  Host only, nothing is
 * launched.  CENET_EUNSUPPORTED where cenet_pvt_mlp_supported(C, HD, H, W) is 0, CENET_EINVAL for B <= 0. */
int cenet_pvt_mlp_bwd_plan(int B, int H, int W, int C, int HD, int* tile_rows, int* k1_tile_rows, int* k1_tiles_per_run,
                           int* k1_runs);
int cenet_pvt_mlp_bwd_bf16(const unsigned short* g, const float* bscale, const unsigned short* w1, const unsigned short* w2,
                           const float* wd, const float* bd, const unsigned short* h, const unsigned short* x, const float* ln_g,
                           const float* mean, const float* rstd, unsigned short* gu, unsigned short* dh, unsigned short* dx,
                           const float* up_scale, unsigned short* dxs, float* dwd_acc, float* dbd_acc, float* dln_g_acc,
                           float* dln_b_acc, float* db2_acc, float* ws, int B, int H, int W, int C, int HD, cenet_stream_t stream);

/* ---- tail of the output head's image branch, fused (res_tail.hip, round 4) — out.py:60,70 over unet.py:201-214 on bf16 maps -------
 * out = w[c] * MaxPool2d(2,2)(LeakyReLU(BN2(x2) + BN3(x3))) with x2 = conv2's output, x3 = the 1x1 shortcut conv's output
 * ([B, C, H, W], H even, W % 8 == 0) and the BatchNorms' batch statistics given (cenet_bn_stats_*): replaces bn_apply x 2 + add +
 * LeakyReLU + max_pool2d + mul forward (one launch; the pre-pool activation is never stored) and max_pool2d_backward +
 * leaky_relu_backward + native_batch_norm_backward x 2 backward (two launches; the activation is recomputed from x2, x3).
 * dgamma / dbeta of both norms and dw (gradient of w) are ADDED into (any may be NULL); ws: cenet_res_tail_bwd_ws_floats(C). */
int cenet_res_tail_supported(int H, int W);
int cenet_res_tail_fwd_bf16(const unsigned short* x2, const unsigned short* x3, const float* mean2, const float* var2,
                            const float* gamma2, const float* beta2, float eps2, const float* mean3, const float* var3,
                            const float* gamma3, const float* beta3, float eps3, const float* w, float slope, unsigned short* out,
                            int B, int C, int H, int W, cenet_stream_t stream);
long cenet_res_tail_bwd_ws_floats(int C);
int cenet_res_tail_bwd_bf16(const unsigned short* g, const unsigned short* x2, const unsigned short* x3, const float* mean2,
                            const float* var2, const float* gamma2, const float* beta2, float eps2, const float* mean3,
                            const float* var3, const float* gamma3, const float* beta3, float eps3, const float* w, float slope,
                            unsigned short* dx2, unsigned short* dx3, float* dgamma2_acc, float* dbeta2_acc, float* dgamma3_acc,
                            float* dbeta3_acc, float* dw_acc, float* ws, int B, int C, int H, int W, cenet_stream_t stream);

/* The same with the shortcut branch NOT materialised (one-channel network input: unet.py conv3 is a 1x1 conv 1 -> C, x3 = w3[c] * img):
 * BN3(x3) is an affine map of the image whose coefficients follow from the image's batch mean / variance (img_mean, img_var: one float
 * each, cenet_bn_stats_* of the [B, 1, H, W] image).  Replaces, besides the above, the shortcut conv, its BatchNorm statistics pass and
 * its weight-gradient kernel.  The forward kernel updates BatchNorm3's running statistics / batch counter (rmean3, rvar3, nbt3, momentum
 * mom3; NULL: not wanted); the backward ADDS dw3 = the shortcut weight's gradient (it reaches the output through eps only). */
int cenet_res_tail_img_fwd_bf16(const unsigned short* x2, const unsigned short* img, const float* mean2, const float* var2,
                                const float* gamma2, const float* beta2, float eps2, const float* img_mean, const float* img_var,
                                const float* w3, const float* gamma3, const float* beta3, float eps3, float* rmean3, float* rvar3,
                                long* nbt3, float mom3, const float* w, float slope, unsigned short* out, int B, int C, int H, int W,
                                cenet_stream_t stream);
int cenet_res_tail_img_bwd_bf16(const unsigned short* g, const unsigned short* x2, const unsigned short* img, const float* mean2,
                                const float* var2, const float* gamma2, const float* beta2, float eps2, const float* img_mean,
                                const float* img_var, const float* w3, const float* gamma3, const float* beta3, float eps3,
                                const float* w, float slope, unsigned short* dx2, float* dgamma2_acc, float* dbeta2_acc,
                                float* dgamma3_acc, float* dbeta3_acc, float* dw3_acc, float* dw_acc, float* ws, int B, int C, int H,
                                int W, cenet_stream_t stream);

/* n <= 4 bias-free, activation-free depthwise 3x3 convs (flip = 1: their data gradients) / weight gradients of bf16 NCHW channel slices
 * in ONE launch — the three dilated SepConvBN branches of a CFAM block (cfam.py:208-212, blocks.py:142-150).  Branch i: x[i] (batch
 * stride sxb[i]) -> y[i] (syb[i]), C[i] channels, dilation dil[i], all on H x W maps of B images.  CENET_EUNSUPPORTED unless every
 * branch takes the plane-in-LDS path (H W % 4 == 0 and the padded plane fits): the caller then launches the branches one by one. */
int cenet_dwconv3x3_nchw_multi_bf16(const unsigned short* const* x, const long* sxb, const float* const* w, unsigned short* const* y,
                                    const long* syb, const int* C, const int* dil, int n, int B, int H, int W, int flip,
                                    cenet_stream_t stream);
int cenet_dwconv3x3_wgrad_nchw_multi_bf16(const unsigned short* const* x, const long* sxb, const unsigned short* const* dy,
                                          const long* sgb, float* const* dw_acc, const int* C, const int* dil, int n, int B, int H,
                                          int W, cenet_stream_t stream);

/* ---- resampling (resample.hip) ---------------------------------------------------------------------------- */
/* aten::upsample_bilinear2d(+_backward) — dseb.py:67-68; cfam.py:217,232; blocks.py:210; out.py:74 */
int cenet_bilinear_fwd_f32(const float* x, long sxb, float* y, long syb, int B, int C, int Hi, int Wi, int Ho, int Wo,
                           float scale_h, float scale_w, int align_corners, cenet_stream_t stream);
int cenet_bilinear_bwd_f32(const float* dy, long sgb, float* dx, long sdb, int B, int C, int Hi, int Wi, int Ho, int Wo,
                           float scale_h, float scale_w, int align_corners, cenet_stream_t stream);
/* dx = backward(dy) + dx_add (laid out like dx): the resampled tensor has further consumers (dseb.py:63-76, 153-160) whose
 * gradients arrive as one addend instead of aten::add launches (round 4) */
int cenet_bilinear_bwd_add_f32(const float* dy, long sgb, float* dx, long sdb, const float* dx_add, int B, int C, int Hi, int Wi,
                               int Ho, int Wo, float scale_h, float scale_w, int align_corners, cenet_stream_t stream);
/* aten::upsample_nearest2d(+_backward) x2 — blocks.py:304 */
int cenet_nearest2x_fwd_f32(const float* x, long sxb, float* y, long syb, int B, int C, int Hi, int Wi, cenet_stream_t stream);
int cenet_nearest2x_bwd_f32(const float* dy, long sgb, float* dx, long sdb, int B, int C, int Hi, int Wi, cenet_stream_t stream);
/* aten::_adaptive_avg_pool2d(+_backward) — cfam.py:213 */
int cenet_adaptive_avgpool_fwd_f32(const float* x, long sxb, float* y, long syb, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                   cenet_stream_t stream);
int cenet_adaptive_avgpool_bwd_f32(const float* dy, long sgb, float* dx, long sdb, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                   cenet_stream_t stream);
/* aten::max_pool2d_with_indices(2,2)(+_backward) fused with the per-channel scale of out.py:70 */
int cenet_maxpool2_fwd_f32(const float* x, float* y, long syb, const float* scale, int B, int C, int Hi, int Wi,
                           cenet_stream_t stream);
int cenet_maxpool2_bwd_acc_f32(const float* x, const float* dy, long sgb, float* dx, const float* scale, float* dscale_acc,
                               int B, int C, int Hi, int Wi, cenet_stream_t stream);

/* ---- CCU / SRM statistics gates (stats.hip) — cfam.py:251-264, 93-101 --------------------------------------- */
int cenet_ccu_stats_fwd_f32(const float* x, const float* fc1, const float* fc2, float* u, int* amax, float* z, int B, int C,
                            int HW, cenet_stream_t stream);
int cenet_gate_chan_fwd_f32(const float* x, const float* g, float* y, int BC, int HW, cenet_stream_t stream);
int cenet_gate_chan_bwd_reduce_f32(const float* x, const float* dy, const float* g, float* dg, int BC, int HW,
                                   cenet_stream_t stream);
int cenet_ccu_bwd_apply_acc_f32(const float* x, const float* dy, const float* g, const float* dz, const float* u,
                                const int* amax, const float* fc1, const float* fc2, float* dfc1_acc, float* dfc2_acc,
                                float* dx, int B, int C, int HW, cenet_stream_t stream);
/* ... + dx_add (like x, may be NULL): the gradient of x's other consumer (the MCA shortcut, cfam.py:298-303), added by the kernel
 * that writes dx (round 4) */
int cenet_ccu_bwd_apply_add_acc_f32(const float* x, const float* dy, const float* g, const float* dz, const float* u,
                                    const int* amax, const float* fc1, const float* fc2, float* dfc1_acc, float* dfc2_acc,
                                    float* dx, const float* dx_add, int B, int C, int HW, cenet_stream_t stream);
int cenet_srm_stats_fwd_f32(const float* x, float* u, int* amax, int B, int C, int HW, cenet_stream_t stream);
int cenet_srm_conv_fwd_f32(const float* u, const float* pwc, const float* dwc, float* f, int B, int H, int W,
                           cenet_stream_t stream);
int cenet_srm_conv_bwd_acc_f32(const float* u, const float* df, const float* pwc, const float* dwc, float* du, float* dpwc_acc,
                               float* ddwc_acc, int B, int H, int W, cenet_stream_t stream);
int cenet_gate_pix_fwd_f32(const float* x, const float* f, float* y, int B, int C, int HW, cenet_stream_t stream);
int cenet_gate_pix_bwd_reduce_f32(const float* x, const float* dy, const float* f, float* df, int B, int C, int HW,
                                  cenet_stream_t stream);
int cenet_srm_bwd_apply_f32(const float* x, const float* dy, const float* f, const float* u, const float* du, const int* amax,
                            float* dx, int B, int C, int HW, cenet_stream_t stream);

/* ---- glue (elementwise.hip) --------------------------------------------------------------------------------- */
int cenet_transpose_f32(const float* x, long sxb, float* y, long syb, int B, int R, int Cc, cenet_stream_t stream);
/* y = x^T + add (add laid out like y, batch stride syb): backward of a layout change whose source has a second consumer
 * (pvtv2.py:320-321: a stage's token output feeds the decoder as NCHW and the next stage's patch embedding as tokens) */
int cenet_transpose_add_f32(const float* x, long sxb, float* y, long syb, const float* add, int B, int R, int Cc,
                            cenet_stream_t stream);
int cenet_copy_batched_f32(const float* x, long sxb, float* y, long syb, int B, long n, int accumulate, cenet_stream_t stream);
/* torch.cat(parts, dim=1) of up to four contiguous NCHW tensors [B, c_j, HW] into joined [B, sum c_j, HW] (split == 0), or
 * its backward: the channel slices of joined copied out into the parts (split == 1) — one launch either way.  Unused
 * trailing parts: pointer NULL, c_j = 0.  Reference call sites: networks/cenet/modules/cfam.py:238 (torch.cat of the four
 * MultiOrderDWConv branches), modules/dseb.py:156, out.py:63. */
int cenet_cat_channels_f32(float* p0, float* p1, float* p2, float* p3, int c0, int c1, int c2, int c3, float* joined, int B,
                           long HW, int split, cenet_stream_t stream);
/* The split with addends (round 4): p_j = channel slice j of joined + a_j (a_j NULL: the slice alone).  Backward of a concat whose
 * inputs have further consumers (dseb.py:156-164: `dec` also feeds decoders.py:96's residual add, `skip` the mixer's residual):
 * the gradients that reached the inputs along those paths are added by this launch instead of one aten::add each. */
int cenet_split_channels_add_f32(float* p0, float* p1, float* p2, float* p3, const float* a0, const float* a1, const float* a2,
                                 const float* a3, int c0, int c1, int c2, int c3, const float* joined, int B, long HW,
                                 cenet_stream_t stream);
/* Add join y = a + b of two equal-shape tensors (modules/dseb.py:156, skip_mode='add': `dec + skip`) and its backward:
 * da = g + ga, db = g + gb in one launch that reads g once (ga / gb NULL: the copy alone).  ga / gb are the gradients that
 * reached a / b through their other consumers (decoders.py:96's residual add, the mixer's `+ skip`). */
int cenet_add2_fwd_f32(const float* a, const float* b, float* y, long n, cenet_stream_t stream);
int cenet_add2_bwd_f32(const float* g, const float* ga, const float* gb, float* da, float* db, long n, cenet_stream_t stream);
/* Space-to-depth of a token map for the kernel == stride spatial-reduction conv (reference networks/cenet/pvtv2.py:93-95,
 * `self.sr = nn.Conv2d(dim, dim, kernel_size=sr_ratio, stride=sr_ratio)` applied to x.permute(0,2,1).reshape(B,C,H,W)):
 * inverse == 0 gathers tok [B, Ho*S, Wo*S, C] into patch rows [B*Ho*Wo, C*S*S] (k = (c, ky, kx), the weight's own order);
 * inverse == 1 scatters patch rows back to the token map (the data gradient). S in {2, 4, 8}. */
int cenet_patch_tok_f32(const float* src, float* dst, int B, int Ho, int Wo, int C, int S, int inverse, cenet_stream_t stream);
/* Overlapping K x K patches of a token-layout map (K = 3; the stride-2 pad-1 patch-embedding convs, pvtv2.py:164):
 * inverse = 0: src tok [B, H*W, C] -> dst rows [B*Ho*Wo, C*K*K] (k = (c, ky, kx), zeros outside the map);
 * inverse = 1: src rows -> dst tok, every pixel summing the row entries that cover it (the conv's data gradient). */
int cenet_im2col_tok_f32(const float* src, float* dst, int B, int H, int W, int C, int K, int stride, int pad, int inverse,
    cenet_stream_t stream);
int cenet_scale_batch_f32(const float* x, const float* s, float* y, int B, long n, cenet_stream_t stream);
int cenet_act_fwd_f32(const float* x, float* y, long n, int act, float slope, cenet_stream_t stream);
int cenet_act_bwd_f32(const float* pre, const float* dy, float* dx, long n, int act, float slope, cenet_stream_t stream);
int cenet_silu_mul_fwd_f32(const float* a, const float* b, float* y, long n, cenet_stream_t stream);
int cenet_silu_mul_bwd_f32(const float* a, const float* b, const float* dy, float* da, float* db, long n, cenet_stream_t stream);
int cenet_mix_fwd_f32(const float* x, const float* p, const float* w, float* z, long n, cenet_stream_t stream);
int cenet_mix_bwd_acc_f32(const float* x, const float* p, const float* w, const float* dz, float* dx, float* dp, float* dw_acc,
                          long n, cenet_stream_t stream);
int cenet_scale_residual_fwd_f32(const float* x, const float* y, const float* ls, float* out, int B, int C, int HW,
                                 cenet_stream_t stream);
int cenet_scale_chan_f32(const float* g, const float* ls, float* out, int B, int C, int HW, cenet_stream_t stream);
int cenet_chan_dot_acc_f32(const float* a, long sab, const float* b, long sbb, float* out_acc, int B, int C, int HW,
                           cenet_stream_t stream);
int cenet_col_sum_acc_f32(const float* a, float* out_acc, long R, int C, cenet_stream_t stream);
int cenet_add_act_fwd_f32(const float* a, const float* b, float* out, long n, int act, float slope, cenet_stream_t stream);
int cenet_lrelu_bwd_from_out_f32(const float* out, const float* dy, float* dx, long n, float slope, cenet_stream_t stream);
/* dseb.py:40-50,63-76,156-163: z = ycoef*y + w[c]*edge(y, r_0..r_{n-1}) + diff*y (r_s NULL = scale 1.0; diff NULL = 0) */
int cenet_dseb_combine_fwd_f32(const float* y, const float* r0, const float* r1, const float* r2, int n, const float* w,
                               const float* diff, float ycoef, float* z, int B, int C, int HW, cenet_stream_t stream);
int cenet_dseb_combine_bwd_acc_f32(const float* y, const float* r0, const float* r1, const float* r2, int n, const float* w,
                                   const float* diff, float ycoef, const float* dz, float* dy, float* dr0, float* dr1, float* dr2,
                                   float* ddiff, float* dw_acc, int B, int C, int HW, cenet_stream_t stream);
/* multihead_diffattn.py:112-123: lambda, A1-lambda*A2 combine, RMSNorm(2hd, eps, no affine), *(1-lambda_init) */
int cenet_diffattn_lambda_fwd_f32(const float* q1, const float* k1, const float* q2, const float* k2, float lambda_init,
                                  float* lam3, int hd, cenet_stream_t stream);
int cenet_diffattn_lambda_bwd_acc_f32(const float* q1, const float* k1, const float* q2, const float* k2, const float* lam3,
                                      const float* dlam, float* dq1, float* dk1, float* dq2, float* dk2, int hd,
                                      cenet_stream_t stream);
int cenet_diffattn_combine_fwd_f32(const float* U, const float* lam3, float* out, int B, int H, int N, int dv, float eps,
                                   float post, cenet_stream_t stream);
int cenet_diffattn_combine_bwd_acc_f32(const float* U, const float* lam3, const float* dout, float* dU, float* dlam_acc, int B,
                                       int H, int N, int dv, float eps, float post, cenet_stream_t stream);

/* ---- loss + optimiser (loss_optim.hip) ---------------------------------------------------------------------- */
/* utils/core.py:44-80,161-188: loss = w_dice*Dice(softmax(logits), onehot(labels)) + w_ce*CE.
 * acc: CENET_LOSS_ACC_FLOATS floats of workspace (replicated partial sums); its first 3K+1 floats are what bwd reads. */
#define CENET_LOSS_ACC_FLOATS 16384
int cenet_dice_ce_fwd_f32(const float* logits, const float* labels, float* acc, float* loss, int B, int K, int HW, float w_dice,
                          float w_ce, cenet_stream_t stream);
int cenet_dice_ce_bwd_f32(const float* logits, const float* labels, const float* acc, const float* gout, float* dlogits, int B,
                          int K, int HW, float w_dice, float w_ce, cenet_stream_t stream);
/* The same with BoundaryDoULoss (utils/core.py:83-131, the loss of scripts/acdc.sh:63 / synapse.sh:67) as a third term:
 * loss = w_dice*Dice + w_ce*CE + w_bd*BoundaryDoU; labels [B,H,W] (class ids as floats). */
int cenet_seg_loss_fwd_f32(const float* logits, const float* labels, float* acc, float* loss, int B, int K, int H, int W,
                           float w_dice, float w_ce, float w_bd, cenet_stream_t stream);
int cenet_seg_loss_bwd_f32(const float* logits, const float* labels, const float* acc, const float* gout, float* dlogits,
                           int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, cenet_stream_t stream);
/* The loss with options (seg_loss_ex.hip): per-class weights, ignore_index, a Jaccard term (utils/core.py:134-158 with the
 * `flatten` of utils/utils.py:39-50) and DiceLoss(softmax=False) (core.py:67-80).  With M = [label != ignore_index] (1 everywhere
 * unless has_ignore), t_c = [label == c] M and sums over the whole batch, I_c = sum M p_c t_c, Z_c = sum M p_c^2, Y_c = sum t_c,
 * S_c = sum M p_c:
 *   loss = w_dice/K sum_c wd_c (1 - (2 I_c + 1e-5) / (Z_c + Y_c + 1e-5))  +  w_ce sum_pix wc_t (-log p_t) / sum_pix wc_t
 *        + w_bd BoundaryDoU  +  w_jac/K sum_c (1 - (I_c + smooth) / (S_c + Y_c - I_c + smooth)).
 * A term whose weight is 0 is left out (not multiplied by 0): the CE of a batch whose every pixel is ignored is NaN, as torch's.
 * cw: [2K] floats, the Dice class weights wd then the CE class weights wc, read on the device by every launch (NULL: all ones).
 * Labels are in [0,K) or equal ignore_index.  from_probs: `logits` already holds the probabilities (no softmax either way);
 * Dice term only, anything else returns 1.  has_ignore with w_bd != 0 returns 2 (a boundary count over a mask with holes is
 * not defined by the reference).  The gradient of an ignored pixel is exactly 0.
 * ws: workspace of ws_floats >= cenet_seg_loss_ex_ws_floats(B, K, H, W) floats, else 1 is returned.  No float atomics: each
 * workgroup of the forward stores one row of partial sums, a one-workgroup second launch adds the rows in a fixed order and
 * leaves the compact sums at the head of ws for the backward call — bitwise reproducible.  K <= 16, B <= 65535. */
long cenet_seg_loss_ex_ws_floats(int B, int K, int H, int W);
int cenet_seg_loss_ex_fwd_f32(const float* logits, const float* labels, const float* cw, float* ws, long ws_floats, float* loss,
                              int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac, float smooth,
                              int has_ignore, int ignore_index, int from_probs, cenet_stream_t stream);
int cenet_seg_loss_ex_bwd_f32(const float* logits, const float* labels, const float* cw, const float* ws, const float* gout,
                              float* dlogits, int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac,
                              float smooth, int has_ignore, int ignore_index, int from_probs, cenet_stream_t stream);
/* Evaluation (main_acdc.py:218-231 val(), metrics_eval.py:24-34,46-49): pred[B,HW] = argmax over the K
 * logit planes (class ids as floats, may be NULL), counts[(K+1)*3] (uint32, zero-filled by the call; may be NULL together with
 * labels) = per class {|pred==c & gt==c|, |pred==c|, |gt==c|} and, in row K, the same for the binary masks pred>0 / gt>0. */
int cenet_argmax_counts_f32(const float* logits, const float* labels, float* pred, unsigned* counts, int B, int K, int HW,
                            cenet_stream_t stream);
/* Surface-distance metrics of metrics_eval.py:9-21 (`calculate_metric_percase`: medpy.metric.binary.hd95 / assd, medpy==0.5.2,
 * requirements.txt:7; medpy is a third-party dependency absent from the reference tree, its published algorithm is restated).
 * border[D*H*W] = mask XOR binary_erosion(mask) with the 6-neighbourhood and background outside the volume (0/1 bytes). */
int cenet_surface_border_u8(const unsigned char* mask, unsigned char* border, int D, int H, int W, cenet_stream_t stream);
/* out[i] = min(out[i], min_j |a_i - b_j|^2): a [na,3], b [nb,3] int32 voxel coordinates (z,y,x), unit spacing as the
 * reference's calls use; out [na] int32 pre-filled by the caller with INT_MAX. The distance transform of medpy's
 * __surface_distances sampled at the other surface, kept in exact integer arithmetic (host takes the square root). */
int cenet_min_sqdist_i32(const int* a, int na, const int* b, int nb, int* out, cenet_stream_t stream);
/* The same distances by an exact distance transform (csrc/edt.hip): linear in the number of voxels instead of quadratic in the
 * border sizes.  d2[v] = min over feature voxels f of |v - f|^2 for a uint8 volume [D,H,W], unit spacing, int32, exact.  A voxel
 * is a feature when it is non-zero (match < 0) or equals `match` (0..255).  tmp and d2: D*H*W int32 each; the result is in d2,
 * INT_MAX everywhere when there is no feature voxel.  CENET_EINVAL unless D^2 + H^2 + W^2 < 2^31. */
int cenet_edt_sq_u8(const unsigned char* feat, int match, int* tmp, int* d2, int D, int H, int W, cenet_stream_t stream);
/* One pass over two label volumes (class ids as float, anything that is not an integer in [1, K) is background): border_pred /
 * border_gt [D*H*W] = the voxel's class where it is a border voxel of that class (a face neighbour differs or lies outside;
 * zfaces = 0 leaves the z neighbours out: medpy's rule for a 2-D mask, passed as D = 1), else 0.  table [K, CENET_LB_COLS] int32,
 * row c: |pred==c & gt==c|, |pred==c|, |gt==c|, |border pred|, |border gt|, then per border min z, y, x and min -z, -y, -x.
 * The caller zeroes columns 0-4 and fills the rest with INT_MAX.  2 <= K <= 64. */
#define CENET_LB_COLS 17
int cenet_label_borders_f32(const float* pred, const float* gt, unsigned char* border_pred, unsigned char* border_gt, int* table,
                            int K, int D, int H, int W, int zfaces, cenet_stream_t stream);
/* Order-preserving compaction of the voxels of bl [n] that equal `match`, in two launches: counts[b] = matches among the voxels
 * [4096 b, 4096 b + 4096); then, with offs = the exclusive prefix sum of counts, out[rank] = src[voxel] (src != NULL) or
 * out[3 rank ..] = (z, y, x) of the voxel (src == NULL), rank in C order. */
int cenet_border_count_u8(const unsigned char* bl, int match, long n, int* counts, cenet_stream_t stream);
int cenet_border_gather_i32(const unsigned char* bl, int match, int D, int H, int W, const int* offs, const int* src, int* out,
                            cenet_stream_t stream);
/* The surface distances with a voxel spacing (sz, sy, sx), in fp64 (medpy's `voxelspacing`, scipy's `sampling`):
 * d2[v] = min over feature voxels f of sz^2 (vz-fz)^2 + sy^2 (vy-fy)^2 + sx^2 (vx-fx)^2.
 * cenet_edt_sq_spaced_u8: the transform of cenet_edt_sq_u8 with that metric.  xd: D*H*W int32 of scratch (the integer x pass), tmp
 * and d2: D*H*W doubles each; the result is in d2, +inf everywhere when there is no feature voxel.  With sy == sx the y pass is the
 * integer one too and the value is sz^2 dz^2 + sx^2 (dy^2 + dx^2), else sz^2 dz^2 + (sy^2 dy^2 + sx^2 dx^2).  Every product and sum is exact
 * when the spacings are dyadic and the volume small enough for 53 bits; no atomics, the same bits on every run.
 * cenet_min_sqdist_spaced_f64: the all-pairs minimum of cenet_min_sqdist_i32 with that metric, the three terms summed as
 * (z + y) + x; out [na] doubles, written (not merged into).  No atomics: the slices of b write partial minima into ws
 * (ws_doubles >= cenet_min_sqdist_spaced_ws_doubles(na, nb) doubles, which is 0 when b is not split: ws may be NULL then) and a
 * second launch takes their minimum.
 * cenet_border_gather_f64: cenet_border_gather_i32 for a source of doubles (src must not be NULL).
 * CENET_EINVAL (nothing launched) for a spacing that is not positive and finite (or whose square is not), and for the shapes the
 * unspaced entry points refuse. */
int cenet_edt_sq_spaced_u8(const unsigned char* feat, int match, int* xd, double* tmp, double* d2, int D, int H, int W, double sz,
                           double sy, double sx, cenet_stream_t stream);
long cenet_min_sqdist_spaced_ws_doubles(int na, int nb);
int cenet_min_sqdist_spaced_f64(const int* a, int na, const int* b, int nb, double sz, double sy, double sx, double* ws,
                                long ws_doubles, double* out, cenet_stream_t stream);
int cenet_border_gather_f64(const unsigned char* bl, int match, int D, int H, int W, const int* offs, const double* src,
                            double* out, cenet_stream_t stream);
/* Connected components of a label volume (csrc/ccl.hip; a post-processing step, not in the reference).  labels [D,H,W]: class ids
 * as float, anything that is not an integer in [1, K) is background.  Two voxels are linked when they are neighbours and carry the
 * same class; connectivity 1 / 2 / 3 = 6 / 18 / 26 neighbours (scipy.ndimage.generate_binary_structure(3, connectivity)), zlinks
 * = 0 leaves out every neighbour with a z offset (per-slice 2-D labelling, connectivity 1 or 2 only).  roots [D*H*W] int32: the
 * smallest linear index z H W + y W + x of the voxel's component, -1 for background — the same bits on every run.
 * CENET_EINVAL (nothing launched) unless 2 <= K <= 64, D, H, W > 0, D*H*W < 2^31, 1 <= connectivity <= 3 and, with zlinks = 0,
 * connectivity <= 2. */
int cenet_ccl_label_f32(const float* labels, int* roots, int K, int D, int H, int W, int connectivity, int zlinks,
                        cenet_stream_t stream);
/* sizes [n] int32, zeroed by the call: sizes[r] = voxels of the component with root r (roots as cenet_ccl_label_f32 writes them),
 * 0 at every voxel that is no root.  CENET_EINVAL unless 0 < n < 2^31. */
int cenet_ccl_sizes_i32(const int* roots, int* sizes, long n, cenet_stream_t stream);
/* Keep the largest component of every class — with zlinks = 0 of every (slice, class) — and drop the others: out [D*H*W] = the
 * voxel's class where its component is the selected one or, when min_size > 0, has at least min_size voxels; 0 elsewhere.  Among
 * components of equal size the one with the smaller root is selected.  table [K, 3] int32, zeroed by the call: per class the
 * components found, the voxels kept, the voxels removed.  ws: ws_ints >= cenet_ccl_ws_ints(K, D, zlinks) ints of scratch, filled by
 * the call.  labels, K, D, H, W, zlinks as given to cenet_ccl_label_f32 for these roots.  CENET_EINVAL (nothing launched) for a
 * shape that call refuses, a workspace that is too small, min_size < 0, or out == labels. */
long cenet_ccl_ws_ints(int K, int D, int zlinks);
int cenet_ccl_keep_f32(const float* labels, const int* roots, const int* sizes, int* ws, long ws_ints, float* out, int* table,
                       int K, int D, int H, int W, int zlinks, int min_size, cenet_stream_t stream);
/* Boundary-distance maps for the distance-map losses (csrc/edt.hip; not in the reference).  For every image b and foreground class
 * c = 1 .. K-1 the plane (b, c) has a mask M: {label == c} for the labels [B,H,W] (class ids as floats), {softmax_c > 1/2} for the
 * logits [B,K,H,W] (the threshold is taken in fp32 from the logits, no probability is stored).  d2 [B, K-1, H, W] int32:
 * the squared Euclidean distance, unit spacing, exact, from the pixel to the nearest pixel of the OTHER kind — the nearest pixel
 * outside M for a pixel of M, the nearest pixel of M otherwise (scipy: distance_transform_edt(M)^2 + distance_transform_edt(~M)^2).
 * A plane whose M is empty or the whole plane is 0 everywhere.  Integer arithmetic only, no atomics: the same bits on every run;
 * nothing is read back.  ws: ws_ints >= cenet_dist_maps_ws_ints(B, K, H, W) ints of scratch.  CENET_EINVAL (nothing launched)
 * unless 2 <= K <= 16, B, H, W >= 1, 2 B (K-1) <= 65535, H^2 + W^2 < 2^31 and the workspace is large enough. */
long cenet_dist_maps_ws_ints(int B, int K, int H, int W);
int cenet_dist_maps_labels_f32(const float* labels, int* ws, long ws_ints, int* d2, int B, int K, int H, int W,
                               cenet_stream_t stream);
int cenet_dist_maps_logits_f32(const float* logits, int* ws, long ws_ints, int* d2, int B, int K, int H, int W,
                               cenet_stream_t stream);
/* The distance-map losses on those maps (csrc/dist_loss.hip): the surface (boundary) loss of Kervadec et al. 2019 and the
 * Hausdorff-DT loss of Karimi & Salcudean 2019 with alpha = 2.  With N = B (K-1) H W, p = softmax(logits) over the K planes,
 * g_c = [label == c], d2g / d2p the maps of the labels / of the logits, and sums over b, c = 1 .. K-1 and the pixels:
 *   phi_c  = +sqrt(d2g_c) outside class c, -(sqrt(d2g_c) - 1) inside      (the signed distance of Kervadec's one_hot2dist)
 *   L_surf = 1/N sum p_c phi_c
 *   L_hd   = 1/N sum (p_c - g_c)^2 (d2g_c + d2p_c)                        (d2p is a constant: no gradient through the threshold)
 *   loss   = w[0] L_surf + w[1] L_hd
 * w: two floats in device memory, read by the kernels of every launch.  surface / hausdorff: which terms are present (one at
 * least); a term that is absent is left out, and without the Hausdorff term d2p is not read (may be NULL).  Forward: one pass that
 * stores a row of two partial sums per workgroup in ws (ws_floats >= cenet_dist_loss_ws_floats(B, K, H, W)) and a one-workgroup
 * launch that adds the rows in a fixed order — no float atomics, bitwise reproducible.  Backward: with a_0 = 0 and
 * a_j = w[0] phi_j + 2 w[1] (p_j - g_j)(d2g_j + d2p_j),  dlogits_j = gout[0] p_j (a_j - sum_c p_c a_c) / N.
 * CENET_EINVAL unless 2 <= K <= 16, 1 <= B <= 65535, H, W >= 1. */
long cenet_dist_loss_ws_floats(int B, int K, int H, int W);
int cenet_dist_loss_fwd_f32(const float* logits, const float* labels, const int* d2g, const int* d2p, const float* w, float* ws,
                            long ws_floats, float* loss, int B, int K, int H, int W, int surface, int hausdorff,
                            cenet_stream_t stream);
int cenet_dist_loss_bwd_f32(const float* logits, const float* labels, const int* d2g, const int* d2p, const float* w,
                            const float* gout, float* dlogits, int B, int K, int H, int W, int surface, int hausdorff,
                            cenet_stream_t stream);
/* The Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018, Alg. 1; csrc/lovasz.hip; not in the reference).  inputs [B,K,H,W]
 * logits, or probabilities with from_probs; labels [B,H,W] class ids as floats.  p = softmax(inputs) over K in fp32 (from_probs:
 * p = inputs), g = [label == c], e = |g - p_c| in fp32.  A SEGMENT is one class over all n = B H W pixels (S = K segments) or, with
 * per_image, one (image, class) with n = H W (S = B K).  Inside a segment the pixels are ordered by descending e, equal e by
 * ascending pixel index (b, h, w): a stable descending sort, so the result is a function of the inputs alone.  All counts are
 * integers: G = pixels with g = 1 in the segment; at sorted position i (from 0) F_i = those among positions 0 .. i, Z_i = the
 * g = 0 among them, I_i = G - F_i, U_i = G + Z_i, J_i = 1 - I_i / U_i, J_{-1} = 0.  The increment J_i - J_{i-1} is evaluated as
 *   1 / U_i  (g = 1)       I_i / (U_i (U_i - 1))  (g = 0)       1  (U_i = 1: i = 0 in a segment with G = 0)
 * from the integers, never as a difference of two numbers near 1.  Segment loss L = sum_i e_(i) (J_i - J_{i-1});
 *   loss = the mean of L over the segments with G > 0 (classes_all: over all K), with per_image per image, then over the B images
 * (the divisor is computed on the device; no segment that counts: 0).  coef [B,K,H,W] fp32 = a = dloss / dp_c(x) =
 * s (J_i - J_{i-1}) / divisor, s = -1 for g = 1, +1 for g = 0, 0 where e == 0 exactly (the gradient of |.|).  has_ignore: a pixel
 * whose label is ignore_index is in no class and no count, sorts below every other pixel and has a = 0.
 * Forward: keys (bits of e, + 1; 0 = ignored) and payloads (pixel index, g bit), a batched stable LSD radix sort over the segments
 * (8 bits a pass, tiles of cenet_lovasz_tile() elements, ranks inside a tile by ballots: no atomic decides an order), an integer
 * scan of the g bits along the sorted order (G is that scan's total over the segment: the keys pass counts nothing), the
 * coefficients, one partial sum per workgroup stored in ws and a one-workgroup launch
 * that adds them in a fixed order — no float atomics, bitwise reproducible.  ws: ws_bytes >= cenet_lovasz_ws_bytes(B, K, H, W,
 * per_image) bytes of scratch, 4-byte aligned.  Backward, one launch: dinputs_j = gout[0] p_j (a_j - sum_c p_c a_c), from_probs:
 * gout[0] a_j; dinputs may not be inputs.  CENET_EINVAL (nothing launched) unless 2 <= K <= 16, B, H, W >= 1, S <= 65535,
 * n < 2^31 and the workspace is large enough.
 * cenet_lovasz_order_f32 is the sort alone: errors [S, n] fp32, non-negative -> perm [S, n] int32, perm[s][i] = the index in
 * segment s of the element at sorted position i (numpy: argsort(-e, kind="stable")); ws_bytes >= cenet_lovasz_order_ws_bytes(S, n);
 * CENET_EINVAL unless 1 <= S <= 65535 and 1 <= n < 2^31. */
int cenet_lovasz_tile(void);
long cenet_lovasz_ws_bytes(int B, int K, int H, int W, int per_image);
long cenet_lovasz_order_ws_bytes(int S, int n);
int cenet_lovasz_order_f32(const float* errors, void* ws, long ws_bytes, int* perm, int S, int n, cenet_stream_t stream);
int cenet_lovasz_fwd_f32(const float* inputs, const float* labels, void* ws, long ws_bytes, float* coef, float* loss, int B, int K,
                         int H, int W, int per_image, int classes_all, int has_ignore, int ignore_index, int from_probs,
                         cenet_stream_t stream);
int cenet_lovasz_bwd_f32(const float* inputs, const float* coef, const float* gout, float* dinputs, int B, int K, int H, int W,
                         int from_probs, cenet_stream_t stream);
/* Top-k cross-entropy: the mean of the cross-entropy over the k % of pixels with the largest loss (hard-pixel mining, the CE half
 * of nnU-Net's DC_and_topk_loss; csrc/topk_ce.hip; not in the reference).  logits [B,K,H,W], 2 <= K <= 16; labels [B,H,W] class
 * ids as floats.  For pixel i, l_i = log sum_c exp(x_c - max) - (x_y - max) in fp32, clamped at >= 0.  The label picks x_y by the
 * comparison label == (float)c and is never a memory index.  A pixel whose label is ignore_index (has_ignore), or matches no
 * class, is INVALID: in no count, zero gradient.  A SEGMENT is the whole batch (S = 1, n = B H W) or, with per_image, one image
 * (S = B, n = H W); n_valid = its valid pixels; m = max(1, floor(n_valid k / 100)) with k = kpercent[0], a float32 percentage READ
 * ON THE DEVICE and clamped into (0, 100], the product and quotient in double: (long long)((double)n_valid * (double)k / 100.0).
 * The kept set of a segment is its m valid pixels with the largest l, equal l by ascending pixel index (numpy:
 * argsort(-l, kind="stable")[:m]).  Segment loss = the mean of l over the kept set; loss = the mean over the S_valid segments
 * that have a valid pixel; no valid pixel in the batch: loss = 0 exactly, gradient all zeros.  wgt [B,H,W] fp32 = 1 / (m_s S_valid)
 * on a kept pixel, 0 elsewhere.  Backward, one launch: dlogits_j = gout[0] wgt_i (p_j - [j == y_i]), exact zeros where wgt_i == 0;
 * dlogits may not be logits.  Non-finite logits are outside the contract (unspecified result, no fault: nothing is indexed by a
 * value).
 * Forward: keys (bits of l, + 1; 0 = invalid) as [S, n] uint32 with the first digit histogram and n_valid in the same pass; a
 * radix SELECT of 4 rounds of 8 bits from the top (a histogram of the digit over the keys whose higher bits equal the prefix so
 * far — LDS bins per workgroup, integer atomics into the segment's 256 bins: counts only —, then one workgroup a segment picks
 * the digit at which the count from the top reaches the remaining quota) that leaves the threshold key tau and r, the number of
 * pixels with key == tau that are kept (no key moves); the tie rank (key == tau per tile of cenet_topk_tile() elements, an
 * exclusive scan over the tiles, ballots and the lane number inside a tile: no atomic decides an order); kept iff key > tau, or
 * key == tau and rank < r; one partial sum of the kept l per workgroup stored in ws and a one-workgroup launch that adds them in a
 * fixed order in double — no float atomics, bitwise reproducible, nothing read back.  ws: ws_bytes >= cenet_topk_ce_ws_bytes(B,
 * H, W, per_image) bytes of scratch, 4-byte aligned.  CENET_EINVAL (nothing launched) unless 2 <= K <= 16, B, H, W >= 1,
 * S <= 65535, n < 2^31 and the workspace is large enough.
 * cenet_topk_mask_f32 is the selection alone: values [S, n] fp32, non-negative; m [S] int32 (device; clamped into [0, n]) ->
 * mask [S, n] uint8 = 1 on the m[s] largest values of segment s, equal values by ascending index; ws_bytes >=
 * cenet_topk_mask_ws_bytes(S, n); CENET_EINVAL unless 1 <= S <= 65535 and 1 <= n < 2^31. */
int cenet_topk_tile(void);
long cenet_topk_ce_ws_bytes(int B, int H, int W, int per_image);
long cenet_topk_mask_ws_bytes(int S, int n);
int cenet_topk_mask_f32(const float* values, const int* m, void* ws, long ws_bytes, unsigned char* mask, int S, int n,
                        cenet_stream_t stream);
int cenet_topk_ce_fwd_f32(const float* logits, const float* labels, const float* kpercent, void* ws, long ws_bytes, float* wgt,
                          float* loss, int B, int K, int H, int W, int per_image, int has_ignore, int ignore_index,
                          cenet_stream_t stream);
int cenet_topk_ce_bwd_f32(const float* logits, const float* labels, const float* wgt, const float* gout, float* dlogits, int B,
                          int K, int H, int W, int has_ignore, int ignore_index, cenet_stream_t stream);
/* torch.optim.SGD(momentum, weight_decay) over a flat arena; hyper5 (device) = [lr, momentum, wd, grad_scale, first_step] */
int cenet_sgd_step_f32(float* p, const float* g, float* buf, const float* hyper5, long n, cenet_stream_t stream);
/* torch.optim.Adam / AdamW (amsgrad off) over a flat arena, one pass; exp_avg / exp_avg_sq are the flat fp32 moment buffers.
 * hyper12 (device) = [lr, beta1, beta2, eps, wd, grad_scale, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t),
 * decoupled (AdamW) flag, 1 - beta1, 1 - beta2, 1 - lr wd], the derived values computed on the host in double.  The _shadow form
 * also rewrites the bf16 shadow of the parameters (as cenet_sgd_step_shadow_f32). */
int cenet_adam_step_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, const float* hyper12, long n,
                        cenet_stream_t stream);
int cenet_adam_step_shadow_f32(float* p, const float* g, float* exp_avg, float* exp_avg_sq, const float* hyper12, long n,
                               unsigned short* shadow_bf16, cenet_stream_t stream);
int cenet_zero_f32(float* p, long n, cenet_stream_t stream);
/* zero-fill of any byte range (bf16 activations with an odd element count, views starting on an odd element): the buffers
 * torch.zeros / Tensor.zero_() would give the reference's autograd (e.g. the absent branch of a channel split) */
int cenet_zero_bytes(void* p, long nbytes, cenet_stream_t stream);

/* ---- bf16 twins (throughput mode) ------------------------------------------------------------------------------------
 * Every `cenet_<op>_f32` entry point above that takes ACTIVATION tensors has a twin `cenet_<op>_bf16` with the same
 * semantics and argument order in which the activation / activation-gradient pointers are bf16 (`unsigned short`, bf16 bit
 * patterns) while parameters, statistics (mean / rstd / var / lse / u / z / f ...), workspaces and parameter gradients stay
 * fp32.  Arithmetic is fp32 in both; the reference sites are those of the fp32 declaration.  (GEMM, attention, direct conv
 * and row softmax declare their bf16 forms next to the fp32 ones.) */
/* attn.hip */
int cenet_softmax_rows_fwd_bf16(const float* x, unsigned short* y, long rows, int n, cenet_stream_t stream);
int cenet_softmax_rows_bwd_bf16(const unsigned short* y, const float* dy, unsigned short* dx, long rows, int n,
    cenet_stream_t stream);
/* dwconv.hip */
int cenet_dwconv3x3_nchw_bf16(const unsigned short* x, long sxb, const float* w, const float* bias, unsigned short* y, long
    syb, unsigned short* a, long sab, int B, int C, int H, int W, int dil, int flip, int act, float slope, cenet_stream_t
    stream);
int cenet_dwconv3x3_tok_bf16(const unsigned short* x, const float* w, const float* bias, unsigned short* y, unsigned short*
    a, int B, int C, int H, int W, int flip, int act, float slope, cenet_stream_t stream);
int cenet_dwconv3x3_wgrad_nchw_acc_bf16(const unsigned short* x, long sxb, const unsigned short* dy, long sgb, float*
    dw_acc, float* dbias_acc, int B, int C, int H, int W, int dil, cenet_stream_t stream);
int cenet_dwconv3x3_wgrad_tok_acc_bf16(const unsigned short* x, const unsigned short* dy, float* dw_acc, float* dbias_acc,
    int B, int C, int H, int W, cenet_stream_t stream);
/* backward of act(DW3x3(x) + bias) on bf16 tokens from the saved INPUT (pvtv2.py:42-43,359-370; the pre-activation is not
 * stored): gu = g * act'(conv(x) + bias), dw_acc += gu (*) x, dbias_acc += sum gu.  C % 8 == 0, 16-byte aligned tensors. */
int cenet_dwconv3x3_tok_bwd_pre_bf16(const unsigned short* x, const unsigned short* g, const float* w, const float* bias,
    unsigned short* gu, float* dw_acc, float* dbias_acc, int B, int C, int H, int W, int act, float slope,
    cenet_stream_t stream);
/* elementwise.hip */
int cenet_transpose_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, int B, int R, int Cc,
    cenet_stream_t stream);
int cenet_transpose_add_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, const unsigned short* add, int B,
    int R, int Cc, cenet_stream_t stream);
int cenet_copy_batched_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, int B, long n, int accumulate,
    cenet_stream_t stream);
int cenet_cat_channels_bf16(unsigned short* p0, unsigned short* p1, unsigned short* p2, unsigned short* p3, int c0, int c1,
    int c2, int c3, unsigned short* joined, int B, long HW, int split, cenet_stream_t stream);
int cenet_split_channels_add_bf16(unsigned short* p0, unsigned short* p1, unsigned short* p2, unsigned short* p3,
    const unsigned short* a0, const unsigned short* a1, const unsigned short* a2, const unsigned short* a3, int c0, int c1, int c2,
    int c3, const unsigned short* joined, int B, long HW, cenet_stream_t stream);
int cenet_add2_fwd_bf16(const unsigned short* a, const unsigned short* b, unsigned short* y, long n, cenet_stream_t stream);
int cenet_add2_bwd_bf16(const unsigned short* g, const unsigned short* ga, const unsigned short* gb, unsigned short* da,
    unsigned short* db, long n, cenet_stream_t stream);
int cenet_patch_tok_bf16(const unsigned short* src, unsigned short* dst, int B, int Ho, int Wo, int C, int S, int inverse,
    cenet_stream_t stream);
int cenet_im2col_tok_bf16(const unsigned short* src, unsigned short* dst, int B, int H, int W, int C, int K, int stride,
    int pad, int inverse, cenet_stream_t stream);
int cenet_scale_batch_bf16(const unsigned short* x, const float* s, unsigned short* y, int B, long n, cenet_stream_t
    stream);
int cenet_act_fwd_bf16(const unsigned short* x, unsigned short* y, long n, int act, float slope, cenet_stream_t stream);
int cenet_act_bwd_bf16(const unsigned short* pre, const unsigned short* dy, unsigned short* dx, long n, int act, float
    slope, cenet_stream_t stream);
int cenet_silu_mul_fwd_bf16(const unsigned short* a, const unsigned short* b, unsigned short* y, long n, cenet_stream_t
    stream);
int cenet_silu_mul_bwd_bf16(const unsigned short* a, const unsigned short* b, const unsigned short* dy, unsigned short* da,
    unsigned short* db, long n, cenet_stream_t stream);
int cenet_mix_fwd_bf16(const unsigned short* x, const unsigned short* p, const float* w, unsigned short* z, long n,
    cenet_stream_t stream);
int cenet_mix_bwd_acc_bf16(const unsigned short* x, const unsigned short* p, const float* w, const unsigned short* dz,
    unsigned short* dx, unsigned short* dp, float* dw_acc, long n, cenet_stream_t stream);
int cenet_scale_residual_fwd_bf16(const unsigned short* x, const unsigned short* y, const float* ls, unsigned short* out,
    int B, int C, int HW, cenet_stream_t stream);
int cenet_scale_chan_bf16(const unsigned short* g, const float* ls, unsigned short* out, int B, int C, int HW,
    cenet_stream_t stream);
int cenet_chan_dot_acc_bf16(const unsigned short* a, long sab, const unsigned short* b, long sbb, float* out_acc, int B, int
    C, int HW, cenet_stream_t stream);
int cenet_col_sum_acc_bf16(const unsigned short* a, float* out_acc, long R, int C, cenet_stream_t stream);
int cenet_add_act_fwd_bf16(const unsigned short* a, const unsigned short* b, unsigned short* out, long n, int act, float
    slope, cenet_stream_t stream);
int cenet_lrelu_bwd_from_out_bf16(const unsigned short* out, const unsigned short* dy, unsigned short* dx, long n, float
    slope, cenet_stream_t stream);
int cenet_dseb_combine_fwd_bf16(const unsigned short* y, const unsigned short* r0, const unsigned short* r1, const unsigned
    short* r2, int n, const float* w, const unsigned short* diff, float ycoef, unsigned short* z, int B, int C, int HW,
    cenet_stream_t stream);
int cenet_dseb_combine_bwd_acc_bf16(const unsigned short* y, const unsigned short* r0, const unsigned short* r1, const
    unsigned short* r2, int n, const float* w, const unsigned short* diff, float ycoef, const unsigned short* dz, unsigned
    short* dy, unsigned short* dr0, unsigned short* dr1, unsigned short* dr2, unsigned short* ddiff, float* dw_acc, int B,
    int C, int HW, cenet_stream_t stream);
int cenet_diffattn_combine_fwd_bf16(const unsigned short* U, const float* lam3, unsigned short* out, int B, int H, int N,
    int dv, float eps, float post, cenet_stream_t stream);
int cenet_diffattn_combine_bwd_acc_bf16(const unsigned short* U, const float* lam3, const unsigned short* dout, unsigned
    short* dU, float* dlam_acc, int B, int H, int N, int dv, float eps, float post, cenet_stream_t stream);
/* loss_optim.hip */
int cenet_seg_loss_fwd_bf16(const unsigned short* logits, const float* labels, float* acc, float* loss, int B, int K, int H,
    int W, float w_dice, float w_ce, float w_bd, cenet_stream_t stream);
int cenet_seg_loss_bwd_bf16(const unsigned short* logits, const float* labels, const float* acc, const float* gout, unsigned
    short* dlogits, int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, cenet_stream_t stream);
int cenet_argmax_counts_bf16(const unsigned short* logits, const float* labels, float* pred, unsigned* counts, int B, int K,
    int HW, cenet_stream_t stream);
/* seg_loss_ex.hip */
int cenet_seg_loss_ex_fwd_bf16(const unsigned short* logits, const float* labels, const float* cw, float* ws, long ws_floats,
    float* loss, int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac, float smooth, int has_ignore,
    int ignore_index, int from_probs, cenet_stream_t stream);
int cenet_seg_loss_ex_bwd_bf16(const unsigned short* logits, const float* labels, const float* cw, const float* ws, const float*
    gout, unsigned short* dlogits, int B, int K, int H, int W, float w_dice, float w_ce, float w_bd, float w_jac, float smooth,
    int has_ignore, int ignore_index, int from_probs, cenet_stream_t stream);
/* edt.hip, dist_loss.hip */
int cenet_dist_maps_logits_bf16(const unsigned short* logits, int* ws, long ws_ints, int* d2, int B, int K, int H, int W,
    cenet_stream_t stream);
int cenet_dist_loss_fwd_bf16(const unsigned short* logits, const float* labels, const int* d2g, const int* d2p, const float* w,
    float* ws, long ws_floats, float* loss, int B, int K, int H, int W, int surface, int hausdorff, cenet_stream_t stream);
int cenet_dist_loss_bwd_bf16(const unsigned short* logits, const float* labels, const int* d2g, const int* d2p, const float* w,
    const float* gout, unsigned short* dlogits, int B, int K, int H, int W, int surface, int hausdorff, cenet_stream_t stream);
/* lovasz.hip */
int cenet_lovasz_fwd_bf16(const unsigned short* inputs, const float* labels, void* ws, long ws_bytes, float* coef, float* loss,
    int B, int K, int H, int W, int per_image, int classes_all, int has_ignore, int ignore_index, int from_probs,
    cenet_stream_t stream);
int cenet_lovasz_bwd_bf16(const unsigned short* inputs, const float* coef, const float* gout, unsigned short* dinputs, int B,
    int K, int H, int W, int from_probs, cenet_stream_t stream);
/* topk_ce.hip */
int cenet_topk_ce_fwd_bf16(const unsigned short* logits, const float* labels, const float* kpercent, void* ws, long ws_bytes,
    float* wgt, float* loss, int B, int K, int H, int W, int per_image, int has_ignore, int ignore_index, cenet_stream_t stream);
int cenet_topk_ce_bwd_bf16(const unsigned short* logits, const float* labels, const float* wgt, const float* gout,
    unsigned short* dlogits, int B, int K, int H, int W, int has_ignore, int ignore_index, cenet_stream_t stream);
/* norm.hip */
int cenet_layernorm_fwd_bf16(const unsigned short* x, const float* gamma, const float* beta, unsigned short* y, float* mean,
    float* rstd, int rows, int C, float eps, cenet_stream_t stream);
int cenet_layernorm_bwd_add_acc_bf16(const unsigned short* dy, const unsigned short* x, const float* gamma, const float*
    mean, const float* rstd, const unsigned short* dx_add, unsigned short* dx, float* dgamma_acc, float* dbeta_acc, int
    rows, int C, cenet_stream_t stream);
int cenet_layernorm_bwd_acc_bf16(const unsigned short* dy, const unsigned short* x, const float* gamma, const float* mean,
    const float* rstd, unsigned short* dx, float* dgamma_acc, float* dbeta_acc, int rows, int C, cenet_stream_t stream);
int cenet_bn_stats_bf16(const unsigned short* x, long sb, int B, int C, int HW, float* ws, float* mean, float* var, float*
    running_mean, float* running_var, float momentum, long* num_batches_tracked, cenet_stream_t stream);
int cenet_bn_apply_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, const float* mean, const float* var,
    float eps, const float* gamma, const float* beta, int act, float slope, int B, int C, int HW, cenet_stream_t stream);
int cenet_bn_train_fwd_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, float* ws, float* mean, float* var,
    float* running_mean, float* running_var, float momentum, long* num_batches_tracked, float eps, const float* gamma,
    const float* beta, int act, float slope, int B, int C, int HW, int nbt_count, cenet_stream_t stream);
int cenet_bn_bwd_acc_bf16(const unsigned short* dy, long sgb, const unsigned short* x, long sxb, unsigned short* dx, long
    sdb, const float* mean, const float* var, float eps, const float* gamma, const float* beta, int act, float slope, int B,
    int C, int HW, float* ws, float* dgamma_acc, float* dbeta_acc, cenet_stream_t stream);
int cenet_bn_bwd_add_acc_bf16(const unsigned short* dy, long sgb, const unsigned short* x, long sxb, unsigned short* dx, long sdb,
    const unsigned short* dx_add, long sab, const float* mean, const float* var, float eps, const float* gamma, const float* beta,
    int act, float slope, int B, int C, int HW, float* ws, float* dgamma_acc, float* dbeta_acc, cenet_stream_t stream);
/* resample.hip */
int cenet_bilinear_fwd_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, int B, int C, int Hi, int Wi,
    int Ho, int Wo, float scale_h, float scale_w, int align_corners, cenet_stream_t stream);
int cenet_bilinear_bwd_bf16(const unsigned short* dy, long sgb, unsigned short* dx, long sdb, int B, int C, int Hi, int Wi,
    int Ho, int Wo, float scale_h, float scale_w, int align_corners, cenet_stream_t stream);
int cenet_bilinear_bwd_add_bf16(const unsigned short* dy, long sgb, unsigned short* dx, long sdb, const unsigned short* dx_add,
    int B, int C, int Hi, int Wi, int Ho, int Wo, float scale_h, float scale_w, int align_corners, cenet_stream_t stream);
int cenet_nearest2x_fwd_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, int B, int C, int Hi, int Wi,
    cenet_stream_t stream);
int cenet_nearest2x_bwd_bf16(const unsigned short* dy, long sgb, unsigned short* dx, long sdb, int B, int C, int Hi, int Wi,
    cenet_stream_t stream);
int cenet_adaptive_avgpool_fwd_bf16(const unsigned short* x, long sxb, unsigned short* y, long syb, int B, int C, int Hi,
    int Wi, int Ho, int Wo, cenet_stream_t stream);
int cenet_adaptive_avgpool_bwd_bf16(const unsigned short* dy, long sgb, unsigned short* dx, long sdb, int B, int C, int Hi,
    int Wi, int Ho, int Wo, cenet_stream_t stream);
int cenet_maxpool2_fwd_bf16(const unsigned short* x, unsigned short* y, long syb, const float* scale, int B, int C, int Hi,
    int Wi, cenet_stream_t stream);
int cenet_maxpool2_bwd_acc_bf16(const unsigned short* x, const unsigned short* dy, long sgb, unsigned short* dx, const
    float* scale, float* dscale_acc, int B, int C, int Hi, int Wi, cenet_stream_t stream);
/* stats.hip */
int cenet_ccu_stats_fwd_bf16(const unsigned short* x, const float* fc1, const float* fc2, float* u, int* amax, float* z, int
    B, int C, int HW, cenet_stream_t stream);
int cenet_gate_chan_fwd_bf16(const unsigned short* x, const float* g, unsigned short* y, int BC, int HW, cenet_stream_t
    stream);
int cenet_gate_chan_bwd_reduce_bf16(const unsigned short* x, const unsigned short* dy, const float* g, float* dg, int BC,
    int HW, cenet_stream_t stream);
int cenet_ccu_bwd_apply_acc_bf16(const unsigned short* x, const unsigned short* dy, const float* g, const float* dz, const
    float* u, const int* amax, const float* fc1, const float* fc2, float* dfc1_acc, float* dfc2_acc, unsigned short* dx, int
    B, int C, int HW, cenet_stream_t stream);
int cenet_ccu_bwd_apply_add_acc_bf16(const unsigned short* x, const unsigned short* dy, const float* g, const float* dz, const
    float* u, const int* amax, const float* fc1, const float* fc2, float* dfc1_acc, float* dfc2_acc, unsigned short* dx, const
    unsigned short* dx_add, int B, int C, int HW, cenet_stream_t stream);
int cenet_srm_stats_fwd_bf16(const unsigned short* x, float* u, int* amax, int B, int C, int HW, cenet_stream_t stream);
int cenet_gate_pix_fwd_bf16(const unsigned short* x, const float* f, unsigned short* y, int B, int C, int HW, cenet_stream_t
    stream);
int cenet_gate_pix_bwd_reduce_bf16(const unsigned short* x, const unsigned short* dy, const float* f, float* df, int B, int
    C, int HW, cenet_stream_t stream);
int cenet_srm_bwd_apply_bf16(const unsigned short* x, const unsigned short* dy, const float* f, const float* u, const float*
    du, const int* amax, unsigned short* dx, int B, int C, int HW, cenet_stream_t stream);

/* bf16 shadow of the fp32 master parameters (the weight operand of cenet_gemm_bf16): the fused SGD step can rewrite it in the
 * same pass (shadow_bf16 may be NULL), and whole buffers can be converted either way. */
int cenet_sgd_step_shadow_f32(float* p, const float* g, float* buf, const float* hyper5, long n, unsigned short* shadow_bf16,
                              cenet_stream_t stream);
int cenet_cast_f32_to_bf16(const float* x, unsigned short* y, long n, cenet_stream_t stream);
int cenet_cast_bf16_to_f32(const unsigned short* x, float* y, long n, cenet_stream_t stream);
/* y = bf16(x) and x = 0 in one pass: x is a persistent fp32 accumulator that kernels add into atomically (the dK / dV of the
 * spatial-reduction attention backward, pvtv2.py:88-109), left zero for its next use instead of a fill before every use */
int cenet_cast_clear_f32_to_bf16(float* x, unsigned short* y, long n, cenet_stream_t stream);
/* rows of N columns (N % 4 == 0): y = bf16(x + bias[col]); x = 0 — the tail of a split-K Linear (pvtv2.py:93-95 spatial-reduction
 * conv as a GEMM over K = C s^2) whose partial products were added atomically into the zero-at-rest accumulator x */
int cenet_cast_clear_bias_f32_to_bf16(float* x, unsigned short* y, const float* bias, int N, long n, cenet_stream_t stream);

/* ---- channel-local fused chains (chanloc.hip, round 5) --------------------------------------------------------------------
 * One workgroup owns one channel over the whole batch: BatchNorm's batch statistics are workgroup reductions, nothing is
 * stored between the steps of the chain, no float atomics (results independent of scheduling).
 * Every batch variance here is the biased one, formed in one pass as s2 / n - (s1 / n)^2 from fp32 sums of (v - K) and (v - K)^2
 * with the shift K = the mean of the first min(HW, 64) values of image 0's plane of the channel (not one sample: a single outlier
 * there used to cost the variance 1e-3 of its value); it meets the two-pass bound of tests/norm_ref.py on any data whose first
 * plane is not far from the channel's mean in units of its deviation.  Where a step's value is also an output tensor (dwbn's conv
 * output, cfam_mid's x1 and d_x0, cfam_front's y1) the chain goes on with the value AS STORED in the tensor type, so that the
 * backward pass, which reads or recomputes and rounds the same value, normalises what the forward normalised.
 * EUCB front, blocks.py:297-321 up to the 1x1 conv: y = LeakyReLU(BatchNorm_train(DW3x3(nearest_x2(x)))); x [B, C, H, W] (batch
 * stride sxb), y [B, C, 2H, 2W] (batch stride syb), w [C][9] (no bias).  Forward writes the batch mean / biased variance of the
 * conv output and updates the running statistics (unbiased variance; NULL: not wanted) and the batch counter.  Backward takes
 * the gradient g of y and writes dx; dw / dgamma / dbeta are ADDED into.  cenet_eucb_supported: the channel's source planes
 * (B*H*W elements of esize bytes) plus one group of gradient planes fit a workgroup's LDS. */
int cenet_eucb_supported(int B, int H, int W, int esize);
int cenet_eucb_fwd_f32(const float* x, long sxb, const float* w, const float* gamma, const float* beta, float eps, float slope,
                       float* y, long syb, float* mean, float* var, float* running_mean, float* running_var, float momentum,
                       long* num_batches_tracked, int B, int C, int H, int W, cenet_stream_t stream);
int cenet_eucb_bwd_acc_f32(const float* g, long sgb, const float* x, long sxb, const float* w, const float* gamma,
                           const float* beta, float eps, float slope, const float* mean, const float* var, float* dx, long sdb,
                           float* dw_acc, float* dgamma_acc, float* dbeta_acc, int B, int C, int H, int W,
                           cenet_stream_t stream);
int cenet_eucb_fwd_bf16(const unsigned short* x, long sxb, const float* w, const float* gamma, const float* beta, float eps,
                        float slope, unsigned short* y, long syb, float* mean, float* var, float* running_mean,
                        float* running_var, float momentum, long* num_batches_tracked, int B, int C, int H, int W,
                        cenet_stream_t stream);
int cenet_eucb_bwd_acc_bf16(const unsigned short* g, long sgb, const unsigned short* x, long sxb, const float* w,
                            const float* gamma, const float* beta, float eps, float slope, const float* mean, const float* var,
                            unsigned short* dx, long sdb, float* dw_acc, float* dgamma_acc, float* dbeta_acc, int B, int C,
                            int H, int W, cenet_stream_t stream);

/* CFAM "mid" chain, cfam.py:368-372 around nlb.py:141-148 (p_raw = the Non-local block's output conv, m = that block's input, x0 =
 * the CFAM block's input; all [B, C, HW] contiguous):  p = BatchNorm_nl(p_raw); z = (1 - w) m + w p; x1 = x0 + ls[c] z;
 * y2 = BatchNorm_2(x1), BatchNorm_2 taking its statistics from x1 as stored (rounded to the tensor type).  One launch each way (workgroup = channel over the batch; cenet_chanloc_supported(B, HW) says whether a
 * channel is small enough).  Forward writes x1, y2, both batch means / biased variances, updates both running statistics and
 * counters (NULL: not wanted).  Backward: g_y2 and (optional) g_x1 in; d_p_raw, d_m, d_x0 out; the six parameter gradients are
 * ADDED into (dw, a scalar, with one float atomic per channel).  d_x0 = d x1 is rounded to the tensor type once; d_m, d_p_raw and the
 * parameter gradients are taken from that stored value. */
int cenet_chanloc_supported(int B, int HW);
int cenet_cfam_mid_fwd_f32(const float* p_raw, const float* m, const float* x0, float* x1, float* y2, const float* gamma_p,
                           const float* beta_p, float eps_p, float* mean_p, float* var_p, float* rmean_p, float* rvar_p,
                           float mom_p, long* nbt_p, const float* w, const float* ls, const float* gamma_2, const float* beta_2,
                           float eps_2, float* mean_2, float* var_2, float* rmean_2, float* rvar_2, float mom_2, long* nbt_2,
                           int B, int C, int HW, cenet_stream_t stream);
int cenet_cfam_mid_bwd_acc_f32(const float* g_y2, const float* g_x1, const float* p_raw, const float* m, const float* x1,
                               float* d_p_raw, float* d_m, float* d_x0, const float* gamma_p, const float* beta_p, float eps_p,
                               const float* mean_p, const float* var_p, const float* w, const float* ls, const float* gamma_2,
                               float eps_2, const float* mean_2, const float* var_2, float* dgamma_p_acc, float* dbeta_p_acc,
                               float* dw_acc, float* dls_acc, float* dgamma_2_acc, float* dbeta_2_acc, int B, int C, int HW,
                               cenet_stream_t stream);
int cenet_cfam_mid_fwd_bf16(const unsigned short* p_raw, const unsigned short* m, const unsigned short* x0, unsigned short* x1,
                            unsigned short* y2, const float* gamma_p, const float* beta_p, float eps_p, float* mean_p,
                            float* var_p, float* rmean_p, float* rvar_p, float mom_p, long* nbt_p, const float* w, const float* ls,
                            const float* gamma_2, const float* beta_2, float eps_2, float* mean_2, float* var_2, float* rmean_2,
                            float* rvar_2, float mom_2, long* nbt_2, int B, int C, int HW, cenet_stream_t stream);
int cenet_cfam_mid_bwd_acc_bf16(const unsigned short* g_y2, const unsigned short* g_x1, const unsigned short* p_raw,
                                const unsigned short* m, const unsigned short* x1, unsigned short* d_p_raw, unsigned short* d_m,
                                unsigned short* d_x0, const float* gamma_p, const float* beta_p, float eps_p, const float* mean_p,
                                const float* var_p, const float* w, const float* ls, const float* gamma_2, float eps_2,
                                const float* mean_2, const float* var_2, float* dgamma_p_acc, float* dbeta_p_acc, float* dw_acc,
                                float* dls_acc, float* dgamma_2_acc, float* dbeta_2_acc, int B, int C, int HW,
                                cenet_stream_t stream);

/* Dilated depthwise branches of MultiOrderDWConv with their BatchNorm, cfam.py:227-241 over blocks.py:169-177, one launch each
 * way (workgroup = channel over the batch; cenet_chanloc_supported(B, H*W)):
 *   v[:, j*g + i] = ReLU(BatchNorm_train(DW3x3 with dilation dil[j] and weights w[j] ([g][9], no bias) of x[:, j*g + i])), j < nb <= 3;
 *   rest = x[:, nb*g : nb*g + p] (the pooled branch's slice; p may be 0).
 * The conv output is rounded to the tensor type (as the launch chain stores it) and the statistics are those of the rounded values;
 * the backward pass recomputes and rounds it the same way.
 * x [B, nb*g + p, H, W] (batch stride sxb), v [B, nb*g, H, W] (svb), rest [B, p, H, W] (srb); gamma / beta / mean / var / running
 * statistics cover the nb*g channels, num_batches_tracked holds nb counters (NULL: not wanted).
 * Backward: g_v, g_rest and g_add (another gradient of x, [B, nb*g + p, H, W], may be NULL) in; dx = their sum through the chain;
 * dw_acc[j] / dgamma / dbeta are ADDED into (B*H*W <= 8192: the channel's planes and gradient planes sit in LDS). */
int cenet_dwbn_fwd_f32(const float* x, long sxb, const float* const* w, const int* dil, int nb, int g, int p, float* v, long svb,
                       float* rest, long srb, const float* gamma, const float* beta, float eps, float* mean, float* var,
                       float* running_mean, float* running_var, float momentum, long* num_batches_tracked, int B, int H, int W,
                       cenet_stream_t stream);
int cenet_dwbn_bwd_acc_f32(const float* g_v, long sgb, const float* g_rest, long srb, const float* g_add, long sab, const float* x,
                           long sxb, const float* const* w, const int* dil, int nb, int g, int p, const float* gamma,
                           const float* beta, float eps, const float* mean, const float* var, float* dx, long sdb,
                           float* const* dw_acc, float* dgamma_acc, float* dbeta_acc, int B, int H, int W, cenet_stream_t stream);
int cenet_dwbn_fwd_bf16(const unsigned short* x, long sxb, const float* const* w, const int* dil, int nb, int g, int p,
                        unsigned short* v, long svb, unsigned short* rest, long srb, const float* gamma, const float* beta,
                        float eps, float* mean, float* var, float* running_mean, float* running_var, float momentum,
                        long* num_batches_tracked, int B, int H, int W, cenet_stream_t stream);
int cenet_dwbn_bwd_acc_bf16(const unsigned short* g_v, long sgb, const unsigned short* g_rest, long srb,
                            const unsigned short* g_add, long sab, const unsigned short* x, long sxb, const float* const* w,
                            const int* dil, int nb, int g, int p, const float* gamma, const float* beta, float eps,
                            const float* mean, const float* var, unsigned short* dx, long sdb, float* const* dw_acc,
                            float* dgamma_acc, float* dbeta_acc, int B, int H, int W, cenet_stream_t stream);

/* CFAM front, cfam.py:366 over cfam.py:251-264, one launch each way (workgroup = channel over the batch, one wave per image for the
 * per-image statistics; cenet_chanloc_supported(B, HW), B <= 256):  y1 = BatchNorm_1(x0);  u[b, c] = [max, mean, biased std] of
 * y1[b, c] as stored (the std in one pass, shifted by the mean of the plane's first min(HW, 64) values; amax: the smallest index of
 * the maximum);  z = fc2 . relu(fc1 u) (fc1 [C][3][3], fc2 [C][3]);  zn = BatchNorm1d_train(z) over the batch (gamma_d == NULL: zn = z,
 * the reference's batch-of-one rule);  xs = y1 * sigmoid(zn).  All tensors [B, C, HW] contiguous; u [B, C, 3], amax / z / zn
 * [B, C] are saved for the backward pass.  Backward: g_xs (gradient of xs), g_y1 (of y1: the MCA shortcut; may be NULL), g_tap (of
 * x0 itself: the residual around the block; may be NULL) in, dx0 out; parameter gradients ADDED into. */
int cenet_cfam_front_fwd_f32(const float* x0, float* y1, float* xs, const float* gamma1, const float* beta1, float eps1,
                             float* mean1, float* var1, float* rmean1, float* rvar1, float mom1, long* nbt1, const float* fc1,
                             const float* fc2, const float* gamma_d, const float* beta_d, float eps_d, float* mean_d, float* var_d,
                             float* rmean_d, float* rvar_d, float mom_d, long* nbt_d, float* u, int* amax, float* z, float* zn,
                             int B, int C, int HW, cenet_stream_t stream);
int cenet_cfam_front_bwd_acc_f32(const float* g_xs, const float* g_y1, const float* g_tap, const float* x0, float* dx0,
                                 const float* gamma1, const float* beta1, float eps1, const float* mean1, const float* var1,
                                 const float* fc1, const float* fc2, const float* gamma_d, float eps_d, const float* mean_d,
                                 const float* var_d, const float* u, const int* amax, const float* z, const float* zn,
                                 float* dgamma1_acc, float* dbeta1_acc, float* dfc1_acc, float* dfc2_acc, float* dgamma_d_acc,
                                 float* dbeta_d_acc, int B, int C, int HW, cenet_stream_t stream);
int cenet_cfam_front_fwd_bf16(const unsigned short* x0, unsigned short* y1, unsigned short* xs, const float* gamma1,
                              const float* beta1, float eps1, float* mean1, float* var1, float* rmean1, float* rvar1, float mom1,
                              long* nbt1, const float* fc1, const float* fc2, const float* gamma_d, const float* beta_d,
                              float eps_d, float* mean_d, float* var_d, float* rmean_d, float* rvar_d, float mom_d, long* nbt_d,
                              float* u, int* amax, float* z, float* zn, int B, int C, int HW, cenet_stream_t stream);
int cenet_cfam_front_bwd_acc_bf16(const unsigned short* g_xs, const unsigned short* g_y1, const unsigned short* g_tap,
                                  const unsigned short* x0, unsigned short* dx0, const float* gamma1, const float* beta1,
                                  float eps1, const float* mean1, const float* var1, const float* fc1, const float* fc2,
                                  const float* gamma_d, float eps_d, const float* mean_d, const float* var_d, const float* u,
                                  const int* amax, const float* z, const float* zn, float* dgamma1_acc, float* dbeta1_acc,
                                  float* dfc1_acc, float* dfc2_acc, float* dgamma_d_acc, float* dbeta_d_acc, int B, int C, int HW,
                                  cenet_stream_t stream);

/* Depthwise 3x3 (+bias) + activation with NO BatchNorm, cfam.py:150-151 (the CFAM Mlp's conv + GELU), one launch each way
 * (workgroup = channel over the batch, B*H*W <= 8192 and cenet_chanloc_supported(B, H*W)): y = act(DW3x3_dil(x) + bias); x, y
 * [B, C, H, W] contiguous, w [C][9], bias [C] or NULL.  The pre-activation is not stored; backward recomputes it from x and
 * writes dx; dw / dbias (may be NULL) are ADDED into.
 * GELU is 0.5 u (1 + erf(u / sqrt 2)).  The fp32 instances evaluate it with erff / expf.  The bf16 instances use max(u, 0) - |u| h
 * and, for the derivative, (u >= 0 ? 1 - h : h) + u phi(u), with h = erfc(|u| / sqrt 2) / 2 by Abramowitz & Stegun 7.1.26 (|error of
 * erf| <= 1.5e-7, so 0.75e-7 on h) on the hardware reciprocal and exponential (1 ulp each; the degree-5 polynomial in t = 1 / (1 + p |u|)
 * amplifies a relative error of t at most 5 times, h <= 1/2: below 2^-21 = 4.8e-7 in all), one exponential serving both terms:
 *   |gelu_bf16(u) - gelu(u)| <= 6e-7 |u|,   |gelu'_bf16(u) - gelu'(u)| <= 7e-7   (u phi(u) <= 0.25 adds its exponential's 2^-23 / 4),
 * a four-hundredth of a bf16 ulp. */
int cenet_dwact_fwd_f32(const float* x, const float* w, const float* bias, float* y, int act, float slope, int dil, int B, int C,
                        int H, int W, cenet_stream_t stream);
int cenet_dwact_bwd_acc_f32(const float* g, const float* x, const float* w, const float* bias, float* dx, float* dw_acc,
                            float* dbias_acc, int act, float slope, int dil, int B, int C, int H, int W, cenet_stream_t stream);
int cenet_dwact_fwd_bf16(const unsigned short* x, const float* w, const float* bias, unsigned short* y, int act, float slope,
                         int dil, int B, int C, int H, int W, cenet_stream_t stream);
int cenet_dwact_bwd_acc_bf16(const unsigned short* g, const unsigned short* x, const float* w, const float* bias,
                             unsigned short* dx, float* dw_acc, float* dbias_acc, int act, float slope, int dil, int B, int C,
                             int H, int W, cenet_stream_t stream);

/* Pooled branch of MultiOrderDWConv, cfam.py:212-218,231-232, two launches each way at every decoder level:
 *   y = bilinear_{(H, W), align_corners = False}(bilinear_{x7, align_corners = True}(LeakyReLU(BatchNorm_train(Conv1x1_{PxP}(AdaptiveAvgPool_7x7(x))))))
 * x [B, P, H, W] (batch stride sxb: a channel slice of a wider tensor), y likewise (syb); P <= 32, B <= 64, H, W <= 64.
 * RH [H, 7] / RW [W, 7]: the two resamplings composed into one linear map per axis (R_{49 -> H} R_{7 -> 49}; host-built with
 * the coordinate rule of cenet_bilinear_fwd).  pooled, t [B, P, 49] fp32 are written for the backward pass, which takes g (the
 * gradient of y, batch stride sgb) and a [B, P, 49] fp32 workspace, writes dx [B, P, H, W] (batch stride sdb) and ADDS the
 * conv-weight [P, P] and BatchNorm gradients. */
int cenet_pool_branch_fwd_f32(const float* x, long sxb, const float* wc, const float* gamma, const float* beta, float eps,
                              float slope, const float* RH, const float* RW, float* y, long syb, float* pooled, float* t,
                              float* mean, float* var, float* running_mean, float* running_var, float momentum,
                              long* num_batches_tracked, int B, int P, int H, int W, cenet_stream_t stream);
int cenet_pool_branch_bwd_acc_f32(const float* g, long sgb, const float* wc, const float* gamma, const float* beta, float eps,
                                  float slope, const float* RH, const float* RW, const float* pooled, const float* t,
                                  const float* mean, const float* var, float* dt_ws, float* dx, long sdb, float* dwc_acc,
                                  float* dgamma_acc, float* dbeta_acc, int B, int P, int H, int W, cenet_stream_t stream);
int cenet_pool_branch_fwd_bf16(const unsigned short* x, long sxb, const float* wc, const float* gamma, const float* beta,
                               float eps, float slope, const float* RH, const float* RW, unsigned short* y, long syb,
                               float* pooled, float* t, float* mean, float* var, float* running_mean, float* running_var,
                               float momentum, long* num_batches_tracked, int B, int P, int H, int W, cenet_stream_t stream);
int cenet_pool_branch_bwd_acc_bf16(const unsigned short* g, long sgb, const float* wc, const float* gamma, const float* beta,
                                   float eps, float slope, const float* RH, const float* RW, const float* pooled, const float* t,
                                   const float* mean, const float* var, float* dt_ws, unsigned short* dx, long sdb,
                                   float* dwc_acc, float* dgamma_acc, float* dbeta_acc, int B, int P, int H, int W,
                                   cenet_stream_t stream);

/* Self-test of the wave reductions every kernel's block reductions rest on (common.h wave_sum / wave_max / wave_min_i on the
 * DPP path): wave w reduces x[64 w .. 64 w + 64) -> sums[w], maxs[w], mins[w] = min over lanes of (int)(1024 x) + lane, as lane 0
 * holds them, and the same three at [nwaves + w] as lane 37 holds them (each array: 2 nwaves entries). */
int cenet_selftest_wave_reduce(const float* x, float* sums, float* maxs, int* mins, int nwaves, cenet_stream_t stream);

/* SRM tail without separate activation / BatchNorm launches (stats.hip, round 5; cfam.py:93-101 after the channel statistics,
 * training mode): cenet_srm_conv_gelu_fwd_f32 writes f = pwc(u) + dwc(u), fa = GELU(f) and cenet_srm_parts(B, H, W) (count, mean, M2)
 * triples; cenet_gate_pix_bn_fwd_* folds them (exact in any order), writes y = x * sigmoid(fb) with fb = BatchNorm(fa) ([B, HW],
 * also stored), the batch mean / biased variance, and updates the running statistics; cenet_srm_conv_bn_bwd_acc_f32 takes dfb (the
 * gradient of fb, from cenet_gate_pix_bwd_reduce_*) and does BatchNorm backward, GELU' and the conv backward (du [B, 3, H, W]; the
 * conv and BatchNorm parameter gradients ADDED into; part2_ws: 2 * cenet_srm_parts floats).  H * W <= 4096. */
int cenet_srm_fused_supported(int B, int H, int W);
int cenet_srm_parts(int B, int H, int W);
int cenet_srm_conv_gelu_fwd_f32(const float* u, const float* pwc, const float* dwc, float* f, float* fa, float* part, int B, int H,
                                int W, cenet_stream_t stream);
int cenet_gate_pix_bn_fwd_f32(const float* x, const float* fa, const float* part, int G, float* fb, float* y, const float* gamma,
                              const float* beta, float eps, float* mean, float* var, float* running_mean, float* running_var,
                              float momentum, long* num_batches_tracked, int B, int C, int HW, cenet_stream_t stream);
int cenet_gate_pix_bn_fwd_bf16(const unsigned short* x, const float* fa, const float* part, int G, float* fb, unsigned short* y,
                               const float* gamma, const float* beta, float eps, float* mean, float* var, float* running_mean,
                               float* running_var, float momentum, long* num_batches_tracked, int B, int C, int HW,
                               cenet_stream_t stream);
int cenet_srm_conv_bn_bwd_acc_f32(const float* u, const float* dfb, const float* fa, const float* f, const float* mean,
                                  const float* var, float eps, const float* gamma, const float* pwc, const float* dwc,
                                  float* part2_ws, float* du, float* dpwc_acc, float* ddwc_acc, float* dgamma_acc, float* dbeta_acc,
                                  int B, int H, int W, cenet_stream_t stream);

/* The ACDC training-time augmentation on the device (augment.hip, round 5; replaces RandomGenerator.__call__,
 * src/datasets/dataset_acdc.py:32-48 with random_rot_flip :15-22 and random_rotate :25-29, for a whole batch).  The training
 * slices live in two device pools (pool_img fp32, pool_lab uint8, same element offsets).  Per sample b:
 *   tab[8 b ..]  = offset, H, W, mode (0 none / 1 quarter turns + flip / 2 rotation), k, axis, resize flag, 0
 *   dp[10 b ..]  = rotation matrix m00 m01 m10 m11, offset0, offset1 (scipy.ndimage.rotate's, mode 2 only);
 *                  pole^(Ha-1), pole^(Wa-1) with pole = sqrt(3) - 2 and (Ha, Wa) the size after stage 1; (Ha-1)/(OH-1), (Wa-1)/(OW-1)
 * all computed by the host in fp64 (cenet_amd/data.py DeviceAugmenter.draw, which consumes `random` / `np.random` in the
 * reference's order).  stage_img (fp64) / stage_lab (uint8): B * stage_stride elements of scratch, stage_stride >= max_h * max_w
 * >= every sample's H * W.  out_img [B, 1, OH, OW] fp32, out_lab [B, OH, OW] fp32 (class indices).  Labels are bit-identical to
 * the reference's, images to fp64 rounding of the same operation order. */
int cenet_augment_acdc(const float* pool_img, const unsigned char* pool_lab, const long* tab, const double* dp, double* stage_img,
                       unsigned char* stage_lab, long stage_stride, int max_h, int max_w, float* out_img, float* out_lab, int B,
                       int OH, int OW, cenet_stream_t stream);

/* Composable slice augmentation on the device (augment_ops.hip): the operator family of the Synapse training pipeline
 * (src/datasets/dataset_synapse.py:86-112), each operator specified by scipy, up to S <= 8 stages per sample for a whole batch.
 * The operators and their distribution are the pipeline's; imgaug's random stream and interpolation bits are not claimed.
 *   tab[(3 + S) b ..]       = offset (elements into the pools), H, W, then S op words
 *   dp[32 (S b + s) ..]     = the parameter row of stage s of sample b, computed by the host in fp64
 *   op word                   image (fp32 in, fp64 arithmetic without contraction, fp32 out)            label (uint8)    dp row
 *   0 copy                    v                                                                          same             -
 *   1 flip_ud / 2 flip_lr     index map                                                                  same map         -
 *   3 affine                  scipy.ndimage.affine_transform(a64, M, offset, order=1, mode="constant")   order=0          M00 M01 M10 M11 off0 off1
 *   4 + 256 R + 65536 C       map_coordinates(order=1, mode="constant") at (i + dY, j + dX), dY / dX     order=0          dY[R*C] at 0, dX[R*C] at 16
 *     grid_warp               the bilinear samples of R x C control grids at (i (R-1)/(H-1), j (C-1)/(W-1))
 *   5 blur                    gaussian_filter(a64, sigma, mode="mirror"), axis 0 then axis 1             unchanged        radius, w[0 .. radius]
 *   6 noise                   v + scale * z(p): Philox4x32-10, counter (p, 0, 0, 0), p = i W + j,        unchanged        scale, key0, key1
 *                             z = sqrt(-2 ln u1) cos(2 pi u2), u = (word + 0.5) / 2^32 of output words 0, 1
 *   7 contrast                c + alpha * (v - c)                                                        unchanged        alpha, c
 * (blur: w[0] the centre weight and w[k] the normalised weight of both taps at distance k.)  Stage s reads the pools (s = 0) or
 * work buffer s & 1 and writes work buffer (s + 1) & 1: the result, sample b at b * stride with its own H x W, is in buffer S & 1.
 * Both work buffers hold B * stride fp32 and B * stride uint8.  tab_host / dp_host are the tables in host memory, tab / dp the
 * same tables on the device: the host copies are checked before anything is launched.  CENET_EINVAL (nothing launched) for an
 * unknown op word, S < 1 or S > 8, a blur radius above 16, R < 2, C < 2 or R*C > 16, H > max_h, W > max_w, H*W > stride or
 * B > 65535. */
int cenet_augment_ops(const float* pool_img, const unsigned char* pool_lab, const long* tab_host, const double* dp_host,
                      const long* tab, const double* dp, float* work_img0, unsigned char* work_lab0, float* work_img1,
                      unsigned char* work_lab1, long stride, int max_h, int max_w, int B, int S, cenet_stream_t stream);
/* Philox4x32-10 as cenet_augment_ops draws it, for n rows of ctr_key [n, 6] = 4 counter and 2 key words (each 0 .. 2^32 - 1,
 * held as long) -> out [n, 4] output words: holds the generator to the published Random123 vectors. */
int cenet_philox4x32_10(const long* ctr_key, long* out, int n, cenet_stream_t stream);
/* x[0 .. n) = (x - mean) / std in fp32, in place: Normalize([mean], [std]) after the augmentation's resize. */
int cenet_augment_normalize(float* x, long n, float mean, float std, cenet_stream_t stream);

/* Composable augmentation of multi-channel images on the device (augment_image_ops.hip): the operator family of the skin training
 * pipeline (src/datasets/skin/dataset_ham.py:273-281, albumentations Compose), each operator specified by scipy / numpy, up to
 * S <= 8 stages per sample for a batch of B samples.  The operators and their distribution are the pipeline's; albumentations'
 * random stream, its cv2 interpolation and its uint8 LUT rounding are not claimed.  The pools hold N samples of one size: sample
 * n's C planar channels (1 <= C <= 4) at pool_img + n*C*H*W, its label plane at pool_lab + n*H*W; H, W <= 1024.
 *   tab[(1 + S) b ..]       = sample index n, then S op words
 *   dp[32 (S b + s) ..]     = the parameter row of stage s of sample b, computed by the host in fp64
 *   op word                   image, every channel (fp32 in, fp64 arithmetic without contraction, fp32 out)   label (uint8)  dp row
 *   0 copy                    v                                                                                same           -
 *   1 flip_ud                 a[H-1-i][j]                                                                      same map       -
 *   2 flip_lr                 a[i][W-1-j]                                                                      same map       -
 *   3 | m affine              affine_transform(a64, M, offset, order=1, mode=m, cval=0)                        order=0        M[4], offset[2]
 *   4 blur                    correlate1d(correlate1d(a64, w, 0, mode='mirror'), w, 1, mode='mirror')          unchanged      radius, w[0 .. radius]
 *   5 brightness_contrast     np.clip(alpha * a64 + beta, lo, hi)                                              unchanged      alpha, beta, lo, hi
 *   6 | m elastic             map_coordinates(a64, [i + alpha g[0], j + alpha g[1]], order=1, mode=m, cval=0)  order=0        alpha, key0, key1
 * m: 0 for mode='constant', 256 (bit 8) for mode='mirror'.  (blur: w[0] the centre weight and w[k] the weight of both taps at
 * distance k.)  The elastic field g is made on the device, p = i*W + j, f = 0 (rows) / 1 (columns):
 *   u[f][i][j] = (philox4x32_10(counter (p, f, 0, 0), key (key0, key1))[0] + 0.5) / 2^31 - 1
 *   g[f]       = correlate1d(correlate1d(u[f], fw, 0, mode='constant', cval=0), fw, 1, mode='constant', cval=0)
 * fw: ONE symmetric kernel per call, fw[0] the centre and fw[k] the weight of both taps at distance k <= field_radius <= 256;
 * field: B*2*H*W doubles of scratch, g of sample b at field + b*2*H*W afterwards.  fw, fw_host and field may be null when no sample
 * carries an elastic stage; at most one elastic stage per sample.  Stage s reads the pools (s = 0) or work buffer s & 1 and writes
 * work buffer (s + 1) & 1: the result, sample b's channels at b*C*H*W and its label at b*H*W, is in buffer S & 1.  Both work
 * buffers hold B*C*H*W fp32 and B*H*W uint8.  out_lab (or null): [B, H, W] fp32, the result's labels as float class ids.
 * tab_host / dp_host / fw_host are the tables in host memory, tab / dp / fw the same on the device: the host copies are checked
 * before anything is launched.  CENET_EINVAL (nothing launched) for an unknown op, stray bits in an op word (bit 8 on an op that
 * takes no mode included), S < 1 or S > 8, C outside 1..4, H or W outside 1..1024, a blur radius above 16 or not an integer, a
 * field radius above 256, a second elastic stage in one chain, a key word outside [0, 2^32), lo > hi, a sample index outside
 * [0, N) or B > 65535. */
int cenet_augment_image_ops(const float* pool_img, const unsigned char* pool_lab, const long* tab_host, const double* dp_host,
                            const long* tab, const double* dp, const double* fw_host, const double* fw, int field_radius,
                            double* field, float* work_img0, unsigned char* work_lab0, float* work_img1, unsigned char* work_lab1,
                            float* out_lab, int N, int C, int H, int W, int B, int S, cenet_stream_t stream);
/* Per-sample min-max normalisation (dataset_ham.py:113 on float32 arrays): y[b][i] = (x[b][i] - mn_b) / ((mx_b - mn_b) + 1e-8f)
 * for x, y [B, n] fp32 (y may be x), all in float32.  Two launches, no atomics: per-workgroup minima / maxima into part
 * (B * 2 * 128 floats of scratch), then a combine and the apply. */
int cenet_augment_minmax(const float* x, float* y, float* part, int B, long n, cenet_stream_t stream);

/* Test-time volume inference on the device (volresize.hip; src/utils/metrics_eval.py:37-84, utils_synapse.py:49-97).
 * cenet_vol_resize_cubic: scipy.ndimage.zoom(slice, (PH / H, PW / W), order=3) for n slices src [n, H, W] fp32 -> out
 * [n, 1, PH, PW] fp32, computed in fp64 in scipy's operation order (prefilter with mirror boundary along axis 0 then axis 1,
 * coordinate o * ((H - 1) / (PH - 1)), cval = 0 above H - 1).  stage: n * H * W doubles of scratch.  zn_h = pole^(H-1), zn_w =
 * pole^(W-1) with pole = sqrt(3) - 2, from the host as for cenet_augment_acdc.  normalize != 0: out = (float(v) - mean) / std in
 * fp32.  H, W, PH, PW >= 2 (scipy special-cases length-1 axes), n <= 65535; CENET_EINVAL otherwise. */
int cenet_vol_resize_cubic(const float* src, double* stage, float* out, int n, int H, int W, int PH, int PW, double zn_h,
                           double zn_w, int normalize, float mean, float std, cenet_stream_t stream);
/* pred [n, H, W] (class ids as floats) = zoom(argmax over K of logits [n, K, PH, PW], (H / PH, W / PW), order=0) without writing
 * the [PH, PW] class map: output pixel (y, x) takes the first maximum over K at the source pixel floor(c + 0.5), c = index *
 * ((PH - 1) / (H - 1)) in fp64, and 0 where c > PH - 1.  (H, W) == (PH, PW) is the plain argmax.  labels [n, H, W] (class ids as
 * floats) and counts [(K+1)*3] (uint32, zero-filled by the call) as for cenet_argmax_counts_f32, both may be NULL together.
 * K <= 16; H, W, PH, PW >= 2; CENET_EINVAL otherwise. */
int cenet_argmax_resize_counts_f32(const float* logits, const float* labels, float* pred, unsigned* counts, int n, int K, int PH,
                                   int PW, int H, int W, cenet_stream_t stream);
int cenet_argmax_resize_counts_bf16(const unsigned short* logits, const float* labels, float* pred, unsigned* counts, int n, int K,
                                    int PH, int PW, int H, int W, cenet_stream_t stream);

/* Flip / rotate test-time augmentation (tta.hip).  A view is an element g of the dihedral group D4 as a bit field: bit 0 flip
 * along W, bit 1 flip along H, bit 2 transpose H and W; forward v = x; g & 4: v = v^T; g & 2: v = flip_H(v); g & 1: v = flip_W(v).
 * view_mask: bit g set = view g is used, 1..255; the T = popcount(view_mask) views are taken in ascending code order.  Views with
 * bit 2 need PH == PW.
 * cenet_tta_views_f32: src [n, C, PH, PW] -> out [T, n, C, PH, PW], every view in one launch (bit copies).
 * cenet_tta_argmax_resize_counts_*: logits [T, n, K, PH, PW], stack t computed from view t of the input -> pred [n, H, W] (class
 * ids as floats): at the source pixel that zoom(order=0) picks (the rule of cenet_argmax_resize_counts_*, class 0 where the
 * coordinate exceeds PH - 1 or PW - 1) every view's K logits are read at that pixel's place in the view, turned into a
 * max-subtracted fp32 softmax and summed in view order; pred is the first maximum of the sums under `>`.  conf (or NULL):
 * [n, H, W], sum[pred] * (1.0f / T), 0 where the coordinate is outside.  labels / counts as for cenet_argmax_resize_counts_*.
 * Non-finite logits are not special-cased: a NaN sum never wins under `>`.  CENET_EINVAL for a null logits / pred, labels
 * without counts, a view_mask outside 1..255, a transposed view with PH != PW, K outside 1..16, a side < 2 (cenet_tta_views_f32:
 * < 1) or a plane of more than 2^31 - 1 pixels. */
int cenet_tta_views_f32(const float* src, float* out, int n, int C, int PH, int PW, int view_mask, cenet_stream_t stream);
int cenet_tta_argmax_resize_counts_f32(const float* logits, const float* labels, float* pred, float* conf, unsigned* counts, int n,
                                       int K, int PH, int PW, int H, int W, int view_mask, cenet_stream_t stream);
int cenet_tta_argmax_resize_counts_bf16(const unsigned short* logits, const float* labels, float* pred, float* conf,
                                        unsigned* counts, int n, int K, int PH, int PW, int H, int W, int view_mask,
                                        cenet_stream_t stream);

/* Sliding-window inference at the image's own resolution (sliding_window.hip): the network runs on overlapping [PH, PW] windows of
 * a [H, W] slice, the windows' class probabilities are blended with a separable importance map, nothing is resized.
 * oy_host [nwy] / ox_host [nwx]: the window origins per axis, in HOST memory; window (b, iy, ix) is entry (b * nwy + iy) * nwx + ix
 * of the window batch and holds source pixel (oy[iy] + y, ox[ix] + x) at (y, x).  An origin may be negative (a slice smaller
 * than the window).  Both tables are checked before anything is launched and reach the kernels by value in the kernel
 * arguments (no upload, no synchronisation): strictly ascending, first <= 0, o[i + 1] <= o[i] + P, last + P >= L, 1..32 entries,
 * every window on the slice (o[0] > -P, last < L) — so every output pixel lies in a window.
 * cenet_sw_windows_f32: src [n, C, H, W] -> out [n * nwy * nwx, C, PH, PW], all windows in one launch: a bit copy inside the
 * slice, or with normalize != 0 the fp32 (x - mean) / std (a true division); pad_value, stored as given, outside.
 * cenet_sw_merge_counts_*: logits [T, n * nwy * nwx, K, PH, PW], stack t computed from view t (cenet_tta_views_f32, view_mask
 * and T as there; 0x01: no augmentation) of the window batch -> pred [n, H, W] (class ids as floats).  Per output pixel (y, x):
 * every window that covers it in ascending (iy, ix), inside a window every view in ascending code: the K logits at the pixel's
 * place in that view become a max-subtracted fp32 softmax p and sum[k] += w * p[k]; once per window wsum += w, with w = wy[y - oy[iy]] *
 * wx[x - ox[ix]] (wy [PH], wx [PW]: the importance map's two fp32 factors, on the device, positive).  pred is the first maximum
 * of the sums under `>`, conf (or NULL) [n, H, W] = sum[pred] / (wsum * T).  The order of the additions is fixed: two calls
 * agree to the bit.  A window's padding is never read.  labels / counts as for cenet_argmax_resize_counts_*.  Non-finite
 * logits are not special-cased: a NaN sum never wins under `>`.
 * CENET_EINVAL (nothing launched) for a null src / out / logits / pred / wy / wx / table, labels without counts, n or C < 1, a
 * side < 1, K outside 1..16, a view_mask outside 1..255, a transposed view with PH != PW, a table that fails the checks above or
 * a plane of more than 2^31 - 1 pixels. */
int cenet_sw_windows_f32(const float* src, float* out, const int* oy_host, const int* ox_host, int n, int C, int H, int W, int PH,
                         int PW, int nwy, int nwx, int normalize, float mean, float std, float pad_value, cenet_stream_t stream);
int cenet_sw_merge_counts_f32(const float* logits, const float* labels, const float* wy, const float* wx, const int* oy_host,
                              const int* ox_host, float* pred, float* conf, unsigned* counts, int n, int K, int PH, int PW, int H,
                              int W, int nwy, int nwx, int view_mask, cenet_stream_t stream);
int cenet_sw_merge_counts_bf16(const unsigned short* logits, const float* labels, const float* wy, const float* wx,
                               const int* oy_host, const int* ox_host, float* pred, float* conf, unsigned* counts, int n, int K,
                               int PH, int PW, int H, int W, int nwy, int nwx, int view_mask, cenet_stream_t stream);

/* LayerNorm of a split-K accumulator (norm.hip, round 5; pvtv2.py:93-95,99-100: sr conv -> norm): acc [rows, C] fp32 holds the
 * conv's products (zero-at-rest accumulator of a split-K GEMM); xpre = bf16(acc + bias) (the rows the LayerNorm backward reads),
 * y = LayerNorm(xpre) * gamma + beta, mean / rstd [rows]; acc is left zero.  bias may be NULL.  C % 4 == 0, C <= 512. */
int cenet_layernorm_fwd_acc_bf16(float* acc, const float* bias, unsigned short* xpre, const float* gamma, const float* beta,
                                 unsigned short* y, float* mean, float* rstd, int rows, int C, float eps, cenet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CENET_HIP_H */
