// lovasz.hip — the Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018, Alg. 1) on the device: keys, a batched stable radix
// sort, integer ranks, coefficients, backward.  include/cenet_hip.h spells the definition out; in short, per segment (one class
// over the batch, or one (image, class) with per_image) the pixels are ordered by descending error e = |g - p_c|, equal errors by
// ascending pixel index, and with the INTEGER counts G (pixels of the class), F_i (of the class among sorted positions 0 .. i),
// Z_i = i + 1 - F_i, I_i = G - F_i, U_i = G + Z_i the increment of the Jaccard loss at position i is
//   1 / U_i  (g = 1)      I_i / (U_i (U_i - 1))  (g = 0)      1  (U_i = 1)
// evaluated from the integers, never as a difference of two floats near 1.
//
// LAUNCHES of a forward (stream order is the only synchronisation, nothing is read back):
//   keys     one pass over inputs and labels: fp32 softmax, key = bits(e) + 1 (non-negative floats order as their bits; key 0 =
//            ignored pixel, which therefore sorts below every other), payload = pixel index << 1 | g
//   4 x (hist, rowscan, scatter)   stable LSD radix sort of the S segments, 8 bits a pass over all 32 key bits, DESCENDING (the
//            digit is taken from the inverted key).  hist: digit counts per tile of TILE_ELEMS elements (integer LDS atomics: counts
//            only).  rowscan (tile_rank.h's tile_rowscan_kernel): exclusive scan of every (segment, digit) row over its tiles (a
//            group of lanes a row).  scatter:
//            the element's place = digits below it in the segment + the same digit in earlier tiles + the same digit earlier in
//            this tile.  The last is a RANK, and no atomic decides it: a wave takes its items in order, finds the lanes holding the
//            same digit with eight ballots, and ranks by lane number; waves are ordered by a fixed walk over their counts.  The
//            tile is put in digit order in LDS first, so that the stores of a digit's run are contiguous.
//   gcount, rowscan   (tile_count_kernel<lv_is_g>, tile_rowscan_kernel) g bits per tile of the sorted order, scanned over the
//            tiles: F before every tile, and G as the row total
//   coef     F_i by ballots inside the tile (tile_rank), the increment in double from the integers, a = dL/dp scattered to coef
//            [B,K,H,W], one partial sum of e_(i) (J_i - J_{i-1}) / divisor per workgroup STORED as a row (block_store_row)
//   finalize one workgroup adds the rows in a fixed order in double (loss_pixel.h's rows_sum_f64)
// No float atomics anywhere: loss, coef and gradient have the same bits on every run.
#include "loss_pixel.h"
#include "tile_rank.h"

#define LV_BINS 256
#define LV_PASSES 4
enum { LV_IGNORE = 1, LV_PROBS = 2 };

// ---- keys -------------------------------------------------------------------------------------------------------------------------
// grid (gx * B), gx = ceil(HW / 1024): block -> image b = blockIdx.x / gx; a thread owns 4 pixels, consecutive lanes on
// consecutive pixels of every plane.  Segment s = c (n = B HW, element b HW + p) or b K + c with per_image (n = HW, element p).
template <typename T, int KM>
__global__ __launch_bounds__(256) void lv_keys_kernel(const T* __restrict__ in, const float* __restrict__ labels,
                                                     unsigned* __restrict__ keys, unsigned* __restrict__ pay, int K, int HW, int gx,
                                                     long n, int per_image, int flags, int ignore_index) {
  const int b = blockIdx.x / gx, bx = blockIdx.x - b * gx;
  const T* in0 = in + (long)b * K * HW;
  const float* lab = labels + (long)b * HW;
#pragma unroll 2
  for (int k = 0; k < 4; ++k) {
    const int p = (bx * 4 + k) * 256 + threadIdx.x;
    if (p >= HW) continue;
    float v[KM];
    px_load<KM>(v, in0, HW, p, K);
    const float t = lab[p];
    if (!(flags & LV_PROBS)) px_softmax<KM, true>(v, K);
    const bool ign = (flags & LV_IGNORE) && (int)t == ignore_index;
    const unsigned i = per_image ? (unsigned)p : (unsigned)b * (unsigned)HW + (unsigned)p;
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) {
        const bool g = !ign && t == (float)c;
        const float e = fabsf((g ? 1.f : 0.f) - v[c]);
        const long at = (long)(per_image ? b * K + c : c) * n + i;
        keys[at] = tile_key(e, !ign);
        pay[at] = (i << 1) | (g ? 1u : 0u);
      }
  }
}

// the sort alone (cenet_lovasz_order_f32): errors [S, n] -> keys, payload = index in the segment
__global__ __launch_bounds__(256) void lv_order_keys_kernel(const float* __restrict__ e, unsigned* __restrict__ keys,
                                                           unsigned* __restrict__ pay, long total, int n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    keys[i] = tile_key(e[i], true);
    pay[i] = (unsigned)(i % n) << 1;
  }
}
__global__ __launch_bounds__(256) void lv_order_out_kernel(const unsigned* __restrict__ pay, int* __restrict__ perm, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) perm[i] = (int)(pay[i] >> 1);
}

// ---- radix sort: one pass = hist, rowscan, scatter ------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned lv_digit(unsigned key, int shift) { return (LV_BINS - 1) - ((key >> shift) & (LV_BINS - 1)); }

// grid (T, S): counts[(s 256 + d) T + tile] = elements of the tile with digit d
__global__ __launch_bounds__(256) void lv_hist_kernel(const unsigned* __restrict__ keys, int* __restrict__ counts, int n, int T,
                                                     int shift) {
  __shared__ unsigned hist[LV_BINS];
  const int tile = blockIdx.x, s = blockIdx.y;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* k0 = keys + (long)s * n;
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const unsigned i = (unsigned)tile * TILE_ELEMS + k * 256 + threadIdx.x;
    if (i < (unsigned)n) atomicAdd(&hist[lv_digit(k0[i], shift)], 1u);
  }
  __syncthreads();
  counts[((long)s * LV_BINS + threadIdx.x) * T + tile] = (int)hist[threadIdx.x];
}

// grid (T, S).  Wave w owns elements [w 64 IT, (w + 1) 64 IT) of the tile, item k of lane l is element w 64 IT + 64 k + l: the order
// of the elements is (wave, item, lane), loads are coalesced.  counts: scanned by tile_rowscan_kernel; totals: the row totals.
__global__ __launch_bounds__(256) void lv_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ pin,
                                                        unsigned* __restrict__ kout, unsigned* __restrict__ pout,
                                                        const int* __restrict__ counts, const int* __restrict__ totals, int n, int T,
                                                        int shift) {
  __shared__ int wcnt_s[4][LV_BINS];
  __shared__ int wsum[4], wsum2[4], gdelta[LV_BINS];
  __shared__ unsigned skey[TILE_ELEMS], spay[TILE_ELEMS];
  // wcnt[w] is touched by wave w alone until the barrier behind the ranking loop.  Inside a wave no barrier is needed between
  // the leader's update at item k and another lane's read at item k + 1: the 64 lanes run one instruction stream, a wave's LDS
  // operations complete in issue order, and `volatile` keeps the compiler from caching or reordering the accesses.
  volatile int(*wcnt)[LV_BINS] = wcnt_s;
  const int tile = blockIdx.x, s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // thread t = digit t: elements of the segment with a smaller digit, plus this digit's in earlier tiles
  const int tot = totals[s * LV_BINS + threadIdx.x];
  const int inc = wave_incl_scan(tot);
  if (lane == 63) wsum[wave] = inc;
#pragma unroll
  for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  int mybase = inc - tot + counts[((long)s * LV_BINS + threadIdx.x) * T + tile];
  for (int w = 0; w < wave; ++w) mybase += wsum[w];

  const unsigned* k0 = kin + (long)s * n;
  const unsigned* p0 = pin + (long)s * n;
  const unsigned start = (unsigned)tile * TILE_ELEMS + wave * (64 * TILE_IT) + lane;
  const wave_mask_t below = ((wave_mask_t)1 << lane) - 1;
  unsigned key[TILE_IT], pv[TILE_IT];
  int loc[TILE_IT];
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const unsigned i = start + 64 * k;
    const bool valid = i < (unsigned)n;
    key[k] = valid ? k0[i] : 0u;
    pv[k] = valid ? p0[i] : 0u;
  }
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const bool valid = start + 64 * k < (unsigned)n;
    const unsigned d = lv_digit(key[k], shift);
    wave_mask_t m = wave_ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const wave_mask_t bal = wave_ballot(bit);
      m &= bit ? bal : ~bal;
    }
    if (!valid) m = (wave_mask_t)1 << lane;  // m: the valid lanes of this item with this lane's digit (this lane among them)
    const int leader = __builtin_ctzll(m);
    int pre = 0;
    if (valid && lane == leader) {
      pre = wcnt[wave][d];
      wcnt[wave][d] = pre + wave_popc(m);
    }
    pre = __shfl(pre, leader);
    loc[k] = pre + wave_popc(m & below);  // elements of this wave with this digit before this one
  }
  __syncthreads();
  // thread t = digit t: the tile sorted by digit is laid out in LDS first — tstart = the tile's elements with a smaller digit,
  // wcnt[w][t] <- the place in the tile of wave w's first element with digit t, gdelta[t] = global place - place in the tile
  int c[4], ttot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) ttot += c[w] = wcnt[w][threadIdx.x];
  const int tinc = wave_incl_scan(ttot);
  if (lane == 63) wsum2[wave] = tinc;
  __syncthreads();
  int run = tinc - ttot;
  for (int w = 0; w < wave; ++w) run += wsum2[w];
  gdelta[threadIdx.x] = mybase - run;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    wcnt[w][threadIdx.x] = run;
    run += c[w];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    if (start + 64 * k >= (unsigned)n) continue;
    const int pos = wcnt[wave][lv_digit(key[k], shift)] + loc[k];
    skey[pos] = key[k];
    spay[pos] = pv[k];
  }
  __syncthreads();
  // consecutive threads take consecutive places of the sorted tile: the stores of a digit's run are contiguous
  unsigned* ko = kout + (long)s * n;
  unsigned* po = pout + (long)s * n;
  const unsigned left = (unsigned)n - (unsigned)tile * TILE_ELEMS;
  const int count = left < TILE_ELEMS ? (int)left : TILE_ELEMS;
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const int j = k * 256 + threadIdx.x;
    if (j >= count) continue;
    const unsigned kv = skey[j];
    const unsigned dst = (unsigned)(gdelta[lv_digit(kv, shift)] + j);
    if (dst < (unsigned)n) {  // (always: the counts add up to n)
      ko[dst] = kv;
      po[dst] = spay[j];
    }
  }
}

// ---- ranks to coefficients ---------------------------------------------------------------------------------------------------------
// the g bit of a payload, for tile_count_kernel: gcnt[s T + tile] = pixels of the class in the tile of the sorted order
struct lv_is_g {
  __device__ unsigned seg(int) const { return 0u; }
  __device__ bool operator()(unsigned pay, unsigned) const { return pay & 1u; }
};

// grid (T, S), elements as in lv_scatter_kernel.  fbase: gcnt scanned (g bits before the tile); G: the row totals.
__global__ __launch_bounds__(256) void lv_coef_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ pay,
                                                     const int* __restrict__ fbase, const int* __restrict__ G,
                                                     float* __restrict__ coef, float* __restrict__ rows, int n, int T, int B, int K,
                                                     int HW, int per_image, int classes_all) {
  __shared__ int wtot[4];
  __shared__ float wred[4][1];
  const int tile = blockIdx.x, s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // 1 / divisor of this segment: the mean over the classes that count, with per_image then over the images
  const int Gs = G[s];
  double scale;
  if (classes_all) {
    scale = 1.0 / ((double)K * (per_image ? B : 1));
  } else {
    const int first = per_image ? (s / K) * K : 0;
    int present = 0;
    for (int c = 0; c < K; ++c) present += G[first + c] > 0;
    scale = Gs > 0 ? 1.0 / ((double)present * (per_image ? B : 1)) : 0.0;
  }
  const unsigned* k0 = keys + (long)s * n;
  const unsigned* p0 = pay + (long)s * n;
  const unsigned start = (unsigned)tile * TILE_ELEMS + wave * (64 * TILE_IT) + lane;
  unsigned key[TILE_IT], pv[TILE_IT];
  int incl[TILE_IT];
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const unsigned i = start + 64 * k;
    const bool in = i < (unsigned)n;
    key[k] = in ? k0[i] : 0u;
    pv[k] = in ? p0[i] : 0u;
  }
  const int Fb = fbase[(long)s * T + tile] + tile_rank<true>([&](int k) { return key[k] != 0u && (pv[k] & 1u); }, incl, wtot);
  float acc[1] = {0.f};
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const unsigned i = start + 64 * k;
    if (i >= (unsigned)n) continue;
    const bool g = pv[k] & 1u;
    float a = 0.f;
    if (key[k] != 0u) {  // (an ignored pixel: in no count, a = 0; they all sort behind the last valid one)
      const long F = (long)Fb + incl[k], Z = (long)i + 1 - F, U = Gs + Z, I = Gs - F;
      const double inc = g ? 1.0 / (double)U : (U == 1 ? 1.0 : (double)I / ((double)U * (double)(U - 1)));
      const float w = (float)(inc * scale);
      acc[0] += tile_key_value(key[k]) * w;
      a = key[k] == 1u ? 0.f : (g ? -w : w);  // e == 0: the gradient of |.| at 0 is 0
    }
    const unsigned pix = pv[k] >> 1;
    long at;
    if (per_image) {
      at = (long)s * HW + pix;
    } else {
      const unsigned b = pix / (unsigned)HW;
      at = ((long)b * K + s) * HW + (pix - b * (unsigned)HW);
    }
    coef[at] = a;
  }
  block_store_row(acc, wred, rows + (long)s * T + tile);
}

__global__ __launch_bounds__(1024) void lv_finalize_kernel(const float* __restrict__ rows, float* __restrict__ loss, long nrows) {
  __shared__ double acc[1][1024];
  double sum[1];
  rows_sum_f64(acc, nrows, [&](long r, int) { return (double)rows[r]; }, sum);
  if (threadIdx.x == 0) loss[0] = (float)sum[0];
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// grid (gx * B) as lv_keys_kernel: dlogits_j = gout p_j (a_j - sum_c p_c a_c), or gout a_j on probabilities
template <typename T, int KM>
__global__ __launch_bounds__(256) void lv_bwd_kernel(const T* __restrict__ in, const float* __restrict__ coef,
                                                    const float* __restrict__ gout, T* __restrict__ din, int K, int HW, int gx,
                                                    int probs) {
  const int b = blockIdx.x / gx, bx = blockIdx.x - b * gx;
  const float go = gout[0];
  const T* in0 = in + (long)b * K * HW;
  const float* a0 = coef + (long)b * K * HW;
  T* d0 = din + (long)b * K * HW;
#pragma unroll 2
  for (int k = 0; k < 4; ++k) {
    const int p = (bx * 4 + k) * 256 + threadIdx.x;
    if (p >= HW) continue;
    float v[KM], a[KM];
#pragma unroll
    for (int c = 0; c < KM; ++c)  // (class by class, a coefficient beside its input)
      if (c < K) {
        a[c] = a0[(long)c * HW + p];
        if (!probs) v[c] = ldf(in0 + (long)c * HW + p);
      }
    float dot = 0.f;
    if (!probs) {
      px_softmax<KM, true>(v, K);
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < K) dot += v[c] * a[c];
    }
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) stf(d0 + (long)c * HW + p, probs ? go * a[c] : go * v[c] * (a[c] - dot));
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
extern "C" int cenet_lovasz_tile(void) { return TILE_ELEMS; }

// the workspace, in 4-byte words: keys and payloads twice (the passes alternate), the digit counts [S, 256, T] and their row totals
// [S, 256], the g counts [S, T] and their totals G [S], the loss rows [S, T]
struct lv_ws_t {
  unsigned *kA, *pA, *kB, *pB;
  int *counts, *totals, *gcnt, *G;
  float* rows;
  long words;
};
static lv_ws_t lv_layout(void* ws, long S, long n) {
  const long T = cdiv(n, TILE_ELEMS), sn = S * n;
  unsigned* w = (unsigned*)ws;
  lv_ws_t L;
  L.kA = w, L.pA = w + sn, L.kB = w + 2 * sn, L.pB = w + 3 * sn;
  long at = 4 * sn;
  L.counts = (int*)(w + at), at += S * LV_BINS * T;
  L.totals = (int*)(w + at), at += S * LV_BINS;
  L.gcnt = (int*)(w + at), at += S * T;
  L.G = (int*)(w + at), at += S;
  L.rows = (float*)(w + at), at += S * T;
  L.words = at;
  return L;
}
static inline bool lv_shape_ok(int B, int K, int H, int W, int per_image, long* S, long* n) {  // a segment a class
  return K >= 2 && K <= PX_MAXK && tile_seg_shape_ok(B, H, W, per_image, K, S, n);
}

extern "C" long cenet_lovasz_order_ws_bytes(int S, int n) {
  if (!tile_seg_ok(S, n)) return 0;
  return 4 * lv_layout(nullptr, S, n).words;
}
extern "C" long cenet_lovasz_ws_bytes(int B, int K, int H, int W, int per_image) {
  long S, n;
  if (!lv_shape_ok(B, K, H, W, per_image, &S, &n)) return 0;
  return 4 * lv_layout(nullptr, S, n).words;
}

// keys / payloads in (kA, pA) -> sorted, in (kA, pA) again after the four passes
static int lv_sort(const lv_ws_t& L, int S, int n, hipStream_t stream) {
  const int T = cdiv(n, TILE_ELEMS);
  unsigned *ki = L.kA, *pi = L.pA, *ko = L.kB, *po = L.pB;
  for (int pass = 0; pass < LV_PASSES; ++pass) {
    const int shift = 8 * pass;
    CENET_LAUNCH(lv_hist_kernel, dim3(T, S), dim3(256), stream, (const unsigned*)ki, L.counts, n, T, shift);
    CENET_CHECK_LAUNCH();
    const int rc = tile_rowscan(L.counts, L.totals, (long)S * LV_BINS, T, stream);
    if (rc != CENET_OK) return rc;
    CENET_LAUNCH(lv_scatter_kernel, dim3(T, S), dim3(256), stream, (const unsigned*)ki, (const unsigned*)pi, ko, po,
                 (const int*)L.counts, (const int*)L.totals, n, T, shift);
    CENET_CHECK_LAUNCH();
    unsigned* t = ki;
    ki = ko, ko = t;
    t = pi, pi = po, po = t;
  }
  return CENET_OK;
}

extern "C" int cenet_lovasz_order_f32(const float* errors, void* ws, long ws_bytes, int* perm, int S, int n, hipStream_t stream) {
  if (!tile_seg_ok(S, n) || !errors || !ws || !perm || ws_bytes < cenet_lovasz_order_ws_bytes(S, n)) return CENET_EINVAL;
  const lv_ws_t L = lv_layout(ws, S, n);
  const long total = (long)S * n;
  const int blocks = (int)(cdiv(total, 256) < 4096 ? cdiv(total, 256) : 4096);
  CENET_LAUNCH(lv_order_keys_kernel, dim3(blocks), dim3(256), stream, errors, L.kA, L.pA, total, n);
  CENET_CHECK_LAUNCH();
  const int rc = lv_sort(L, S, n, stream);
  if (rc != CENET_OK) return rc;
  CENET_LAUNCH(lv_order_out_kernel, dim3(blocks), dim3(256), stream, (const unsigned*)L.pA, perm, total);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

template <typename T>
static int lovasz_fwd_impl(const T* inputs, const float* labels, void* ws, long ws_bytes, float* coef, float* loss, int B, int K,
                           int H, int W, int per_image, int classes_all, int has_ignore, int ignore_index, int from_probs,
                           hipStream_t stream) {
  long Sl, nl;
  if (!lv_shape_ok(B, K, H, W, per_image, &Sl, &nl)) return CENET_EINVAL;
  if (!inputs || !labels || !ws || !coef || !loss || ws_bytes < cenet_lovasz_ws_bytes(B, K, H, W, per_image)) return CENET_EINVAL;
  const int S = (int)Sl, n = (int)nl, HW = H * W, Tn = cdiv(n, TILE_ELEMS), gx = cdiv(HW, 1024);
  if ((long)gx * B >= (1L << 31)) return CENET_EINVAL;
  const lv_ws_t L = lv_layout(ws, S, n);
  const int flags = (has_ignore ? LV_IGNORE : 0) | (from_probs ? LV_PROBS : 0);
  const dim3 pg(gx * B);
  CENET_LAUNCH_KM(lv_keys_kernel, T, K, pg, dim3(256), stream, inputs, labels, L.kA, L.pA, K, HW, gx, nl, per_image, flags, ignore_index);
  CENET_CHECK_LAUNCH();
  int rc = lv_sort(L, S, n, stream);
  if (rc != CENET_OK) return rc;
  CENET_LAUNCH(tile_count_kernel<lv_is_g>, dim3(Tn, S), dim3(256), stream, (const unsigned*)L.pA, lv_is_g(), L.gcnt, n, Tn);
  CENET_CHECK_LAUNCH();
  rc = tile_rowscan(L.gcnt, L.G, S, Tn, stream);
  if (rc != CENET_OK) return rc;
  CENET_LAUNCH(lv_coef_kernel, dim3(Tn, S), dim3(256), stream, (const unsigned*)L.kA, (const unsigned*)L.pA, (const int*)L.gcnt,
               (const int*)L.G, coef, L.rows, n, Tn, B, K, HW, per_image, classes_all);
  CENET_CHECK_LAUNCH();
  CENET_LAUNCH(lv_finalize_kernel, dim3(1), dim3(1024), stream, (const float*)L.rows, loss, (long)S * Tn);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(lovasz_fwd, (const T* inputs, const float* labels, void* ws, long ws_bytes, float* coef, float* loss, int B, int K, int H,
                        int W, int per_image, int classes_all, int has_ignore, int ignore_index, int from_probs, hipStream_t stream),
           (inputs, labels, ws, ws_bytes, coef, loss, B, K, H, W, per_image, classes_all, has_ignore, ignore_index, from_probs, stream))

template <typename T>
static int lovasz_bwd_impl(const T* inputs, const float* coef, const float* gout, T* dinputs, int B, int K, int H, int W,
                           int from_probs, hipStream_t stream) {
  if (B < 1 || K < 2 || K > PX_MAXK || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return CENET_EINVAL;
  if (!inputs || !coef || !gout || !dinputs || (const void*)inputs == (const void*)dinputs) return CENET_EINVAL;
  const int HW = H * W, gx = cdiv(HW, 1024);
  if ((long)gx * B >= (1L << 31)) return CENET_EINVAL;
  const dim3 pg(gx * B);
  CENET_LAUNCH_KM(lv_bwd_kernel, T, K, pg, dim3(256), stream, inputs, coef, gout, dinputs, K, HW, gx, from_probs);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(lovasz_bwd, (const T* inputs, const float* coef, const float* gout, T* dinputs, int B, int K, int H, int W, int from_probs,
                        hipStream_t stream),
           (inputs, coef, gout, dinputs, B, K, H, W, from_probs, stream))
