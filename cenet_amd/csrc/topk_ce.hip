// topk_ce.hip — top-k cross-entropy (hard-pixel mining; the CE half of nnU-Net's DC_and_topk_loss) on the device: keys, a radix
// SELECT of the k-th order statistic, a tie rank, weights, backward.  include/cenet_hip.h spells the definition out; in short,
// per segment (the batch, or one image with per_image) the m = max(1, floor(n_valid k / 100)) valid pixels with the largest
// l = logsumexp(x) - x_y are kept, equal l by ascending pixel index, and the loss is the mean of l over them.
//
// LAUNCHES of a forward (stream order is the only synchronisation, nothing is read back, no host decision):
//   zero     the integer bins and counters of the workspace
//   keys     one pass over logits and labels: fp32 log-softmax, key = bits(l) + 1 (non-negative floats order as their bits; key
//            0 = invalid pixel, below every valid one) stored as [S, n]; the digit histogram of round 0 and the count of valid
//            pixels in the same pass (LDS bins per workgroup, then integer atomics into the segment's bins: COUNTS only)
//   pick 0, 3 x (hist, pick)   the select: round r looks at the 8 bits below the 8 r already fixed.  hist counts that digit over the
//            keys whose higher bits equal the prefix found so far; pick (one workgroup a segment) walks the 256 bins from the top
//            to the digit at which the running count reaches the remaining quota, extends the prefix and takes what lies above
//            off the quota.  Round 0 derives n_valid and m.  After round 3: the threshold key tau and r = how many of the pixels
//            with key == tau are kept.  No key moves.
//   tiecount, scan   (tile_rank.h's tile_count_kernel<tk_is_tie>, tile_rowscan_kernel) pixels with key == tau per tile of TILE_ELEMS
//            elements, scanned over the tiles of a segment
//   weights  rank among the ties = ties in earlier tiles + earlier in this tile (tile_rank: ballots and the lane number, no atomic
//            decides an order); kept iff key > tau, or key == tau and rank < r; wgt = 1 / (m S_valid) or 0; one partial sum of the
//            kept l per workgroup STORED as a row (block_store_row)
//   finalize one workgroup adds the rows in a fixed order in double (loss_pixel.h's rows_sum_f64)
// No float atomics anywhere: loss, wgt and gradient have the same bits on every run.
#include "loss_pixel.h"
#include "tile_rank.h"

#define TK_BINS 256
#define TK_ROUNDS 4
#define TK_KEYS_IT 4     // pixels a thread of the keys pass takes
#define TK_HIST_WGS 4096 // workgroups of a histogram launch over all segments, at most
#define TK_COPIES 8      // copies of a segment's bins, at most (tk_copies)
enum { TK_PREFIX = 0, TK_QUOTA = 1, TK_M = 2, TK_STATE = 4 };  // the state words of a segment

// ---- keys -------------------------------------------------------------------------------------------------------------------------
// The bins of a workgroup go into the segment's: counts[d] += hist[d] by an integer atomic (a count, whatever the order).  Atomics
// on one word go one after the other, and with one segment every workgroup of a launch ends on the same few words: a segment has
// C copies of its bins (and of its count of valid pixels), workgroup x adds into copy x % C, pick adds the copies up.
__device__ __forceinline__ void tk_flush_bins(const int* hist, int* bins) {
  const int h = hist[threadIdx.x];
  if (h) atomicAdd(&bins[threadIdx.x], h);
}
__device__ __forceinline__ long tk_bins_at(int s, int round, int copy, int C) {
  return (((long)s * TK_ROUNDS + round) * C + copy) * TK_BINS;
}

// grid (gx * B), gx = ceil(HW / (256 TK_KEYS_IT)): block -> image b = blockIdx.x / gx; a thread owns TK_KEYS_IT pixels, consecutive
// lanes on consecutive pixels of every plane.  Segment s = 0 (n = B HW, element b HW + p) or b with per_image
// (n = HW, element p).
// The label picks x_y by comparison and is never an index.
template <typename T, int KM>
__global__ __launch_bounds__(256) void tk_keys_kernel(const T* __restrict__ in, const float* __restrict__ labels,
                                                     unsigned* __restrict__ keys, int* __restrict__ bins, int* __restrict__ nvalid,
                                                     int K, int HW, int gx, int per_image, int has_ignore, int ignore_index, int C) {
  __shared__ int hist[TK_BINS];
  __shared__ int wvalid[4];
  const int b = blockIdx.x / gx, bx = blockIdx.x - b * gx;
  const T* in0 = in + (long)b * K * HW;
  const float* lab = labels + (long)b * HW;
  unsigned* k0 = keys + (long)b * HW;  // ([S, n] with either kind of segment is [B, HW])
  hist[threadIdx.x] = 0;
  __syncthreads();
  int cnt = 0;
#pragma unroll 2
  for (int k = 0; k < TK_KEYS_IT; ++k) {
    const long p = ((long)bx * TK_KEYS_IT + k) * 256 + threadIdx.x;  // (long: the last block may reach past 2^31)
    const bool in_range = p < HW;
    unsigned key = 0u;
    if (in_range) {
      float v[KM];
      px_load<KM>(v, in0, HW, p, K);
      const float t = lab[p];
      float mx = -3.4e38f;
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < K) mx = fmaxf(mx, v[c]);
      float s = 0.f, xy = 0.f;
      bool hit = false;
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < K) {
          const float d = v[c] - mx;
          s += expf(d);  // libm's, as lovasz.hip: the order of near-equal losses follows the last bits
          if (t == (float)c) xy = d, hit = true;
        }
      const bool valid = hit && !(has_ignore && (int)t == ignore_index);
      const float l = fmaxf(logf(s) - xy, 0.f);
      key = tile_key(l, valid);
      k0[p] = key;
      atomicAdd(&hist[key >> 24], 1);
    }
    cnt += wave_popc(wave_ballot(key != 0u));
  }
  if ((threadIdx.x & 63) == 0) wvalid[threadIdx.x >> 6] = cnt;
  __syncthreads();
  const int s = per_image ? b : 0, copy = blockIdx.x % C;
  tk_flush_bins(hist, bins + tk_bins_at(s, 0, copy, C));
  if (threadIdx.x == 0) atomicAdd(&nvalid[s * C + copy], (wvalid[0] + wvalid[1]) + (wvalid[2] + wvalid[3]));
}

// the selection alone (cenet_topk_mask_f32), grid (tk_hist_wgs, S), a workgroup takes the tiles blockIdx.x, + gridDim.x, ...:
// values [S, n] -> keys (every element valid) and the round-0 bins
__global__ __launch_bounds__(256) void tk_value_keys_kernel(const float* __restrict__ values, unsigned* __restrict__ keys,
                                                           int* __restrict__ bins, int n, int T, int C) {
  __shared__ int hist[TK_BINS];
  const int s = blockIdx.y;
  hist[threadIdx.x] = 0;
  __syncthreads();
  for (int tile = blockIdx.x; tile < T; tile += gridDim.x) {
#pragma unroll
    for (int k = 0; k < TILE_IT; ++k) {
      const unsigned i = (unsigned)tile * TILE_ELEMS + k * 256 + threadIdx.x;
      if (i < (unsigned)n) {
        const unsigned key = tile_key(values[(long)s * n + i], true);
        keys[(long)s * n + i] = key;
        atomicAdd(&hist[key >> 24], 1);
      }
    }
  }
  __syncthreads();
  tk_flush_bins(hist, bins + tk_bins_at(s, 0, blockIdx.x % C, C));
}

// ---- radix select: hist, pick ----------------------------------------------------------------------------------------------------------
// grid (tk_hist_wgs, S), round 1 .. 3, a workgroup takes the tiles blockIdx.x, + gridDim.x, ...: bins[s][round][d] += keys of
// those tiles whose bits above the round's digit equal the prefix's
__global__ __launch_bounds__(256) void tk_hist_kernel(const unsigned* __restrict__ keys, const int* __restrict__ state,
                                                     int* __restrict__ bins, int n, int T, int round, int C) {
  __shared__ int hist[TK_BINS];
  const int s = blockIdx.y;
  const int shift = 24 - 8 * round;
  const unsigned high = (unsigned)state[s * TK_STATE + TK_PREFIX] >> (shift + 8);
  hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* k0 = keys + (long)s * n;
  for (int tile = blockIdx.x; tile < T; tile += gridDim.x) {
#pragma unroll
    for (int k = 0; k < TILE_IT; ++k) {
      const unsigned i = (unsigned)tile * TILE_ELEMS + k * 256 + threadIdx.x;
      if (i < (unsigned)n) {
        const unsigned key = k0[i];
        if ((key >> (shift + 8)) == high) atomicAdd(&hist[(key >> shift) & (TK_BINS - 1)], 1);
      }
    }
  }
  __syncthreads();
  tk_flush_bins(hist, bins + tk_bins_at(s, round, blockIdx.x % C, C));
}

// grid (S), 256 threads: thread t holds the bin of digit 255 - t, so that an inclusive scan over the threads counts from the top.
// Round 0 sets the quota: m_in[s] (the selection alone; clamped into [0, n]) or m = max(1, floor(n_valid k / 100)) with k read
// from the device and clamped into (0, 100]; a segment without a valid pixel keeps nothing (m = 0).  svalid counts the segments
// that keep something (an integer atomic: a count).
__global__ __launch_bounds__(256) void tk_pick_kernel(const int* __restrict__ bins, int* __restrict__ state,
                                                     const int* __restrict__ nvalid, int* __restrict__ svalid,
                                                     const float* __restrict__ kpercent, const int* __restrict__ m_in, int n,
                                                     int round, int C) {
  __shared__ int wsum[4];
  const int s = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int* st = state + s * TK_STATE;
  unsigned prefix = 0u;
  int quota;
  if (round == 0) {
    if (m_in) {
      quota = m_in[s] < 0 ? 0 : (m_in[s] > n ? n : m_in[s]);
    } else {
      int nv = 0;
      for (int j = 0; j < C; ++j) nv += nvalid[s * C + j];
      float k = kpercent[0];
      k = k > 100.f ? 100.f : k;
      if (!(k > 0.f)) k = 0.f;
      long long m = (long long)((double)nv * (double)k / 100.0);
      if (m < 1) m = 1;
      quota = nv > 0 ? (int)m : 0;
    }
  } else {
    prefix = (unsigned)st[TK_PREFIX];
    quota = st[TK_QUOTA];
  }
  const int d = (TK_BINS - 1) - threadIdx.x;
  int c = 0;
  for (int j = 0; j < C; ++j) c += bins[tk_bins_at(s, round, j, C) + d];
  int incl = wave_incl_scan(c);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += wsum[w];
  const int above = incl - c;  // keys of the candidates with a larger digit
  if (round == 0 && threadIdx.x == 0) {
    st[TK_M] = quota;
    if (quota == 0) st[TK_PREFIX] = (int)0xFFFFFFFFu, st[TK_QUOTA] = 0;  // tau above every key: nothing is kept
    else atomicAdd(svalid, 1);
  }
  // exactly one digit has above < quota <= above + c when 1 <= quota <= the candidates' count (which it is: the quota never
  // exceeds the count of the bin picked a round earlier, nor n_valid in round 0)
  if (quota > 0 && above < quota && quota <= incl) {
    st[TK_PREFIX] = (int)(prefix | ((unsigned)d << (24 - 8 * round)));
    st[TK_QUOTA] = quota - above;
  }
}

// ---- tie rank, weights, loss ----------------------------------------------------------------------------------------------------------
// key == tau of the segment, for tile_count_kernel: tcnt[s T + tile] = keys of the tile equal to tau
struct tk_is_tie {
  const int* state;
  __device__ unsigned seg(int s) const { return (unsigned)state[s * TK_STATE + TK_PREFIX]; }
  __device__ bool operator()(unsigned key, unsigned tau) const { return key == tau; }
};

// grid (T, S).  Wave w owns elements [w 64 IT, (w + 1) 64 IT) of the tile, item k of lane l is element w 64 IT + 64 k + l: the order
// (wave, item, lane) is the order of the pixel index.  tbase: tcnt scanned over the tiles.  wgt / mask: either may be null.
__global__ __launch_bounds__(256) void tk_weights_kernel(const unsigned* __restrict__ keys, const int* __restrict__ state,
                                                        const int* __restrict__ tbase, const int* __restrict__ svalid,
                                                        float* __restrict__ wgt, unsigned char* __restrict__ mask,
                                                        float* __restrict__ rows, int n, int T) {
  __shared__ int wtot[4];
  __shared__ float wred[4][1];
  const int tile = blockIdx.x, s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned tau = (unsigned)state[s * TK_STATE + TK_PREFIX];
  const int r = state[s * TK_STATE + TK_QUOTA], m = state[s * TK_STATE + TK_M];
  const float w = m > 0 ? (float)(1.0 / ((double)m * (double)svalid[0])) : 0.f;
  const unsigned* k0 = keys + (long)s * n;
  const unsigned start = (unsigned)tile * TILE_ELEMS + wave * (64 * TILE_IT) + lane;
  unsigned key[TILE_IT];
  int before[TILE_IT];
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) key[k] = start + 64 * k < (unsigned)n ? k0[start + 64 * k] : 0u;
  const int base = tbase[(long)s * T + tile] +
                   tile_rank<false>([&](int k) { return start + 64 * k < (unsigned)n && key[k] == tau; }, before, wtot);
  float acc[1] = {0.f};
#pragma unroll
  for (int k = 0; k < TILE_IT; ++k) {
    const unsigned i = start + 64 * k;
    if (i >= (unsigned)n) continue;
    const bool kept = m > 0 && key[k] != 0u && (key[k] > tau || (key[k] == tau && base + before[k] < r));
    if (kept) acc[0] += tile_key_value(key[k]);
    if (wgt) wgt[(long)s * n + i] = kept ? w : 0.f;
    if (mask) mask[(long)s * n + i] = kept ? 1 : 0;
  }
  block_store_row(acc, wred, rows + (long)s * T + tile);
}

// the rows over m_s S_valid
__global__ __launch_bounds__(1024) void tk_finalize_kernel(const float* __restrict__ rows, const int* __restrict__ state,
                                                          const int* __restrict__ svalid, float* __restrict__ loss, long nrows,
                                                          int T) {
  __shared__ double acc[1][1024];
  const double sv = (double)svalid[0];
  double sum[1];
  rows_sum_f64(acc, nrows, [&](long r, int) {
    const int m = state[(r / T) * TK_STATE + TK_M];
    return m > 0 ? (double)rows[r] / ((double)m * sv) : 0.0;  // (a sum that starts at +0 stays as it is under + 0)
  }, sum);
  if (threadIdx.x == 0) loss[0] = (float)sum[0];
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// grid (gx * B) as tk_keys_kernel: dlogits_j = gout wgt (p_j - [j == y]); a pixel with wgt == 0 gets exact zeros
template <typename T, int KM>
__global__ __launch_bounds__(256) void tk_bwd_kernel(const T* __restrict__ in, const float* __restrict__ labels,
                                                    const float* __restrict__ wgt, const float* __restrict__ gout,
                                                    T* __restrict__ din, int K, int HW, int gx) {
  const int b = blockIdx.x / gx, bx = blockIdx.x - b * gx;
  const float go = gout[0];
  const T* in0 = in + (long)b * K * HW;
  T* d0 = din + (long)b * K * HW;
#pragma unroll 2
  for (int k = 0; k < 4; ++k) {
    const long p = ((long)bx * 4 + k) * 256 + threadIdx.x;
    if (p >= HW) continue;
    const float w = wgt[(long)b * HW + p];
    if (w == 0.f) {
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < K) stf(d0 + (long)c * HW + p, 0.f);
      continue;
    }
    const float t = labels[(long)b * HW + p];
    float v[KM];
    px_load<KM>(v, in0, HW, p, K);
    px_softmax<KM, true>(v, K);
    const float gw = go * w;
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) stf(d0 + (long)c * HW + p, gw * (v[c] - (t == (float)c ? 1.f : 0.f)));
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
extern "C" int cenet_topk_tile(void) { return TILE_ELEMS; }

// the workspace, in 4-byte words: what the zero launch clears first — the bins [S, 4, C, 256], n_valid [S, C], S_valid [1] —, then the
// state [S, 4], the tie counts [S, T], the loss rows [S, T] and the keys [S, n]
// copies of a segment's bins: 8 for up to 8 segments, fewer as the segments themselves spread the atomics, 1 from 64 segments on
static inline int tk_copies(long S) {
  const long c = 64 / S;
  return c < 1 ? 1 : (c > TK_COPIES ? TK_COPIES : (int)c);
}
struct tk_ws_t {
  int *bins, *nvalid, *svalid, *state, *tcnt;
  float* rows;
  unsigned* keys;
  long zero_words, words;
};
static tk_ws_t tk_layout(void* ws, long S, long n) {
  const long T = cdiv(n, TILE_ELEMS);
  int* w = (int*)ws;
  tk_ws_t L;
  long at = 0;
  const long C = tk_copies(S);
  L.bins = w + at, at += S * TK_ROUNDS * C * TK_BINS;
  L.nvalid = w + at, at += S * C;
  L.svalid = w + at, at += 1;
  L.zero_words = at;
  L.state = w + at, at += S * TK_STATE;
  L.tcnt = w + at, at += S * T;
  L.rows = (float*)(w + at), at += S * T;
  L.keys = (unsigned*)(w + at), at += S * n;
  L.words = at;
  return L;
}
// workgroups a segment of a histogram launch: all its tiles, or its share of TK_HIST_WGS
static inline int tk_hist_wgs(int T, int S) {
  const int share = TK_HIST_WGS / S < 1 ? 1 : TK_HIST_WGS / S;
  return T < share ? T : share;
}

extern "C" long cenet_topk_mask_ws_bytes(int S, int n) {
  if (!tile_seg_ok(S, n)) return 0;
  return 4 * tk_layout(nullptr, S, n).words;
}
extern "C" long cenet_topk_ce_ws_bytes(int B, int H, int W, int per_image) {
  long S, n;
  if (!tile_seg_shape_ok(B, H, W, per_image, 1, &S, &n)) return 0;
  return 4 * tk_layout(nullptr, S, n).words;
}

// keys and the round-0 bins are in place -> state (tau, r, m), then wgt / mask and the loss rows
static int tk_select(const tk_ws_t& L, const float* kpercent, const int* m_in, float* wgt, unsigned char* mask, int S, int n,
                     hipStream_t stream) {
  const int T = cdiv(n, TILE_ELEMS), C = tk_copies(S);
  for (int round = 0; round < TK_ROUNDS; ++round) {
    if (round > 0) {
      CENET_LAUNCH(tk_hist_kernel, dim3(tk_hist_wgs(T, S), S), dim3(256), stream, (const unsigned*)L.keys, (const int*)L.state, L.bins,
                   n, T, round, C);
      CENET_CHECK_LAUNCH();
    }
    CENET_LAUNCH(tk_pick_kernel, dim3(S), dim3(256), stream, (const int*)L.bins, L.state, (const int*)L.nvalid, L.svalid, kpercent,
                 m_in, n, round, C);
    CENET_CHECK_LAUNCH();
  }
  CENET_LAUNCH(tile_count_kernel<tk_is_tie>, dim3(T, S), dim3(256), stream, (const unsigned*)L.keys, tk_is_tie{L.state}, L.tcnt, n, T);
  CENET_CHECK_LAUNCH();
  const int rc = tile_rowscan(L.tcnt, nullptr, S, T, stream);
  if (rc != CENET_OK) return rc;
  CENET_LAUNCH(tk_weights_kernel, dim3(T, S), dim3(256), stream, (const unsigned*)L.keys, (const int*)L.state, (const int*)L.tcnt,
               (const int*)L.svalid, wgt, mask, L.rows, n, T);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_topk_mask_f32(const float* values, const int* m, void* ws, long ws_bytes, unsigned char* mask, int S, int n,
                                   hipStream_t stream) {
  if (!tile_seg_ok(S, n) || !values || !m || !ws || !mask || ws_bytes < cenet_topk_mask_ws_bytes(S, n)) return CENET_EINVAL;
  const tk_ws_t L = tk_layout(ws, S, n);
  int rc = cenet_zero_async((float*)L.bins, L.zero_words, stream);  // (the bits of 0.f are those of the integer 0)
  if (rc != CENET_OK) return rc;
  const int T = cdiv(n, TILE_ELEMS);
  CENET_LAUNCH(tk_value_keys_kernel, dim3(tk_hist_wgs(T, S), S), dim3(256), stream, values, L.keys, L.bins, n, T, tk_copies(S));
  CENET_CHECK_LAUNCH();
  return tk_select(L, nullptr, m, nullptr, mask, S, n, stream);
}

template <typename T>
static int topk_ce_fwd_impl(const T* logits, const float* labels, const float* kpercent, void* ws, long ws_bytes, float* wgt,
                            float* loss, int B, int K, int H, int W, int per_image, int has_ignore, int ignore_index,
                            hipStream_t stream) {
  long Sl, nl;
  if (K < 2 || K > PX_MAXK || !tile_seg_shape_ok(B, H, W, per_image, 1, &Sl, &nl)) return CENET_EINVAL;
  if (!logits || !labels || !kpercent || !ws || !wgt || !loss || ws_bytes < cenet_topk_ce_ws_bytes(B, H, W, per_image))
    return CENET_EINVAL;
  const int S = (int)Sl, n = (int)nl, HW = H * W, Tn = cdiv(n, TILE_ELEMS), gx = cdiv(HW, 256 * TK_KEYS_IT);
  if ((long)gx * B >= (1L << 31)) return CENET_EINVAL;
  const tk_ws_t L = tk_layout(ws, S, n);
  int rc = cenet_zero_async((float*)L.bins, L.zero_words, stream);  // (the bits of 0.f are those of the integer 0)
  if (rc != CENET_OK) return rc;
  const dim3 pg(gx * B);
  const int C = tk_copies(S);
  CENET_LAUNCH_KM(tk_keys_kernel, T, K, pg, dim3(256), stream, logits, labels, L.keys, L.bins, L.nvalid, K, HW, gx, per_image, has_ignore, ignore_index, C);
  CENET_CHECK_LAUNCH();
  rc = tk_select(L, kpercent, nullptr, wgt, nullptr, S, n, stream);
  if (rc != CENET_OK) return rc;
  CENET_LAUNCH(tk_finalize_kernel, dim3(1), dim3(1024), stream, (const float*)L.rows, (const int*)L.state, (const int*)L.svalid, loss,
               (long)S * Tn, Tn);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(topk_ce_fwd, (const T* logits, const float* labels, const float* kpercent, void* ws, long ws_bytes, float* wgt, float* loss,
                         int B, int K, int H, int W, int per_image, int has_ignore, int ignore_index, hipStream_t stream),
           (logits, labels, kpercent, ws, ws_bytes, wgt, loss, B, K, H, W, per_image, has_ignore, ignore_index, stream))

template <typename T>
static int topk_ce_bwd_impl(const T* logits, const float* labels, const float* wgt, const float* gout, T* dlogits, int B, int K,
                            int H, int W, int has_ignore, int ignore_index, hipStream_t stream) {
  (void)has_ignore, (void)ignore_index;  // (an ignored pixel has wgt == 0 from the forward)
  if (B < 1 || K < 2 || K > PX_MAXK || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return CENET_EINVAL;
  if (!logits || !labels || !wgt || !gout || !dlogits || (const void*)logits == (const void*)dlogits) return CENET_EINVAL;
  const int HW = H * W, gx = cdiv(HW, 1024);
  if ((long)gx * B >= (1L << 31)) return CENET_EINVAL;
  const dim3 pg(gx * B);
  CENET_LAUNCH_KM(tk_bwd_kernel, T, K, pg, dim3(256), stream, logits, labels, wgt, gout, dlogits, K, HW, gx);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
CENET_TWIN(topk_ce_bwd, (const T* logits, const float* labels, const float* wgt, const float* gout, T* dlogits, int B, int K, int H,
                         int W, int has_ignore, int ignore_index, hipStream_t stream),
           (logits, labels, wgt, gout, dlogits, B, K, H, W, has_ignore, ignore_index, stream))
