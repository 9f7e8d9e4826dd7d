// edt.hip — surface metrics by an exact distance transform (evaluate.label_metrics, surface_distances(method="edt")).
// medpy's __surface_distances reads the Euclidean distance transform of the complement of one border at the voxels of the other
// border; metrics.hip restates that as an all-pairs minimum, which is quadratic in the border sizes.  Here the transform itself
// runs on the device: linear in the number of voxels, whatever the masks look like.  With unit spacing every squared distance is
// an integer and the transform is integer arithmetic; with a voxel spacing (cenet_edt_sq_spaced_u8) the line passes that carry a
// weight run in fp64.  No atomics in either transform: bit-reproducible.
//   label_borders_kernel   one pass over two label volumes: per class the border flags of both, the overlap counts, the border
//                          counts and the borders' bounding boxes
//   edt_x_kernel           squared distance to the nearest feature voxel within each row, rows staged through LDS
//   edt_line_kernel        g[j] + (u - j)^2 minimised over j along y or z: lower envelope of parabolas with the integer Sep of
//                          Meijster, Roerdink & Hesselink (2000), one thread per line, consecutive lanes = consecutive x
//   edt_line_w_kernel      the same line pass with a voxel spacing, in fp64: g[j] + w2 (u - j)^2 (cenet_edt_sq_spaced_u8)
//   border_count / border_gather   order-preserving compaction of a border: coordinates (for the all-pairs kernel) or the
//                          transform's values (int32, or fp64 for the spaced transform) in C order of the border voxels
//   dm_labels / dm_logits / dm_merge   boundary-distance maps of a stack of 2-D class planes for the distance-map losses
//                          (dist_loss.hip): the planes' masks and their complements as one stack of features, the x and y passes
//                          above over that stack, and the sum of the two halves
#include "common.h"
#include "../../include/cenet_hip.h"

#define EDT_INF 0x7fffffff

static inline unsigned edt_cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }

// ---- label volumes -> border labels + per-class table ------------------------------------------------------------------------
// table row c (CENET_LB_COLS ints): 0 |pred==c & gt==c|, 1 |pred==c|, 2 |gt==c|, 3 |border(pred==c)|, 4 |border(gt==c)|,
// 5-7 min (z, y, x) of the pred border, 8-10 min of (-z, -y, -x) (i.e. minus the maximum), 11-16 the same for the gt border.
// The caller zeroes columns 0-4 and fills 5-16 with INT_MAX.  Integer atomics only: exact and order-independent.
#define LB_MAXK 64
__device__ __forceinline__ int lb_class(float v, int K) {
  const int c = (int)v;
  return (v >= 1.f && v < (float)K && (float)c == v) ? c : 0;
}
__device__ __forceinline__ bool lb_border(const float* __restrict__ vol, long i, float v, int x, int y, int z, int D, int H, int W,
                                          int zfaces) {
  const long sz = (long)H * W;
  bool interior = x > 0 && x + 1 < W && y > 0 && y + 1 < H && vol[i - 1] == v && vol[i + 1] == v && vol[i - W] == v &&
                  vol[i + W] == v;
  if (zfaces) interior = interior && z > 0 && z + 1 < D && vol[i - sz] == v && vol[i + sz] == v;
  return !interior;
}
__global__ __launch_bounds__(256) void label_borders_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           unsigned char* __restrict__ blp, unsigned char* __restrict__ blg,
                                                           int* __restrict__ table, int K, int D, int H, int W, int zfaces) {
  __shared__ int acc[LB_MAXK * CENET_LB_COLS];
  const int nacc = K * CENET_LB_COLS;
  for (int k = threadIdx.x; k < nacc; k += 256) acc[k] = (k % CENET_LB_COLS) < 5 ? 0 : EDT_INF;
  __syncthreads();
  const long n = (long)D * H * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float p = pred[i], g = gt[i];
    const int cp = lb_class(p, K), cg = lb_class(g, K);
    unsigned char bp = 0, bg = 0;
    if (cp | cg) {
      const int x = (int)(i % W);
      const long t = i / W;
      const int y = (int)(t % H);
      const int z = (int)(t / H);
      if (cp) {
        int* a = acc + cp * CENET_LB_COLS;
        atomicAdd(&a[1], 1);
        if (cg == cp) atomicAdd(&a[0], 1);
        if (lb_border(pred, i, p, x, y, z, D, H, W, zfaces)) {
          bp = (unsigned char)cp;
          atomicAdd(&a[3], 1);
          atomicMin(&a[5], z), atomicMin(&a[6], y), atomicMin(&a[7], x);
          atomicMin(&a[8], -z), atomicMin(&a[9], -y), atomicMin(&a[10], -x);
        }
      }
      if (cg) {
        int* a = acc + cg * CENET_LB_COLS;
        atomicAdd(&a[2], 1);
        if (lb_border(gt, i, g, x, y, z, D, H, W, zfaces)) {
          bg = (unsigned char)cg;
          atomicAdd(&a[4], 1);
          atomicMin(&a[11], z), atomicMin(&a[12], y), atomicMin(&a[13], x);
          atomicMin(&a[14], -z), atomicMin(&a[15], -y), atomicMin(&a[16], -x);
        }
      }
    }
    blp[i] = bp;
    blg[i] = bg;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nacc; k += 256) {
    const int v = acc[k];
    if ((k % CENET_LB_COLS) < 5) {
      if (v) atomicAdd(&table[k], v);
    } else if (v != EDT_INF) {
      atomicMin(&table[k], v);
    }
  }
}

// ---- x pass ------------------------------------------------------------------------------------------------------------------
// A workgroup owns EX_ROWS consecutive rows and walks them in chunks of EX_COLS columns: the chunk is loaded with consecutive
// lanes on consecutive x, one thread per row sweeps it in LDS carrying the position of the last feature voxel across chunks, and
// the chunk is written back the way it was loaded.  Forward sweep (distance to the feature on the left) over all chunks, then
// the backward sweep over the chunks in reverse, which also squares.  The row pitch of EX_COLS + 1 dwords puts the EX_ROWS
// sweeping threads on distinct banks.
#define EX_ROWS 128
#define EX_COLS 64
__global__ __launch_bounds__(256) void edt_x_kernel(const unsigned char* __restrict__ feat, int match, int* __restrict__ d2,
                                                   long rows, int W) {
  __shared__ int tile[EX_ROWS][EX_COLS + 1];
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
  const long r0 = (long)blockIdx.x * EX_ROWS;
  const int nr = (rows - r0 < EX_ROWS) ? (int)(rows - r0) : EX_ROWS;
  const int nchunk = (W + EX_COLS - 1) / EX_COLS;
  int last = -1;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int x0 = ch * EX_COLS;
    const int nc = (W - x0 < EX_COLS) ? W - x0 : EX_COLS;
    if (col < nc)
      for (int r = rg; r < nr; r += 4) {
        const unsigned char v = feat[(r0 + r) * W + x0 + col];
        tile[r][col] = match < 0 ? (v != 0) : (v == (unsigned char)match);
      }
    __syncthreads();
    if (tid < nr)
      for (int c = 0; c < nc; ++c) {
        if (tile[tid][c]) last = x0 + c;
        tile[tid][c] = last < 0 ? EDT_INF : x0 + c - last;
      }
    __syncthreads();
    if (col < nc)
      for (int r = rg; r < nr; r += 4) d2[(r0 + r) * W + x0 + col] = tile[r][col];
    __syncthreads();
  }
  int next = -1;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int x0 = ch * EX_COLS;
    const int nc = (W - x0 < EX_COLS) ? W - x0 : EX_COLS;
    if (col < nc)
      for (int r = rg; r < nr; r += 4) tile[r][col] = d2[(r0 + r) * W + x0 + col];
    __syncthreads();
    if (tid < nr)
      for (int c = nc - 1; c >= 0; --c) {
        int d = tile[tid][c];
        if (d == 0) next = x0 + c;
        if (next >= 0 && next - (x0 + c) < d) d = next - (x0 + c);
        tile[tid][c] = d == EDT_INF ? EDT_INF : d * d;
      }
    __syncthreads();
    if (col < nc)
      for (int r = rg; r < nr; r += 4) d2[(r0 + r) * W + x0 + col] = tile[r][col];
    __syncthreads();
  }
}

// ---- y / z pass --------------------------------------------------------------------------------------------------------------
// out[u] = min over j with g[j] finite of g[j] + (u - j)^2 along a line of m elements `es` apart; line = (blockIdx.y, i) starts at
// blockIdx.y * outer_stride + i, so consecutive lanes hold consecutive x and every access to g and out is a row segment.
// Meijster's two scans: the first builds the lower envelope as a stack of (s = site, t = first position where it wins), the second
// walks down from m - 1 and reads it off.  The stack lives in the line's own slots of `out`, s and t packed into one int (both
// < 65536): entry q is only ever at slot q <= t[q] <= u, so the second scan overwrites a slot only after its entry was popped.
__device__ __forceinline__ int edt_f(int u, int s, int gs) { return (u - s) * (u - s) + gs; }
__global__ __launch_bounds__(64) void edt_line_kernel(const int* __restrict__ g, int* __restrict__ out, long inner, long outer_stride,
                                                     int m, long es) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= inner) return;
  const long base = (long)blockIdx.y * outer_stride + i;
  g += base;
  out += base;
  int q = -1, s = 0, t = 0, gs = 0;  // top of the stack, kept in registers
  for (int u = 0; u < m; ++u) {
    const int gu = g[u * es];
    if (gu == EDT_INF) continue;
    while (q >= 0 && edt_f(t, s, gs) > edt_f(t, u, gu)) {
      if (--q >= 0) {
        const unsigned e = (unsigned)out[q * es];
        s = (int)(e & 0xffffu), t = (int)(e >> 16), gs = g[s * es];
      }
    }
    if (q < 0) {
      q = 0, s = u, t = 0, gs = gu;
      out[0] = u;
    } else {
      // Sep(s, u) = floor((u^2 - s^2 + g(u) - g(s)) / (2 (u - s))); the numerator is >= 2 (u - s) t >= 0 here
      const long long num = (long long)u * u - (long long)s * s + gu - gs;
      const int w = 1 + (int)(num / (2 * (u - s)));
      if (w < m) {
        ++q, s = u, t = w, gs = gu;
        out[q * es] = (int)((unsigned)s | ((unsigned)t << 16));
      }
    }
  }
  if (q < 0) {
    for (int u = 0; u < m; ++u) out[u * es] = EDT_INF;
    return;
  }
  for (int u = m - 1; u >= 0; --u) {
    const bool pop = (u == t);
    int ns = s, nt = t, ngs = gs;
    if (pop && q > 0) {
      const unsigned e = (unsigned)out[(q - 1) * es];
      ns = (int)(e & 0xffffu), nt = (int)(e >> 16), ngs = g[ns * es];
    }
    out[u * es] = edt_f(u, s, gs);
    if (pop) --q, s = ns, t = nt, gs = ngs;
  }
}

// ---- y / z pass with a voxel spacing ------------------------------------------------------------------------------------------
// out[u] = min over j with g[j] finite of g[j] + w2 (u - j)^2 in fp64, w2 = the squared spacing along the line: the kernel above
// with the same lines, the same access pattern and the same two scans.  G = int: g is the x pass's integer dx^2, scaled by
// `gscale` (the squared x spacing) on load, EDT_INF read as +inf (the y pass); G = double: g as it is (the z pass).  A site without
// a finite g is skipped, so no infinity enters the arithmetic; a line without a site comes out +inf.
// The stack lives in the line's own 8-byte slots of `out`, as in the integer kernel: s in the low and t in the high 32 bits of the
// slot (a bit pattern with a zero exponent, only ever copied), no separate workspace.  "Entry q sits at slot q <= t[q] <= u" holds
// whatever the rounding does, because t is forced to grow strictly from one entry to the next: Sep is floor(num / den) in fp64,
// which rounding can put one below the t of the entry under it, and the new entry then starts at t + 1.  Such a tie is between two
// sites whose values at that position agree to rounding.  Products and sums are exact for dyadic spacings at these sizes.
#ifdef __clang__
#pragma clang fp contract(off)  // w2 * d^2 + g as a product and a sum, on the device as on the host checker
#endif
#define EDT_DINF __builtin_huge_val()
template <typename G>
__device__ __forceinline__ double edtw_ld(const G* __restrict__ g, long k, double gscale);
template <>
__device__ __forceinline__ double edtw_ld<int>(const int* __restrict__ g, long k, double gscale) {
  const int v = g[k];
  return v == EDT_INF ? EDT_DINF : gscale * (double)v;
}
template <>
__device__ __forceinline__ double edtw_ld<double>(const double* __restrict__ g, long k, double) {
  return g[k];
}
__device__ __forceinline__ double edtw_f(int u, int s, double gs, double w2) {
  const double d = (double)(u - s);
  return w2 * (d * d) + gs;
}
__device__ __forceinline__ void edtw_put(double* slot, int s, int t) {
  const unsigned long long e = (unsigned long long)(unsigned)s | ((unsigned long long)(unsigned)t << 32);
  double d;
  __builtin_memcpy(&d, &e, 8);
  *slot = d;
}
__device__ __forceinline__ void edtw_get(const double* slot, int& s, int& t) {
  const double d = *slot;
  unsigned long long e;
  __builtin_memcpy(&e, &d, 8);
  s = (int)(unsigned)(e & 0xffffffffull), t = (int)(unsigned)(e >> 32);
}
template <typename G>
__global__ __launch_bounds__(64) void edt_line_w_kernel(const G* __restrict__ g, double* __restrict__ out, long inner,
                                                       long outer_stride, int m, long es, double w2, double gscale) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= inner) return;
  const long base = (long)blockIdx.y * outer_stride + i;
  g += base;
  out += base;
  int q = -1, s = 0, t = 0;  // top of the stack, kept in registers
  double gs = 0.0;
  for (int u = 0; u < m; ++u) {
    const double gu = edtw_ld<G>(g, u * es, gscale);
    if (gu == EDT_DINF) continue;
    while (q >= 0 && edtw_f(t, s, gs, w2) > edtw_f(t, u, gu, w2)) {
      if (--q >= 0) {
        edtw_get(out + q * es, s, t);
        gs = edtw_ld<G>(g, s * es, gscale);
      }
    }
    if (q < 0) {
      q = 0, s = u, t = 0, gs = gu;
      edtw_put(out, u, 0);
    } else {
      // Sep(s, u) = floor((w2 (u^2 - s^2) + g(u) - g(s)) / (2 w2 (u - s)))
      const double num = w2 * (double)((long long)u * u - (long long)s * s) + (gu - gs);
      const double sep = floor(num / (2.0 * w2 * (double)(u - s)));
      if (sep < (double)(m - 1)) {  // (so the conversion below is in range)
        const int w = sep < (double)t ? t + 1 : 1 + (int)sep;
        if (w < m) {
          ++q, s = u, t = w, gs = gu;
          edtw_put(out + q * es, s, t);
        }
      }
    }
  }
  if (q < 0) {
    for (int u = 0; u < m; ++u) out[u * es] = EDT_DINF;
    return;
  }
  for (int u = m - 1; u >= 0; --u) {
    const bool pop = (u == t);
    int ns = s, nt = t;
    double ngs = gs;
    if (pop && q > 0) {
      edtw_get(out + (q - 1) * es, ns, nt);
      ngs = edtw_ld<G>(g, ns * es, gscale);
    }
    out[u * es] = edtw_f(u, s, gs, w2);
    if (pop) --q, s = ns, t = nt, gs = ngs;
  }
}

// ---- ordered compaction of a border ------------------------------------------------------------------------------------------
// A workgroup owns CP_CHUNK consecutive voxels.  border_count: how many of them carry `match`.  border_gather: with the exclusive
// prefix sum of those counts (taken between the two launches), writes for every matching voxel, in C order, either its (z, y, x)
// or src[voxel] (T = int; T = double: src[voxel] only).  Thread t ranks the 16 voxels [16 t, 16 t + 16) of the chunk after a block
// scan of the per-thread counts.
#define CP_CHUNK 4096
__global__ __launch_bounds__(256) void border_count_kernel(const unsigned char* __restrict__ bl, int match, long n,
                                                          int* __restrict__ counts) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * CP_CHUNK;
  int c = 0;
  for (int k = threadIdx.x; k < CP_CHUNK; k += 256)
    if (base + k < n && bl[base + k] == (unsigned char)match) ++c;
  if (c) atomicAdd(&total, c);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
template <typename T>
__global__ __launch_bounds__(256) void border_gather_kernel(const unsigned char* __restrict__ bl, int match, long n, int H, int W,
                                                           const int* __restrict__ offs, const T* __restrict__ src,
                                                           T* __restrict__ out) {
  __shared__ unsigned char fl[CP_CHUNK];
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * CP_CHUNK;
  for (int k = tid; k < CP_CHUNK; k += 256) fl[k] = (base + k < n && bl[base + k] == (unsigned char)match) ? 1 : 0;
  __syncthreads();
  int c = 0;
  for (int j = 0; j < 16; ++j) c += fl[tid * 16 + j];
  cnt[tid] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = tid >= off ? cnt[tid - off] : 0;
    __syncthreads();
    cnt[tid] += v;
    __syncthreads();
  }
  long pos = (long)offs[blockIdx.x] + cnt[tid] - c;
  if (!c) return;
  for (int j = 0; j < 16; ++j) {
    if (!fl[tid * 16 + j]) continue;
    const long i = base + tid * 16 + j;
    if (src) {
      out[pos] = src[i];
    } else {
      const long t = i / W;
      out[pos * 3] = (T)(t / H), out[pos * 3 + 1] = (T)(t % H), out[pos * 3 + 2] = (T)(i % W);
    }
    ++pos;
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
extern "C" int cenet_label_borders_f32(const float* pred, const float* gt, unsigned char* border_pred, unsigned char* border_gt,
                                       int* table, int K, int D, int H, int W, int zfaces, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || K < 2 || K > LB_MAXK) return CENET_EINVAL;
  const long n = (long)D * H * W;
  if (n >= EDT_INF) return CENET_EINVAL;  // the counts are int32
  unsigned blocks = edt_cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  CENET_LAUNCH(label_borders_kernel, dim3(blocks), dim3(256), stream, pred, gt, border_pred, border_gt, table, K, D, H, W, zfaces);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// The in-plane transform of `planes` planes of H x W: the x pass over planes * H rows into xd, then the line pass along y with
// blockIdx.y = plane into out.  A volume is this plus the z pass; a stack of unrelated planes is this alone.  planes <= 65535.
static int edt_planes_launch(const unsigned char* feat, int match, int* xd, int* out, int planes, int H, int W, hipStream_t stream) {
  const long rows = (long)planes * H, plane = (long)H * W;
  CENET_LAUNCH(edt_x_kernel, dim3(edt_cdiv(rows, EX_ROWS)), dim3(256), stream, feat, match, xd, rows, W);
  CENET_CHECK_LAUNCH();
  CENET_LAUNCH(edt_line_kernel, dim3(edt_cdiv(W, 64), (unsigned)planes), dim3(64), stream, (const int*)xd, out, (long)W, plane, H,
               (long)W);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_edt_sq_u8(const unsigned char* feat, int match, int* tmp, int* d2, int D, int H, int W, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || match > 255) return CENET_EINVAL;
  if ((long)D * D + (long)H * H + (long)W * W >= (1L << 31)) return CENET_EINVAL;  // (so every side is < 65536 as well)
  const long rows = (long)D * H, plane = (long)H * W;
  if (plane * D >= (1L << 40) || edt_cdiv(rows, EX_ROWS) == 0) return CENET_EINVAL;
  const int rc = edt_planes_launch(feat, match, d2, tmp, D, H, W, stream);
  if (rc != CENET_OK) return rc;
  CENET_LAUNCH(edt_line_kernel, dim3(edt_cdiv(plane, 64), 1u), dim3(64), stream, (const int*)tmp, d2, plane, 0L, D, plane);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// The transform with a voxel spacing: the integer x pass, then the weighted line pass along y (which scales the x result by sx^2 as
// it loads it) and along z; with sy == sx the integer y pass as well, and one weighted pass.  xd: D*H*W ints, tmp and d2: D*H*W
// doubles each.
static inline bool edt_spacing_ok(double s) {
  const double w2 = s * s;
  return s > 0.0 && w2 > 0.0 && w2 - w2 == 0.0;  // positive and finite, and so is its square
}
extern "C" int cenet_edt_sq_spaced_u8(const unsigned char* feat, int match, int* xd, double* tmp, double* d2, int D, int H, int W,
                                      double sz, double sy, double sx, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || match > 255) return CENET_EINVAL;
  if (!edt_spacing_ok(sz) || !edt_spacing_ok(sy) || !edt_spacing_ok(sx)) return CENET_EINVAL;
  if ((long)D * D + (long)H * H + (long)W * W >= (1L << 31)) return CENET_EINVAL;  // the x pass is int32, the stack packs sides
  const long rows = (long)D * H, plane = (long)H * W;
  if (plane * D >= (1L << 40) || edt_cdiv(rows, EX_ROWS) == 0) return CENET_EINVAL;
  if (sy == sx) {
    // the in-plane spacing is isotropic (every clinical volume): the integer passes give dy^2 + dx^2 exactly, into the first half of
    // tmp, and only the z pass is weighted: sz^2 dz^2 + sx^2 (dy^2 + dx^2), the in-plane scale applied as the z pass loads
    int* yd = (int*)tmp;
    const int rc = edt_planes_launch(feat, match, xd, yd, D, H, W, stream);
    if (rc != CENET_OK) return rc;
    CENET_LAUNCH(edt_line_w_kernel<int>, dim3(edt_cdiv(plane, 64), 1u), dim3(64), stream, (const int*)yd, d2, plane, 0L, D, plane,
                 sz * sz, sx * sx);
    CENET_CHECK_LAUNCH();
    return CENET_OK;
  }
  CENET_LAUNCH(edt_x_kernel, dim3(edt_cdiv(rows, EX_ROWS)), dim3(256), stream, feat, match, xd, rows, W);
  CENET_CHECK_LAUNCH();
  CENET_LAUNCH(edt_line_w_kernel<int>, dim3(edt_cdiv(W, 64), (unsigned)D), dim3(64), stream, (const int*)xd, tmp, (long)W, plane, H,
               (long)W, sy * sy, sx * sx);
  CENET_CHECK_LAUNCH();
  CENET_LAUNCH(edt_line_w_kernel<double>, dim3(edt_cdiv(plane, 64), 1u), dim3(64), stream, (const double*)tmp, d2, plane, 0L, D,
               plane, sz * sz, 1.0);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// ---- boundary-distance maps --------------------------------------------------------------------------------------------------
// Plane (b, c), c = 1 .. K-1, has the mask M = {label == c} or {softmax_c > 1/2}.  The map is the squared distance to the nearest
// pixel of the other kind: the transform with M as features (non-zero outside M) plus the one with the complement as features
// (non-zero inside M).  Both run as ONE stack of 2 P planes, P = B (K-1): planes [0, P) hold M, planes [P, 2P) its complement.
// A plane whose M is empty or full has one half without a feature, INT_MAX everywhere, and the other half 0 everywhere:
// INT_MAX counts as 0 in the sum, so such a plane comes out 0 — decided per pixel on the device, nothing is read back.
// ws (ints): xd [2 P H W], yd [2 P H W], then the feature bytes [2 P H W].
#define DM_MAXK 16
static inline bool dm_shape_ok(int B, int K, int H, int W) {
  return B > 0 && K >= 2 && K <= DM_MAXK && H >= 1 && W >= 1 && 2L * B * (K - 1) <= 65535 &&
         (long)H * H + (long)W * W < (1L << 31);
}
extern "C" long cenet_dist_maps_ws_ints(int B, int K, int H, int W) {
  if (!dm_shape_ok(B, K, H, W)) return 0;
  const long n2 = 2L * B * (K - 1) * H * W;
  return 2 * n2 + (n2 + 3) / 4;
}

// one thread per pixel of an image: its K - 1 bytes of M and of the complement, consecutive lanes on consecutive pixels
__global__ __launch_bounds__(256) void dm_labels_kernel(const float* __restrict__ labels, unsigned char* __restrict__ feat, int K,
                                                        long HW, long half) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const long b = blockIdx.y;
  const float t = labels[b * HW + p];
  unsigned char* f = feat + b * (K - 1) * HW + p;
  for (int c = 1; c < K; ++c) {
    const unsigned char m = t == (float)c;
    f[(c - 1) * HW] = m;
    f[half + (c - 1) * HW] = m ^ 1;
  }
}
// softmax_c > 1/2  <=>  exp(v_c - max) > sum / 2, in fp32 from the logits; no probability is stored
template <typename T, int KM>
__global__ __launch_bounds__(256) void dm_logits_kernel(const T* __restrict__ logits, unsigned char* __restrict__ feat, int K,
                                                        long HW, long half) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const long b = blockIdx.y;
  const T* lg = logits + b * K * HW + p;
  float v[KM];
  float mx = -3.4e38f;
#pragma unroll
  for (int c = 0; c < KM; ++c)
    if (c < K) {
      v[c] = ldf(lg + c * HW);
      mx = fmaxf(mx, v[c]);
    }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < KM; ++c)
    if (c < K) {
      v[c] = expf(v[c] - mx);
      s += v[c];
    }
  unsigned char* f = feat + b * (K - 1) * HW + p;
#pragma unroll
  for (int c = 1; c < KM; ++c)
    if (c < K) {
      const unsigned char m = v[c] > 0.5f * s;
      f[(c - 1) * HW] = m;
      f[half + (c - 1) * HW] = m ^ 1;
    }
}
__global__ __launch_bounds__(256) void dm_merge_kernel(const int* __restrict__ yd, int* __restrict__ d2, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int a = yd[i], b = yd[n + i];
    d2[i] = (a == EDT_INF ? 0 : a) + (b == EDT_INF ? 0 : b);
  }
}

// the stack's transform and the sum of its halves, after one of the two kernels above has filled the feature bytes
static int dm_finish(int* ws, int* d2, int B, int K, int H, int W, hipStream_t stream) {
  const int P = B * (K - 1);
  const long n = (long)P * H * W;
  const int rc = edt_planes_launch((const unsigned char*)(ws + 4 * n), 1, ws, ws + 2 * n, 2 * P, H, W, stream);
  if (rc != CENET_OK) return rc;
  long blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  CENET_LAUNCH(dm_merge_kernel, dim3((unsigned)blocks), dim3(256), stream, (const int*)(ws + 2 * n), d2, n);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
static inline bool dm_args_ok(const void* src, int* ws, long ws_ints, int* d2, int B, int K, int H, int W) {
  return dm_shape_ok(B, K, H, W) && src && ws && d2 && ws_ints >= cenet_dist_maps_ws_ints(B, K, H, W) &&
         ((long)H * W + 255) / 256 <= 0x7fffffffL;
}

extern "C" int cenet_dist_maps_labels_f32(const float* labels, int* ws, long ws_ints, int* d2, int B, int K, int H, int W,
                                          hipStream_t stream) {
  if (!dm_args_ok(labels, ws, ws_ints, d2, B, K, H, W)) return CENET_EINVAL;
  const long HW = (long)H * W, n = (long)B * (K - 1) * HW;
  CENET_LAUNCH(dm_labels_kernel, dim3(edt_cdiv(HW, 256), (unsigned)B), dim3(256), stream, labels, (unsigned char*)(ws + 4 * n), K,
               HW, n);
  CENET_CHECK_LAUNCH();
  return dm_finish(ws, d2, B, K, H, W, stream);
}

template <typename T>
static int dist_maps_logits_impl(const T* logits, int* ws, long ws_ints, int* d2, int B, int K, int H, int W, hipStream_t stream) {
  if (!dm_args_ok(logits, ws, ws_ints, d2, B, K, H, W)) return CENET_EINVAL;
  const long HW = (long)H * W, n = (long)B * (K - 1) * HW;
  const dim3 grid(edt_cdiv(HW, 256), (unsigned)B);
  unsigned char* feat = (unsigned char*)(ws + 4 * n);
  if (K <= 4) CENET_LAUNCH((dm_logits_kernel<T, 4>), grid, dim3(256), stream, logits, feat, K, HW, n);
  else if (K <= 9) CENET_LAUNCH((dm_logits_kernel<T, 9>), grid, dim3(256), stream, logits, feat, K, HW, n);
  else CENET_LAUNCH((dm_logits_kernel<T, DM_MAXK>), grid, dim3(256), stream, logits, feat, K, HW, n);
  CENET_CHECK_LAUNCH();
  return dm_finish(ws, d2, B, K, H, W, stream);
}
CENET_TWIN(dist_maps_logits, (const T* logits, int* ws, long ws_ints, int* d2, int B, int K, int H, int W, hipStream_t stream),
           (logits, ws, ws_ints, d2, B, K, H, W, stream))

extern "C" int cenet_border_count_u8(const unsigned char* bl, int match, long n, int* counts, hipStream_t stream) {
  if (n <= 0 || match < 0 || match > 255) return CENET_EINVAL;
  CENET_LAUNCH(border_count_kernel, dim3(edt_cdiv(n, CP_CHUNK)), dim3(256), stream, bl, match, n, counts);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_border_gather_i32(const unsigned char* bl, int match, int D, int H, int W, const int* offs, const int* src,
                                       int* out, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || match < 0 || match > 255) return CENET_EINVAL;
  const long n = (long)D * H * W;
  CENET_LAUNCH(border_gather_kernel<int>, dim3(edt_cdiv(n, CP_CHUNK)), dim3(256), stream, bl, match, n, H, W, offs, src, out);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_border_gather_f64(const unsigned char* bl, int match, int D, int H, int W, const int* offs, const double* src,
                                       double* out, hipStream_t stream) {
  if (D <= 0 || H <= 0 || W <= 0 || match < 0 || match > 255 || !src) return CENET_EINVAL;
  const long n = (long)D * H * W;
  CENET_LAUNCH(border_gather_kernel<double>, dim3(edt_cdiv(n, CP_CHUNK)), dim3(256), stream, bl, match, n, H, W, offs, src, out);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
