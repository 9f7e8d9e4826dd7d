// ccl.hip — connected components of a label volume and the keep-largest filter (evaluate.keep_largest_component).
// Two voxels are linked when they are neighbours (6 / 18 / 26 neighbourhood, or its in-plane part with zlinks = 0) AND carry the
// same class, so one pass labels every class.  Union-find with the parent array in global memory: parent[v] <= v always, values
// only ever decrease, roots are joined with an integer atomicMin — the root of a component ends up as its smallest linear index,
// whatever the schedule.  No workgroup waits for another one; the only grid-wide ordering is the kernel boundary.  A find that
// reads an outdated parent still reads an ancestor of the same set, and a union whose atomicMin did not hit a root goes on from
// the value it displaced, so outdated reads cost steps, never a link.  Integer arithmetic only.
//   ccl_init_kernel      parent[v] = first voxel of v's run of equal class along x inside its tile of 256 voxels (-1: background)
//   ccl_link_kernel      unions across tile edges and with the neighbours that come before v in raster order; a union that the
//                        unions of the voxel to the left already imply is skipped, so the interior of a blob issues no atomic
//   ccl_flatten_kernel   parent[v] = find(v)
//   ccl_count_kernel     sizes[root] += length of each run of equal roots inside a tile, gathered per workgroup in LDS
//   ccl_select_kernel    per class (or slice and class): the largest size, then the smallest root among the components that have it
//   ccl_filter_kernel    out[v] = class of v where its component is kept, else 0; per class components / kept / removed
#include "common.h"
#include "../../include/cenet_hip.h"

#define CCL_TILE 256
#define CCL_MAXK 64  // as cenet_label_borders_f32
#define CCL_INT_MAX 0x7fffffff
#define CCL_CHUNK 16384  // voxels per workgroup of the size, selection and filter kernels

#ifdef CENET_HOSTSIM_BUILD  // (the host checker runs one thread at a time)
static inline int atomicCAS(int* p, int expect, int val) {
  const int o = *p;
  if (o == expect) *p = val;
  return o;
}
#endif

static inline unsigned ccl_blocks(long n) { return (unsigned)((n + CCL_TILE - 1) / CCL_TILE); }
static inline unsigned ccl_chunks(long n) { return (unsigned)((n + CCL_CHUNK - 1) / CCL_CHUNK); }

// the rule of cenet_label_borders_f32 (edt.hip): anything that is not an integer in [1, K) is background
__device__ __forceinline__ int ccl_class(float v, int K) {
  const int c = (int)v;
  return (v >= 1.f && v < (float)K && (float)c == v) ? c : 0;
}

// h[tid] = the largest t <= tid with first(t): the head of tid's run.  Inclusive max-scan over the tile; every thread calls it.
__device__ __forceinline__ int ccl_run_head(int* h, int tid, bool first) {
  h[tid] = first ? tid : 0;
  __syncthreads();
  for (int off = 1; off < CCL_TILE; off <<= 1) {
    const int t = tid >= off ? h[tid - off] : 0;
    __syncthreads();
    if (t > h[tid]) h[tid] = t;
    __syncthreads();
  }
  return h[tid];
}

__global__ __launch_bounds__(CCL_TILE) void ccl_init_kernel(const float* __restrict__ labels, int* __restrict__ parent, long n,
                                                           int K, int W) {
  __shared__ int cls[CCL_TILE];
  __shared__ int h[CCL_TILE];
  const int tid = threadIdx.x;
  const long v = (long)blockIdx.x * CCL_TILE + tid;
  const int c = v < n ? ccl_class(labels[v], K) : 0;
  cls[tid] = c;
  __syncthreads();
  const bool first = tid == 0 || v % W == 0 || cls[tid - 1] != c;
  const int head = ccl_run_head(h, tid, first);
  if (v < n) parent[v] = c ? (int)(v - tid) + head : -1;
}

__device__ __forceinline__ int ccl_find(const int* parent, int x) {
  int p;
  while ((p = parent[x]) != x) x = p;
  return x;
}
// every pass either ends or replaces the larger of the two by a smaller voxel of the same set
__device__ __forceinline__ void ccl_union(int* parent, int a, int b) {
  for (;;) {
    a = ccl_find(parent, a);
    b = ccl_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(&parent[b], a);
    if (old == b) return;  // b was a root and now hangs under a
    b = old;               // b had been linked meanwhile: a still has to meet what it was linked to
  }
}

// The neighbours (dz, dy, dx) that precede v in raster order, (0, 0, -1) aside: init linked that one inside the tile, thread 0
// links it across the tile edge.  Same class <=> same float, as v's own value is an integer in [1, K).
// Skipped, with L = v - 1 of v's class:  (a) dx != 0 and v + (dz, dy, 0) has the class: v meets u through that neighbour and an x
// link;  (b) u - 1 has the class as well: L makes (or skips, by the same rules) the union with u - 1, and x links close the square.
__global__ __launch_bounds__(CCL_TILE) void ccl_link_kernel(const float* __restrict__ labels, int* parent, long n, int K, int D,
                                                           int H, int W, int conn, int zlinks) {
  const long v = (long)blockIdx.x * CCL_TILE + threadIdx.x;
  if (v >= n) return;
  const float lv = labels[v];
  if (!ccl_class(lv, K)) return;
  const long plane = (long)H * W;
  const int x = (int)(v % W);
  const long t = v / W;
  const int y = (int)(t % H), z = (int)(t / H);
  (void)D;
  const bool left = x > 0 && labels[v - 1] == lv;
  if (left && threadIdx.x == 0) ccl_union(parent, (int)v, (int)v - 1);
  for (int dz = zlinks ? -1 : 0; dz <= 0; ++dz) {
    if (z + dz < 0) continue;
    for (int dy = -1; dy <= (dz ? 1 : -1); ++dy) {
      if (y + dy < 0 || y + dy >= H) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if ((dz != 0) + (dy != 0) + (dx != 0) > conn || x + dx < 0 || x + dx >= W) continue;
        const long u = v + dz * plane + (long)dy * W + dx;
        if (labels[u] != lv) continue;
        if (dx != 0 && labels[u - dx] == lv) continue;
        if (left && x + dx > 0 && labels[u - 1] == lv) continue;
        ccl_union(parent, (int)v, (int)u);
      }
    }
  }
}

__global__ __launch_bounds__(CCL_TILE) void ccl_flatten_kernel(int* parent, long n) {
  const long v = (long)blockIdx.x * CCL_TILE + threadIdx.x;
  if (v >= n) return;
  const int p = parent[v];
  if (p < 0) return;
  const int r = ccl_find(parent, p);
  if (r != p) parent[v] = r;  // (a reader that still sees p sees an ancestor)
}

__global__ __launch_bounds__(CCL_TILE) void ccl_fill_kernel(int* __restrict__ p, long n, int val) {
  const long i = (long)blockIdx.x * CCL_TILE + threadIdx.x;
  if (i < n) p[i] = val;
}

// A workgroup of the three kernels below walks CCL_CHUNK consecutive voxels tile by tile and gathers what it adds to global memory in
// LDS first: a giant component, or one class's slot, would otherwise take an atomic from every tile of the volume on one address.
//
// sizes: one add per run of equal roots inside a tile, into a direct-mapped LDS table keyed by the root (a root that finds its
// slot taken by another one adds to global memory directly); the table is flushed once per chunk.
__global__ __launch_bounds__(CCL_TILE) void ccl_count_kernel(const int* __restrict__ roots, int* __restrict__ sizes, long n) {
  __shared__ int key[CCL_TILE];
  __shared__ int h[CCL_TILE];
  __shared__ int hk[CCL_TILE];
  __shared__ int hc[CCL_TILE];
  const int tid = threadIdx.x;
  hk[tid] = -1, hc[tid] = 0;
  for (int t = 0; t < CCL_CHUNK / CCL_TILE; ++t) {
    const long base = (long)blockIdx.x * CCL_CHUNK + (long)t * CCL_TILE;
    if (base >= n) break;
    const int r = base + tid < n ? roots[base + tid] : -1;
    __syncthreads();  // (the previous tile's readers of key[]; the first pass: hk / hc)
    key[tid] = r;
    __syncthreads();
    const int head = ccl_run_head(h, tid, tid == 0 || key[tid - 1] != r);
    if (r >= 0 && (tid == CCL_TILE - 1 || key[tid + 1] != r)) {
      const int len = tid - head + 1, slot = (int)(((unsigned)r * 2654435761u) >> 24);
      const int old = atomicCAS(&hk[slot], -1, r);
      if (old == -1 || old == r)
        atomicAdd(&hc[slot], len);
      else
        atomicAdd(&sizes[r], len);
    }
  }
  __syncthreads();
  if (hk[tid] >= 0) atomicAdd(&sizes[hk[tid]], hc[tid]);
}

// ws[0, slots): minus the largest size per slot, ws[slots, 2 slots): the smallest root of that size; slot = slice * K + class
// (slice = 0 with z links).  pass 0 takes the sizes and counts the components, pass 1 the roots.  Only roots act.  best[] gathers
// the slots of slice `zcur` and is flushed when the walk enters another slice; a root of a tile's other slice (planes that are no
// multiple of a tile) goes to global memory directly.
__global__ __launch_bounds__(CCL_TILE) void ccl_select_kernel(const float* __restrict__ labels, const int* __restrict__ roots,
                                                             const int* __restrict__ sizes, int* ws, int* __restrict__ table,
                                                             long n, int K, long plane, int zlinks, int slots, int pass) {
  __shared__ int best[CCL_MAXK];
  __shared__ int ncomp[CCL_MAXK];
  const int tid = threadIdx.x, none = pass ? CCL_INT_MAX : 0;
  int zcur = -1;
  if (tid < CCL_MAXK) best[tid] = none, ncomp[tid] = 0;
  for (int t = 0; t < CCL_CHUNK / CCL_TILE; ++t) {
    const long base = (long)blockIdx.x * CCL_CHUNK + (long)t * CCL_TILE, v = base + tid;
    if (base >= n) break;
    const int z0 = zlinks ? 0 : (int)(base / plane);
    if (z0 != zcur) {  // (the same for every thread)
      __syncthreads();
      if (tid < K && best[tid] != none) atomicMin(&ws[pass * slots + zcur * K + tid], best[tid]), best[tid] = none;
      __syncthreads();
      zcur = z0;
    }
    if (v < n && roots[v] == (int)v) {
      const int c = ccl_class(labels[v], K), zs = zlinks ? 0 : (int)(v / plane);
      const int s = -sizes[v];
      if (!pass) atomicAdd(&ncomp[c], 1);
      if (!pass || s == ws[zs * K + c]) {
        const int val = pass ? (int)v : s;
        if (zs == zcur)
          atomicMin(&best[c], val);
        else
          atomicMin(&ws[pass * slots + zs * K + c], val);
      }
    }
  }
  __syncthreads();
  if (tid < K) {
    if (best[tid] != none) atomicMin(&ws[pass * slots + zcur * K + tid], best[tid]);
    if (ncomp[tid]) atomicAdd(&table[3 * tid], ncomp[tid]);
  }
}

__global__ __launch_bounds__(CCL_TILE) void ccl_keep_init_kernel(int* __restrict__ ws, int slots, int* __restrict__ table, int K) {
  const int i = blockIdx.x * CCL_TILE + threadIdx.x;
  if (i < 2 * slots) ws[i] = i < slots ? 0 : CCL_INT_MAX;
  if (i < 3 * K) table[i] = 0;
}

// the kept / removed voxel counts are added up at the roots, from the components' sizes: no atomic per voxel
__global__ __launch_bounds__(CCL_TILE) void ccl_filter_kernel(const float* __restrict__ labels, const int* __restrict__ roots,
                                                             const int* __restrict__ sizes, const int* __restrict__ ws,
                                                             float* __restrict__ out, int* __restrict__ table, long n, int K,
                                                             long plane, int zlinks, int slots, int min_size) {
  __shared__ int acc[2 * CCL_MAXK];  // kept, removed
  const int tid = threadIdx.x;
  if (tid < 2 * CCL_MAXK) acc[tid] = 0;
  __syncthreads();
  for (int t = 0; t < CCL_CHUNK / CCL_TILE; ++t) {
    const long v = (long)blockIdx.x * CCL_CHUNK + (long)t * CCL_TILE + tid;
    if (v >= n) break;
    const int c = ccl_class(labels[v], K);
    bool keep = false;
    if (c) {
      const int r = roots[v];
      keep = r == ws[slots + (zlinks ? 0 : (int)(v / plane)) * K + c] || (min_size > 0 && sizes[r] >= min_size);
      if (r == (int)v) atomicAdd(&acc[keep ? c : CCL_MAXK + c], sizes[v]);
    }
    out[v] = keep ? (float)c : 0.f;
  }
  __syncthreads();
  if (tid < K) {
    if (acc[tid]) atomicAdd(&table[3 * tid + 1], acc[tid]);
    if (acc[CCL_MAXK + tid]) atomicAdd(&table[3 * tid + 2], acc[CCL_MAXK + tid]);
  }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------
static inline bool ccl_shape_ok(int K, int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && K >= 2 && K <= CCL_MAXK && (long)D * H * W <= CCL_INT_MAX;
}

extern "C" int cenet_ccl_label_f32(const float* labels, int* roots, int K, int D, int H, int W, int connectivity, int zlinks,
                                   hipStream_t stream) {
  if (!ccl_shape_ok(K, D, H, W) || connectivity < 1 || connectivity > 3 || (!zlinks && connectivity == 3)) return CENET_EINVAL;
  const long n = (long)D * H * W;
  const dim3 grid(ccl_blocks(n)), block(CCL_TILE);
  CENET_LAUNCH(ccl_init_kernel, grid, block, stream, labels, roots, n, K, W);
  CENET_CHECK_LAUNCH();
  CENET_LAUNCH(ccl_link_kernel, grid, block, stream, labels, roots, n, K, D, H, W, connectivity, zlinks ? 1 : 0);
  CENET_CHECK_LAUNCH();
  CENET_LAUNCH(ccl_flatten_kernel, grid, block, stream, roots, n);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_ccl_sizes_i32(const int* roots, int* sizes, long n, hipStream_t stream) {
  if (n <= 0 || n > CCL_INT_MAX) return CENET_EINVAL;
  const dim3 grid(ccl_blocks(n)), block(CCL_TILE);
  CENET_LAUNCH(ccl_fill_kernel, grid, block, stream, sizes, n, 0);
  CENET_CHECK_LAUNCH();
  CENET_LAUNCH(ccl_count_kernel, dim3(ccl_chunks(n)), block, stream, roots, sizes, n);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" long cenet_ccl_ws_ints(int K, int D, int zlinks) {
  if (K < 2 || K > CCL_MAXK || D <= 0) return 0;
  return 2L * K * (zlinks ? 1 : D);
}

extern "C" int cenet_ccl_keep_f32(const float* labels, const int* roots, const int* sizes, int* ws, long ws_ints, float* out,
                                  int* table, int K, int D, int H, int W, int zlinks, int min_size, hipStream_t stream) {
  if (!ccl_shape_ok(K, D, H, W) || min_size < 0 || out == labels) return CENET_EINVAL;
  const long n = (long)D * H * W, plane = (long)H * W, need = cenet_ccl_ws_ints(K, D, zlinks);
  if (ws_ints < need || need / 2 > CCL_INT_MAX / 2) return CENET_EINVAL;
  const int slots = (int)(need / 2), zl = zlinks ? 1 : 0;
  const dim3 grid(ccl_chunks(n)), block(CCL_TILE);
  CENET_LAUNCH(ccl_keep_init_kernel, dim3(ccl_blocks(need > 3 * K ? need : 3 * K)), block, stream, ws, slots, table, K);
  CENET_CHECK_LAUNCH();
  for (int pass = 0; pass < 2; ++pass) {
    CENET_LAUNCH(ccl_select_kernel, grid, block, stream, labels, roots, sizes, ws, table, n, K, plane, zl, slots, pass);
    CENET_CHECK_LAUNCH();
  }
  CENET_LAUNCH(ccl_filter_kernel, grid, block, stream, labels, roots, sizes, (const int*)ws, out, table, n, K, plane, zl, slots,
               min_size);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}
