// attn_diff.hip — differential attention of the DSEB skip blocks on bf16 tensors (throughput mode), forward and backward.
//
// Reference: multihead_diffattn.py:83-109 — q, k [B, N, 2H, hd], v [B, N, H, 2hd]; softmax head 2h+s (s = 0, 1) attends with
// q_{2h+s}, k_{2h+s} over the SHARED value head h:  U[b, 2h+s] = softmax(q k^T / sqrt(hd)) v_h   ([B, 2H, N, 2hd]).
// DSEB-56^2 (ACDC: N = 3136, hd = 16, 8 softmax heads, B = 32) is the largest attention problem of the step: 2.5 G scores
// per pass, 96 MFMA FLOP per score — the exponentials and the softmax algebra (VALU), not the matrix cores, bound it.
//
// Design (wave64, v_mfma_f32_32x32x16_bf16; C/D: lane = column, 16 registers = rows (r&3) + 8(r>>2) + 4(lane>>5)):
//   * a wave owns 32-row tiles of the side that stays fixed (queries in fwd / dQ, keys in dK/dV) for BOTH softmax heads of
//     a pair; the four waves of a workgroup share the streamed side: each 32-row tile is fetched once per workgroup with
//     16-byte loads (register prefetch one tile ahead: the loads of tile t + 1 are issued in front of the body of tile t and
//     waited for behind it, tools/isa_loops.py shows the order per instance) into a double-buffered ROW-MAJOR bf16 image in
//     LDS, one barrier per tile;
//   * scores are computed transposed w.r.t. the fixed side (S^T = K Q^T in fwd / dQ, S = Q K^T in dK/dV), so the fixed index is
//     the MFMA column = the lane: softmax state (max, sum, lse, delta) is one scalar per lane, a row reduction is 15 in-lane
//     ops + one exchange with lane ^ 32, and the probability registers ARE the B operand of the next product (k-step s takes
//     registers 8s..8s+7 = rows 16s + 8(j>>2) + 4(lane>>5) + (j&3));
//   * the A operand of that next product runs along the token index of the streamed tile: it is read from the same row-major
//     image with the transposing LDS read (ds_read_b64_tr_b16: a 16-lane group gets a 4-row x 16-column block column-major),
//     two per fragment — no transposed copy in HBM, no 2-byte scatter into LDS;
//   * hd = 16 is exactly one K = 16 step of the 32x32x16 MFMA (no zero padding of the contraction as with K = 32 tiles);
//     hd = 8 runs zero-padded to 16, hd = 32 as two k-steps; value width 2hd = 32 / 64 = one / two 32-row tiles;
//   * the shared value head: both softmax heads of a pair accumulate dV in the same registers — no atomics anywhere;
//   * in dK/dV the softmax statistics belong to the ROWS (queries) of the score tile; instead of 2 x 16 loads and subtractions
//     per lane they ride in the contraction: the dQ kernel leaves lse / scale and delta split into three bf16 terms each
//     (24 significant bits) per (head, query), and one extra k-step against a constant -1 fragment gives S - lse/scale and
//     dP - delta straight out of the MFMA;
//   * base-2 exponentials with scale*log2(e) folded into one multiply per score; the running maximum of the forward pass is
//     rescaled only when some lane of the wave actually raised it (wave-uniform branch);
//   * the key loops of the forward and dQ kernels hold ONE instantiation of the tile body, the unmasked one, and run over the
//     full 32-key tiles; the masked instantiation runs once after the loop on the ragged last tile (N % 32 keys), which the
//     fetch -> stage -> barrier pipeline delivers like any other tile.  The trip count depends on N alone, so every wave of a
//     workgroup meets the same barriers whatever its q0.  With both instantiations inside the loop (`klim < 32 ? masked :
//     unmasked` per iteration) the register allocator gave the two bodies' results different registers and copied every
//     loop-carried accumulator across the join: 32-36 v_mov_b64 / v_mov_b32 per iteration and 30-70 more registers per instance
//     (hd 16: forward 168 -> 122, Non-local forward 194 -> 129; profiles/r07_attn_isa.md);
//   * the softmax denominator stays on the VALU (one v_add_f32 per score): accumulating it on the matrix pipe against an
//     all-ones A fragment costs 16 registers per head, which takes the hd-16 forward from four waves per SIMD back to three
//     and measured 7 % SLOWER.
#include "common.h"
#include "../../include/cenet_hip.h"
#include <cstdlib>

typedef bf16_t bf;
#define DA_NEG (-1.0e30f)
#define DA_LOG2E 1.4426950408889634f

#ifdef CENET_HOSTSIM_BUILD
__device__ __forceinline__ float da_exp2(float x) { return exp2f(x); }
__device__ __forceinline__ bool da_any(bool v) {
  int x = v ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o);
  return x != 0;
}
#else
__device__ __forceinline__ float da_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ bool da_any(bool v) { return __any(v); }
typedef short da_s4 __attribute__((ext_vector_type(4)));
#endif
// max of three; built with -fno-honor-nans (cenet_amd/build.py) the compiler emits v_max3_f32 without the canonicalising
// v_max it otherwise puts in front of fmaxf on MFMA results.  (NOT inline asm: hipcc pads no MFMA -> VALU wait states for
// an asm statement that reads accumulator registers, cdna_hip_programming.md §5.7 — the asm form read stale scores.)
__device__ __forceinline__ float da_max3(float a, float b, float c3) { return fmaxf(fmaxf(a, b), c3); }
// wave-level ordering point between LDS stores and loads of the SAME wave
__device__ __forceinline__ void da_wave_sync() {
#ifdef CENET_HOSTSIM_BUILD
  hipsim::wave_barrier();
#else
  __builtin_amdgcn_wave_barrier();
#endif
}

// every global load issued so far has landed (vmcnt(0); expcnt / lgkmcnt left alone).  Stands once between the prologue loads
// (operand fragments, tile 0) and the key / query loop: the prologue's own wait sits inside the divergent block of its LDS write,
// so without this the loop is entered with loads that MAY be pending and the compiler waits for them in front of the first
// MFMA of every trip — behind the trip's prefetch.
__device__ __forceinline__ void da_loads_landed() {
#ifndef CENET_HOSTSIM_BUILD
  __builtin_amdgcn_s_waitcnt(0x0F70);
#endif
}

struct DiffArgs {
  const bf *q, *k, *v;  // row-major: q, k [B, N, 2H*hd] ; v [B, N, H*2hd]
  bf* U;                // [B, 2H, N, 2hd]
  float* lse;           // [B, 2H, N]  (natural log)
  const bf* dU;         // [B, 2H, N, 2hd]
  bf *dq, *dk, *dv;     // like q, k, v
  bf* aug;              // [B, 2H, N, 16]: lse/scale as 3 bf16 terms at [0..2], delta at [8..10] (written by dQ, read by dK/dV)
  int B, H, N, hd;
  float scale;
  int bmul;             // batch stride of q / k / v / dq / dk / dv in units of their own [N, row] block (1: dense)
};

// ---- LDS images -------------------------------------------------------------------------------------------------------------
// one 16-byte chunk in registers (chunks are 16-byte aligned: da_fill checks the bases, every row and column offset is a multiple
// of 8 elements).  A 4-word vector, not a byte copy into an unsigned[4]: with several chunks per thread the compiler took the
// copied registers apart into 16-bit pieces and put them together again with shifts and masks (64 - 100 vector instructions per
// trip in the dK/dV kernels at HDP >= 32).
#ifdef CENET_HOSTSIM_BUILD
struct da_u4 { unsigned x, y, z, w; };
#else
typedef unsigned da_u4 __attribute__((ext_vector_type(4)));
#endif
// One staged 16-byte chunk of a thread: 8 consecutive elements of one global row -> 8 consecutive elements of one image row.
// A fetch is a straight line of loads: every thread loads 16 bytes for every chunk slot, unconditionally, from an address that
// always lies inside the chunk's tensor — a row beyond the tensor reads the tensor's last row instead, a chunk in the zero
// padding of the image (or a slot past the image) reads a real chunk of the same tensor.  What the image gets in those cases
// (the fill pattern) is selected on the landed registers, in da_land, directly in front of the LDS write.  (A load under a
// branch sits in a basic block of its own, followed by its wait: at HDP >= 32 the dK/dV kernels went through three to seven
// memory round trips one after another at the top of every trip, before the first MFMA.)  For the same reason the loops
// fetch on EVERY trip, the last one included (its rows are all clamped, nothing of it is staged): under `if (more)` the
// prefetch registers are carried around the branch, the loads land in temporaries and are copied — behind a wait.
struct DaChunk {
  const bf* g;   // address of the chunk's columns in row 0 of its tensor (padding chunk / empty slot: of a real chunk)
  int lrow;      // row inside the 32-row tile; DA_NOROW: padding chunk or empty slot (never a row of the tensor)
  int loff;      // element offset inside the image (-1: empty slot, nothing is staged)
  unsigned fill; // low word of the 16-byte fill pattern for rows beyond the tensor (rest zero)
};
#define DA_NOROW 0x40000000
// row0 = first row of the tile, N = rows of the tensor (>= 1), stride = elements per row
__device__ __forceinline__ void da_fetch(const DaChunk& c, int row0, int N, int stride, da_u4& r) {
  const int row = row0 + c.lrow < N ? row0 + c.lrow : N - 1;
  r = *(const da_u4*)(c.g + (long)row * stride);
}
// the staged value of a fetched chunk: the landed bytes for a row of the tensor, the fill pattern otherwise; H4 (half = 0 / 1, -1:
// not a q / k chunk): the two heads of a pair share the 16-byte row, the chunk keeps half `half` in its low 8 bytes (da_half)
__device__ __forceinline__ da_u4 da_land(const DaChunk& c, int rows_left, da_u4 r, int half) {
  const bool ok = c.lrow < rows_left;
  r.x = ok ? r.x : c.fill;
  r.y = ok ? r.y : 0u;
  r.z = ok ? r.z : 0u;
  r.w = ok ? r.w : 0u;
  if (half >= 0) {
    if (half) r.x = r.z, r.y = r.w;
    r.z = r.w = 0u;
  }
  return r;
}
// row-major fragment: 8 consecutive columns [col + 8hh, +8) of image row `row`
__device__ __forceinline__ bf16x8 da_rm(const bf* img, int pitch, int row, int col, int hh) {
  bf16x8 f;
  memcpy(&f, img + row * pitch + col + 8 * hh, 16);
  return f;
}
// transposed fragment for k-step s2: lane (r = lane & 31, hh) gets column C0 + r of image rows 16 s2 + 4hh + {0..3} and
// 16 s2 + 8 + 4hh + {0..3} — the accumulator-row order of da_pack8.  Device: two ds_read_b64_tr_b16 (per 16-lane group a
// 4-row x 16-column block: lane 4q+p supplies the address of row q, columns 4p..4p+3, lane i receives column i).
__device__ __forceinline__ bf16x8 da_tr(const bf* img, int pitch, int s2, int C0, int lane) {
  const int hh = lane >> 5;
  bf16x8 f;
#ifdef CENET_HOSTSIM_BUILD
  const int r = lane & 31;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (short)img[(16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3)) * pitch + C0 + r];
#else
  const int g2 = (lane >> 4) & 1, i = lane & 15, q = i >> 2, p = i & 3;
  const bf* a0 = img + (16 * s2 + 4 * hh + q) * pitch + C0 + 16 * g2 + 4 * p;
  const da_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((da_s4 __attribute__((address_space(3)))*)a0);
  const da_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((da_s4 __attribute__((address_space(3)))*)(a0 + 8 * pitch));
  f[0] = lo[0], f[1] = lo[1], f[2] = lo[2], f[3] = lo[3];
  f[4] = hi[0], f[5] = hi[1], f[6] = hi[2], f[7] = hi[3];
#endif
  return f;
}
__device__ __forceinline__ bf16x8 da_ld8(const bf* p, bool ok) {
  bf16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) memcpy(&f, p, 16);
  return f;
}
// hd = 4: the two heads of a pair share one 16-byte row (q_{2h} | q_{2h+1}); the chunk / fragment is loaded whole and half s is
// kept in elements 0..3, elements 4..7 zeroed (the padding columns of the HDP = 16 tile)
__device__ __forceinline__ void da_half(unsigned (&r)[4], int s) {
  if (s) r[0] = r[2], r[1] = r[3];
  r[2] = r[3] = 0u;
}
__device__ __forceinline__ bf16x8 da_ld4h(const bf* pair, int s, bool ok) {
  unsigned u[4] = {0u, 0u, 0u, 0u};
  if (ok) {
    memcpy(u, pair, 16);
    da_half(u, s);
  }
  bf16x8 f;
  memcpy(&f, u, 16);
  return f;
}
__device__ __forceinline__ bf16x8 da_pack8(const f32x16& x, int s) {  // registers 8s .. 8s+7 -> one B fragment
  unsigned u[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = cenet_pack_bf2(x[8 * s + 2 * j], x[8 * s + 2 * j + 1]);
  bf16x8 f;
  memcpy(&f, u, 16);
  return f;
}
__device__ __forceinline__ int da_row(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }
__device__ __forceinline__ f32x16 da_zero() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
struct da_true { static constexpr bool value = true; };
struct da_false { static constexpr bool value = false; };
#define DA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// x as hi + mid + lo with bf16 terms (24 significant bits)
__device__ __forceinline__ void da_split3(float x, unsigned short* o) {
  const unsigned h = cenet_f2bf(x);
  const float r1 = x - cenet_bf2f(h);
  const unsigned m = cenet_f2bf(r1);
  const unsigned l = cenet_f2bf(r1 - cenet_bf2f(m));
  o[0] = (unsigned short)h, o[1] = (unsigned short)m, o[2] = (unsigned short)l;
}

// image geometry (elements): K / Q image = both heads of the pair side by side, V / dU image = one value head
template <int HDP>
struct DaGeo {
  static constexpr int DVP = 2 * HDP;
  static constexpr int KP = 2 * HDP + 8;   // pitch of the K / Q image (16-byte row reads conflict-free)
  static constexpr int VPT = DVP;          // pitch of a value image that is only read transposed (forward)
  static constexpr int VPR = DVP + 8;      // pitch of a value image that is also read by rows
  static constexpr int CK = 2 * HDP / 8, CV = DVP / 8;  // 16-byte chunks per row
};

// ---------------------------------------------------------------------------------------------------------------------------
// forward: wave = QT tiles of 32 queries x both softmax heads of pair h; workgroup = 4 waves; grid (ceil(N / (128 QT)), B*H)
// ---------------------------------------------------------------------------------------------------------------------------
// ONE: a single softmax over BOTH halves of the pair's 2*HDP query / key columns (one head of dimension 2*HDP = value width):
// plain attention with head dimension 64 through the same tiles — the two half-products add into one score tile.  Tensors:
// q, k, v [B, N, H*2HDP], U [B, H, N, 2HDP], lse / aug rows [B, H, N].
// Workgroups per CU the registers of an instance are bounded for: MINB, except for the single-softmax instance at HDP = 32.  That
// one takes 129 registers with one tile body in the key loop; bounded to FOUR workgroups it takes 127, nothing spilled (17.6 KB of
// LDS fit four times): 0.203 -> 0.181 ms through ops.nonlocal_attention at 56x56, batch 32, same box.  The instance keeps the
// template arguments <32, 1, 2, true> — its symbol is the key of the committed profiles — so the `2` written at its launch site
// (cenet_attn64_fwd_bf16) is NOT its bound; a static_assert there says so.
constexpr int da_fwd_wg_per_cu(int hdp, int minb, bool one) { return (one && hdp == 32) ? 4 : minb; }
template <int HDP, int QT, int MINB, bool ONE, bool H4 = false>
__global__ __launch_bounds__(256, da_fwd_wg_per_cu(HDP, MINB, ONE)) void dattn_fwd_kernel(DiffArgs a) {
  typedef DaGeo<HDP> G;
  constexpr int NKS = HDP / 16, NDT = G::DVP / 32, NH = ONE ? 1 : 2;
  constexpr int KIMG = 32 * G::KP, VIMG = 32 * G::VPT + 64, IMG = KIMG + VIMG;  // (+64: transposed reads of padded rows)
  constexpr int NCH = 32 * (G::CK + G::CV), CPT = (NCH + 255) / 256;
  __shared__ __attribute__((aligned(16))) bf lds[2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const cenet_bid bid = cenet_xcd_block();
  const int b = bid.y / a.H, h = bid.y - b * a.H;
  const int q0 = (bid.x * 4 + wave) * (32 * QT);
  const int N = a.N, hd = a.hd, dv = 2 * hd, E = 2 * a.H * hd;
  const float c = a.scale * DA_LOG2E;
  const bf* qb = a.q + (long)b * a.bmul * N * E;
  const bf* kb = a.k + (long)b * a.bmul * N * E;
  const bf* vb = a.v + (long)b * a.bmul * N * (a.H * dv) + h * dv;

  // this thread's staged chunks (fixed for the whole key loop)
  DaChunk ch[CPT];
  int hs[CPT];  // H4: which half of the staged 16-byte pair row the chunk keeps (-1: not a q / k chunk)
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int id = tid + 256 * j;
    ch[j].fill = 0u;
    hs[j] = -1;
    if (id >= NCH) {
      ch[j].g = kb;
      ch[j].lrow = DA_NOROW;
      ch[j].loff = -1;
    } else if (id < 32 * G::CK) {
      const int row = id / G::CK, cc = id - row * G::CK, s = cc / (HDP / 8), c8 = cc - s * (HDP / 8);
      const bool real = H4 ? c8 == 0 : 8 * c8 < hd;  // (else: zero padding of the image, loads the head's first chunk)
      ch[j].lrow = real ? row : DA_NOROW;
      ch[j].loff = row * G::KP + s * HDP + 8 * c8;
      ch[j].g = H4 ? kb + 2 * h * hd : kb + (2 * h + s) * hd + (real ? 8 * c8 : 0);
      hs[j] = s;
    } else {
      const int id2 = id - 32 * G::CK, row = id2 / G::CV, c8 = id2 - row * G::CV;
      const bool real = 8 * c8 < dv;
      ch[j].lrow = real ? row : DA_NOROW;
      ch[j].loff = KIMG + row * G::VPT + 8 * c8;
      ch[j].g = vb + (real ? 8 * c8 : 0);
    }
  }
  da_u4 pre[CPT];
  // (k and v rows have the same length: E = 2 H hd = H dv elements)
  auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < CPT; ++j) da_fetch(ch[j], k0, N, E, pre[j]);
  };
  auto stage = [&](int buf, int k0) __attribute__((always_inline)) {  // k0: first key of the fetched tile
#pragma unroll
    for (int j = 0; j < CPT; ++j)
      if (ch[j].loff >= 0) *(da_u4*)(lds + buf * IMG + ch[j].loff) = da_land(ch[j], N - k0, pre[j], H4 ? hs[j] : -1);
  };

  bf16x8 qf[QT][2][NKS];
  f32x16 O[QT][NH][NDT];
  float m[QT][NH], l[QT][NH];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qi = q0 + 32 * t + r < N ? q0 + 32 * t + r : N - 1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
        qf[t][s][ks] = H4 ? da_ld4h(qb + (long)qi * E + 2 * h * hd, s, hh == 0)
                          : da_ld8(qb + (long)qi * E + (2 * h + s) * hd + 16 * ks + 8 * hh, 16 * ks + 8 * hh < hd);
    }
#pragma unroll
    for (int s = 0; s < NH; ++s) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) O[t][s][dt] = da_zero();
      m[t][s] = DA_NEG;
      l[t][s] = 0.f;
    }
  }
  // One score-tile body for the key loop: `masked` selects the instantiation.  The loop below holds ONLY the unmasked one (full
  // 32-key tiles); the masked one runs once, after the loop, on the ragged last tile.  (With both instantiations inside the loop
  // the register allocator gave their accumulators different registers and copied O / dQ across the join on every iteration.)
  auto tile = [&](auto masked, const bf* Kimg, const bf* Vimg, int klim) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(masked)::value;
    // HDP <= 32: the tile's K / V fragments are read once and shared by both heads (and all QT query tiles).  HDP = 64 has
    // 128 accumulator registers per wave: fragments are read where they are used (LATE) — holding them across the softmax
    // cost 640 bytes of scratch per lane when the key loop still held two tile bodies (256 + 256 registers and 400 B of scratch
    // even with LATE; one body: 254 + 148, no scratch, HDP = 48: 208 + 112).  Whether LATE is still needed was not re-measured.
    constexpr bool LATE = HDP > 32;
    bf16x8 kf[LATE ? 1 : 2][NKS], vf[LATE ? 1 : NDT][2];
    if (!LATE) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) kf[LATE ? 0 : s][ks] = da_rm(Kimg, G::KP, r, s * HDP + 16 * ks, hh);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) vf[LATE ? 0 : dt][s2] = da_tr(Vimg, G::VPT, s2, 32 * dt, lane);
    }
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
      for (int s = 0; s < NH; ++s) {
        f32x16 S = da_zero();
#pragma unroll
        for (int sp = (ONE ? 0 : s); sp <= (ONE ? 1 : s); ++sp)
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks)
            S = DA_MFMA(LATE ? da_rm(Kimg, G::KP, r, sp * HDP + 16 * ks, hh) : kf[LATE ? 0 : sp][ks], qf[t][sp][ks], S);  // S^T[key][query]
        if (MASKED) {  // ragged last tile only (its own instantiation of the tile body: no per-score selects elsewhere)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (da_row(i, hh) >= klim) S[i] = DA_NEG;
        }
        float mx = da_max3(S[0], S[1], S[2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) mx = da_max3(mx, S[i], S[i + 1]);
        mx = fmaxf(mx, S[15]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        if (da_any(mx > m[t][s])) {  // some query of the wave raised its maximum: rescale (wave-uniform branch)
          const float mn = fmaxf(m[t][s], mx);
          const float alpha = da_exp2((m[t][s] - mn) * c);
          m[t][s] = mn;
          l[t][s] *= alpha;
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) O[t][s][dt][i] *= alpha;
        }
        const float mc = m[t][s] * c;
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = da_exp2(S[i] * c - mc);
          S[i] = p;
          rs += p;
        }
        l[t][s] += rs;
        const bf16x8 p0 = da_pack8(S, 0), p1 = da_pack8(S, 1);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {  // O^T[value feature][query] += V^T[feature][key] P^T[key][query]
          O[t][s][dt] = DA_MFMA(LATE ? da_tr(Vimg, G::VPT, 0, 32 * dt, lane) : vf[LATE ? 0 : dt][0], p0, O[t][s][dt]);
          O[t][s][dt] = DA_MFMA(LATE ? da_tr(Vimg, G::VPT, 1, 32 * dt, lane) : vf[LATE ? 0 : dt][1], p1, O[t][s][dt]);
        }
      }
  };
  const int nfull = N & ~31;  // keys in full tiles; the same for every wave: equal barrier counts whatever q0
  fetch(0);
  stage(0, 0);
  da_loads_landed();
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < nfull; k0 += 32) {
    const bool more = k0 + 32 < N;  // (the ragged tile is fetched and staged like any other)
    fetch(k0 + 32);
    // (wave-uniform: a wave past the last query only helps with the staging)
    if (q0 < N) tile(da_false(), lds + cur * IMG, lds + cur * IMG + KIMG, 32);
    if (more) stage(cur ^ 1, k0 + 32);
    __syncthreads();
    cur ^= 1;
  }
  // ragged last tile (N % 32 keys): staged by the last loop iteration (by the prologue when N < 32), nothing is staged after it
  if (nfull < N && q0 < N) tile(da_true(), lds + cur * IMG, lds + cur * IMG + KIMG, N - nfull);
  if (q0 >= N) return;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qi = q0 + 32 * t + r;
#pragma unroll
    for (int s = 0; s < NH; ++s) {
      const float lt = l[t][s] + __shfl_xor(l[t][s], 32);
      const long hrow = ((long)b * NH * a.H + NH * h + s) * N + qi;
      if (qi < N) {
        const float inv = 1.f / lt;
        bf* up = a.U + hrow * dv;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int f0 = 32 * dt + 8 * g + 4 * hh;  // four consecutive value features
            if (f0 < dv) {
              float o[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) o[i] = O[t][s][dt][4 * g + i] * inv;
              st4v(up + f0, o);
            }
          }
        if (hh == 0) a.lse[hrow] = m[t][s] * a.scale + logf(lt);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, dQ (+ delta = rowsum(dU * U) and the bf16 statistics rows for dK/dV): wave = 32 queries x both softmax heads
// ---------------------------------------------------------------------------------------------------------------------------
// (HDP <= 16: three workgroups per CU — 167 registers under the 168 cap, nothing spilled (H4: 140); the kernel waits on dependent
// MFMA / exponential chains, a third wave per SIMD covers more of them: 0.78 -> 0.74 ms at DSEB-56x56, same box.  Bounded to four
// workgroups it takes 128 registers and 20 B of scratch and measures 1.394 - 1.403 against 1.402 - 1.420 ms for the whole backward:
// inside the spread, not taken.)
template <int HDP, bool ONE, bool H4 = false>
__global__ __launch_bounds__(256, HDP > 32 ? 1 : (HDP <= 16 ? 3 : 2)) void dattn_bwd_dq_kernel(DiffArgs a) {
  typedef DaGeo<HDP> G;
  constexpr int NKS = HDP / 16, NKD = G::DVP / 16, NH = ONE ? 1 : 2;
  constexpr int NFT = (HDP + 31) / 32;  // 32-feature accumulator tiles per head (HDP = 64: two)
  constexpr int KIMG = 32 * G::KP + 64, VIMG = 32 * G::VPR, IMG = KIMG + VIMG;
  constexpr int NCH = 32 * (G::CK + G::CV), CPT = (NCH + 255) / 256;
  __shared__ __attribute__((aligned(16))) bf lds[2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const cenet_bid bid = cenet_xcd_block();
  const int b = bid.y / a.H, h = bid.y - b * a.H;
  const int q0 = (bid.x * 4 + wave) * 32;
  const int N = a.N, hd = a.hd, dv = 2 * hd, E = 2 * a.H * hd;
  const float c = a.scale * DA_LOG2E;
  const bf* qb = a.q + (long)b * a.bmul * N * E;
  const bf* kb = a.k + (long)b * a.bmul * N * E;
  const bf* vb = a.v + (long)b * a.bmul * N * (a.H * dv) + h * dv;
  const int qi = q0 + r < N ? q0 + r : N - 1;

  DaChunk ch[CPT];
  int hs[CPT];  // H4: which half of the staged 16-byte pair row the chunk keeps (-1: not a q / k chunk)
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int id = tid + 256 * j;
    ch[j].fill = 0u;
    hs[j] = -1;
    if (id >= NCH) {
      ch[j].g = kb;
      ch[j].lrow = DA_NOROW;
      ch[j].loff = -1;
    } else if (id < 32 * G::CK) {
      const int row = id / G::CK, cc = id - row * G::CK, s = cc / (HDP / 8), c8 = cc - s * (HDP / 8);
      const bool real = H4 ? c8 == 0 : 8 * c8 < hd;  // (else: zero padding of the image, loads the head's first chunk)
      ch[j].lrow = real ? row : DA_NOROW;
      ch[j].loff = row * G::KP + s * HDP + 8 * c8;
      ch[j].g = H4 ? kb + 2 * h * hd : kb + (2 * h + s) * hd + (real ? 8 * c8 : 0);
      hs[j] = s;
    } else {
      const int id2 = id - 32 * G::CK, row = id2 / G::CV, c8 = id2 - row * G::CV;
      const bool real = 8 * c8 < dv;
      ch[j].lrow = real ? row : DA_NOROW;
      ch[j].loff = KIMG + row * G::VPR + 8 * c8;
      ch[j].g = vb + (real ? 8 * c8 : 0);
    }
  }
  da_u4 pre[CPT];
  // (k and v rows have the same length: E = 2 H hd = H dv elements)
  auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < CPT; ++j) da_fetch(ch[j], k0, N, E, pre[j]);
  };
  auto stage = [&](int buf, int k0) __attribute__((always_inline)) {  // k0: first key of the fetched tile
#pragma unroll
    for (int j = 0; j < CPT; ++j)
      if (ch[j].loff >= 0) *(da_u4*)(lds + buf * IMG + ch[j].loff) = da_land(ch[j], N - k0, pre[j], H4 ? hs[j] : -1);
  };

  bf16x8 qf[2][NKS], gf[NH][NKD];
  float lse2[NH], dl[NH];
  f32x16 dq[2][NFT];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      qf[s][ks] = H4 ? da_ld4h(qb + (long)qi * E + 2 * h * hd, s, hh == 0)
                     : da_ld8(qb + (long)qi * E + (2 * h + s) * hd + 16 * ks + 8 * hh, 16 * ks + 8 * hh < hd);
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) dq[s][ft] = da_zero();
  }
#pragma unroll
  for (int s = 0; s < NH; ++s) {
    const long hrow = ((long)b * NH * a.H + NH * h + s) * N + qi;
    float acc = 0.f;
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) {
      const bool ok = 16 * kd + 8 * hh < dv;
      gf[s][kd] = da_ld8(a.dU + hrow * dv + 16 * kd + 8 * hh, ok);
      const bf16x8 uf = da_ld8(a.U + hrow * dv + 16 * kd + 8 * hh, ok);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += cenet_bf2f((unsigned short)gf[s][kd][j]) * cenet_bf2f((unsigned short)uf[j]);
    }
    acc += __shfl_xor(acc, 32);
    dl[s] = acc;
    const float lse = a.lse[hrow];
    lse2[s] = lse * DA_LOG2E;
    if (q0 + r < N) {  // statistics rows for the dK/dV kernel: lane half 0 writes lse / scale, half 1 writes delta
      unsigned short row8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      da_split3(hh == 0 ? lse / a.scale : acc, row8);
      memcpy(a.aug + hrow * 16 + 8 * hh, row8, 16);
    }
  }
  // one tile body; the key loop holds only its unmasked instantiation, the ragged last tile runs once after it (see the forward)
  auto tile = [&](auto masked, const bf* Kimg, const bf* Vimg, int klim) __attribute__((always_inline)) {
    constexpr bool MASKED = decltype(masked)::value;
    bf16x8 vf[NKD];
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) vf[kd] = da_rm(Vimg, G::VPR, r, 16 * kd, hh);
#pragma unroll
    for (int s = 0; s < NH; ++s) {
      // the query is the MFMA column: its delta is a lane constant, so the dP chain can start from -delta (dP - delta comes out
      // of the accumulator: one VALU instruction per score less).  Not at HDP = 16: a zero accumulator is an inline constant of
      // the first MFMA, a -delta one is 16 live registers more, and that instance sat on its 168-register cap (30 spilled) while
      // the key loop held two tile bodies.  With one body it fits (165 registers, no scratch) but trades the 30 packed ops of the
      // step for scalar ones, 123 -> 121 vector instructions: 1.370 - 1.416 against 1.417 - 1.425 ms for the DSEB-56x56 backward, same
      // box — inside the spread, left as it is.
      constexpr bool INITD = HDP > 16;
      f32x16 S = da_zero(), dP;
#pragma unroll
      for (int i = 0; i < 16; ++i) dP[i] = INITD ? -dl[s] : 0.f;
#pragma unroll
      for (int sp = (ONE ? 0 : s); sp <= (ONE ? 1 : s); ++sp)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) S = DA_MFMA(da_rm(Kimg, G::KP, r, sp * HDP + 16 * ks, hh), qf[sp][ks], S);
#pragma unroll
      for (int kd = 0; kd < NKD; ++kd) dP = DA_MFMA(vf[kd], gf[s][kd], dP);  // dP^T[key][query] = V dU^T - delta
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float p = da_exp2(S[i] * c - lse2[s]);
        if (MASKED && da_row(i, hh) >= klim) p = 0.f;
        S[i] = INITD ? p * dP[i] : p * (dP[i] - dl[s]);
      }
      // dQ^T[d][query] += K^T[d][key] dS^T[key][query]; accumulator rows >= hd (the other head's columns, padding) are
      // never stored
#pragma unroll
      for (int sp = (ONE ? 0 : s); sp <= (ONE ? 1 : s); ++sp)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8 dsB = da_pack8(S, s2);
#pragma unroll
          for (int ft = 0; ft < NFT; ++ft)
            dq[sp][ft] = DA_MFMA(da_tr(Kimg, G::KP, s2, sp * HDP + 32 * ft, lane), dsB, dq[sp][ft]);
        }
    }
  };
  const int nfull = N & ~31;
  fetch(0);
  stage(0, 0);
  da_loads_landed();
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < nfull; k0 += 32) {
    const bool more = k0 + 32 < N;
    fetch(k0 + 32);
    if (q0 < N) tile(da_false(), lds + cur * IMG, lds + cur * IMG + KIMG, 32);
    if (more) stage(cur ^ 1, k0 + 32);
    __syncthreads();
    cur ^= 1;
  }
  if (nfull < N && q0 < N) tile(da_true(), lds + cur * IMG, lds + cur * IMG + KIMG, N - nfull);
  if (q0 + r < N) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf* dp = a.dq + ((long)b * a.bmul * N + qi) * E + (2 * h + s) * hd;
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft)
#pragma unroll
        for (int g = 0; g < (HDP < 32 ? HDP / 8 : 4); ++g) {
          const int d0 = 32 * ft + 8 * g + 4 * hh;
          if (d0 < hd) {
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = dq[s][ft][4 * g + i] * a.scale;
            st4v(dp + d0, o);
          }
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, dK / dV: wave = 32 keys x both softmax heads (one shared dV accumulator); streams query tiles
// ---------------------------------------------------------------------------------------------------------------------------
template <int HDP, bool ONE, bool H4 = false>
__global__ __launch_bounds__(256, HDP > 32 ? 1 : 2) void dattn_bwd_dkv_kernel(DiffArgs a) {
  typedef DaGeo<HDP> G;
  constexpr int NKS = HDP / 16, NKD = G::DVP / 16, NDT = G::DVP / 32, NH = ONE ? 1 : 2;
  constexpr int NFT = (HDP + 31) / 32;  // 32-feature accumulator tiles of dK per head
  constexpr int AP = 40;  // statistics image: [query][head s: lse(8) delta(8)] + pad
  constexpr int QIMG = 32 * G::KP + 64, GIMG = 32 * G::VPR + 64, AIMG = 32 * AP, IMG = QIMG + NH * GIMG + AIMG;
  constexpr int NCH = 32 * (G::CK + NH * G::CV + 2 * NH), CPT = (NCH + 255) / 256;
  __shared__ __attribute__((aligned(16))) bf lds[2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const cenet_bid bid = cenet_xcd_block();
  const int b = bid.y / a.H, h = bid.y - b * a.H;
  const int k0 = (bid.x * 4 + wave) * 32;
  const int N = a.N, hd = a.hd, dv = 2 * hd, E = 2 * a.H * hd;
  const float c = a.scale * DA_LOG2E;
  const bf* qb = a.q + (long)b * a.bmul * N * E;
  const bf* kb = a.k + (long)b * a.bmul * N * E;
  const bf* vb = a.v + (long)b * a.bmul * N * (a.H * dv) + h * dv;
  const long hb0 = ((long)b * NH * a.H + NH * h) * N;  // (b, head 2h) row base of dU / aug; head 2h+1 is N rows further
  const int ki = k0 + r < N ? k0 + r : N - 1;

  DaChunk ch[CPT];
  int gstride[CPT];  // elements per row of the chunk's tensor
  int hs[CPT];      // H4: which half of the staged 16-byte pair row the chunk keeps (-1: not a q chunk)
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    int id = tid + 256 * j;
    ch[j].fill = 0u;
    hs[j] = -1;
    if (id >= NCH) {
      ch[j].g = qb;
      ch[j].lrow = DA_NOROW;
      ch[j].loff = -1;
      gstride[j] = E;
    } else if (id < 32 * G::CK) {  // Q rows, both heads
      const int row = id / G::CK, cc = id - row * G::CK, s = cc / (HDP / 8), c8 = cc - s * (HDP / 8);
      const bool real = H4 ? c8 == 0 : 8 * c8 < hd;  // (else: zero padding of the image, loads the head's first chunk)
      ch[j].lrow = real ? row : DA_NOROW;
      ch[j].loff = row * G::KP + s * HDP + 8 * c8;
      ch[j].g = H4 ? qb + 2 * h * hd : qb + (2 * h + s) * hd + (real ? 8 * c8 : 0);
      hs[j] = s;
      gstride[j] = E;
    } else if ((id -= 32 * G::CK) < NH * 32 * G::CV) {  // dU rows of head s
      const int s = id / (32 * G::CV), id2 = id - s * 32 * G::CV, row = id2 / G::CV, c8 = id2 - row * G::CV;
      const bool real = 8 * c8 < dv;
      ch[j].lrow = real ? row : DA_NOROW;
      ch[j].loff = QIMG + s * GIMG + row * G::VPR + 8 * c8;
      ch[j].g = a.dU + (hb0 + (long)s * N) * dv + (real ? 8 * c8 : 0);
      gstride[j] = dv;
    } else {  // statistics rows: chunk (row, s, kind): kind 0 = lse / scale, 1 = delta
      id -= NH * 32 * G::CV;
      const int row = id / (2 * NH), s = (id - row * 2 * NH) >> 1, kind = id & 1;
      ch[j].lrow = row;
      ch[j].loff = QIMG + NH * GIMG + row * AP + s * 16 + 8 * kind;
      ch[j].g = a.aug + (hb0 + (long)s * N) * 16 + 8 * kind;
      ch[j].fill = kind == 0 ? 0x7149u : 0u;  // rows beyond N: lse / scale = 1e30 -> probability 0
      gstride[j] = 16;
    }
  }
  da_u4 pre[CPT];
  auto fetch = [&](int q0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < CPT; ++j) da_fetch(ch[j], q0, N, gstride[j], pre[j]);
  };
  auto stage = [&](int buf, int q0) __attribute__((always_inline)) {  // q0: first query of the fetched tile
#pragma unroll
    for (int j = 0; j < CPT; ++j)
      if (ch[j].loff >= 0) *(da_u4*)(lds + buf * IMG + ch[j].loff) = da_land(ch[j], N - q0, pre[j], H4 ? hs[j] : -1);
  };

  bf16x8 kfB[2][NKS], vfB[NKD];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      kfB[s][ks] = H4 ? da_ld4h(kb + (long)ki * E + 2 * h * hd, s, hh == 0)
                      : da_ld8(kb + (long)ki * E + (2 * h + s) * hd + 16 * ks + 8 * hh, 16 * ks + 8 * hh < hd);
#pragma unroll
  for (int kd = 0; kd < NKD; ++kd) vfB[kd] = da_ld8(vb + (long)ki * (a.H * dv) + 16 * kd + 8 * hh, 16 * kd + 8 * hh < dv);
  // constant B fragment of the statistics k-step: -1 at k = 0, 1, 2 (lane half 0), zero elsewhere
  bf16x8 negB = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hh == 0) negB[0] = negB[1] = negB[2] = (short)0xBF80;
  f32x16 dK[2][NFT], dV[NDT];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) dK[s][ft] = da_zero();
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) dV[dt] = da_zero();

  fetch(0);
  stage(0, 0);
  da_loads_landed();
  __syncthreads();
  int cur = 0;
  for (int q0 = 0; q0 < N; q0 += 32) {
    const bool more = q0 + 32 < N;
    fetch(q0 + 32);
    const bf* Qimg = lds + cur * IMG;
    const bf* Aimg = Qimg + QIMG + NH * GIMG;
    if (k0 < N) {
#pragma unroll
      for (int s = 0; s < NH; ++s) {
        const bf* Gimg = Qimg + QIMG + s * GIMG;
        f32x16 S = da_zero(), dP = da_zero();
#pragma unroll
        for (int sp = (ONE ? 0 : s); sp <= (ONE ? 1 : s); ++sp)
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks) S = DA_MFMA(da_rm(Qimg, G::KP, r, sp * HDP + 16 * ks, hh), kfB[sp][ks], S);  // S[q][key]
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd) dP = DA_MFMA(da_rm(Gimg, G::VPR, r, 16 * kd, hh), vfB[kd], dP);  // dP[q][key] = dU V^T
        // row (query) statistics through the contraction: S -= lse / scale, dP -= delta
        // both lane halves read the row: the upper half's k = 8..15 meets the zero rows of negB, so its products are exact zeros
        // and the result is bit-identical to loading the lower half only — for FINITE statistics, which is every staged term of a
        // finite problem (three bf16 terms + five zeros per row from the dQ kernel, the finite fill 0x7149 beyond N).  A non-finite
        // lse or delta (non-finite inputs only) now meets 0 in the upper half too: inf * 0 = NaN for that query's row, where the
        // lower-half load kept it to the terms it touches.  No zero-filled fragments (16 v_mov_b32), no divergent branch per head.
        bf16x8 al, ad;
        memcpy(&al, Aimg + r * AP + s * 16, 16);
        memcpy(&ad, Aimg + r * AP + s * 16 + 8, 16);
        S = DA_MFMA(al, negB, S);
        dP = DA_MFMA(ad, negB, dP);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = da_exp2(S[i] * c);
          S[i] = p;
          dP[i] = p * dP[i];
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8 pB = da_pack8(S, s2), dsB = da_pack8(dP, s2);
          // dV^T[feature][key] += dU^T[feature][query] P[query][key]
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) dV[dt] = DA_MFMA(da_tr(Gimg, G::VPR, s2, 32 * dt, lane), pB, dV[dt]);
          // dK^T[d][key] += Q^T[d][query] dS[query][key]   (accumulator rows >= hd are never stored)
#pragma unroll
          for (int sp = (ONE ? 0 : s); sp <= (ONE ? 1 : s); ++sp)
#pragma unroll
            for (int ft = 0; ft < NFT; ++ft)
              dK[sp][ft] = DA_MFMA(da_tr(Qimg, G::KP, s2, sp * HDP + 32 * ft, lane), dsB, dK[sp][ft]);
        }
      }
    }
    if (more) stage(cur ^ 1, q0 + 32);
    __syncthreads();
    cur ^= 1;
  }
  if (k0 + r < N) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf* dp = a.dk + ((long)b * a.bmul * N + ki) * E + (2 * h + s) * hd;
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft)
#pragma unroll
        for (int g = 0; g < (HDP < 32 ? HDP / 8 : 4); ++g) {
          const int d0 = 32 * ft + 8 * g + 4 * hh;
          if (d0 < hd) {
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = dK[s][ft][4 * g + i] * a.scale;
            st4v(dp + d0, o);
          }
        }
    }
    bf* dvp = a.dv + ((long)b * a.bmul * N + ki) * (a.H * dv) + h * dv;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f0 = 32 * dt + 8 * g + 4 * hh;
        if (f0 < dv) {
          float o[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = dV[dt][4 * g + i];
          st4v(dvp + f0, o);
        }
      }
  }
}

// head dims served: 8 and 16 (one k-step), 32 (two), 64 (four k-steps, two 32-feature accumulator tiles per head: the
// 64x64-token level of the 512x512 three-scale preset, skin.sh:93-94); for skip_mode='add' (embed = C instead of 2C):
// 4 (Synapse 56x56: the HDP = 16 tiles, the pair's two heads share one 16-byte row, H4) and 40 (ACDC 14x14: HDP = 48, three
// k-steps and three 32-feature value tiles; the HDP = 64 tiles stay selectable for the A/B, da_hd40_p64).  Columns past hd are
// zero in LDS and in the fragments, so scores and gradients are exact, and nothing is stored past the real columns.
extern "C" int cenet_diffattn_heads_supported(int hd, int N) {
  return (hd == 4 || hd == 8 || hd == 16 || hd == 32 || hd == 40 || hd == 64) && N >= 1;
}
// measurement aid (tools/skip_add_ab.py): hd = 40 through the HDP = 64 instances instead of HDP = 48; read per call so that one
// process can time both
static bool da_hd40_p64() {
  const char* e = getenv("CENET_DATTN_HD40_HDP64");
  return e && e[0] == '1';
}
extern "C" long cenet_diffattn_heads_ws_bytes(int B, int H, int N) { return (long)B * 2 * H * N * 16 * 2; }

static int da_fill(DiffArgs& a, const cenet_diffattn_t* p) {
  if (!p || !p->q || !p->k || !p->v || !p->U || !p->lse) return CENET_EINVAL;
  if (p->B <= 0 || p->H <= 0 || p->N <= 0 || !cenet_diffattn_heads_supported(p->hd, p->N)) return CENET_EUNSUPPORTED;
  a.q = (const bf*)p->q; a.k = (const bf*)p->k; a.v = (const bf*)p->v;
  a.U = (bf*)p->U; a.lse = p->lse; a.dU = (const bf*)p->dU;
  a.dq = (bf*)p->dq; a.dk = (bf*)p->dk; a.dv = (bf*)p->dv; a.aug = (bf*)p->ws;
  a.B = p->B; a.H = p->H; a.N = p->N; a.hd = p->hd; a.scale = p->scale;
  a.bmul = p->batch_mul > 0 ? p->batch_mul : 1;
  const uintptr_t m = (uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.U | (uintptr_t)a.dU | (uintptr_t)a.dq |
                      (uintptr_t)a.dk | (uintptr_t)a.dv | (uintptr_t)a.aug;
  if (m & 15) return CENET_EINVAL;  // rows are moved in 16-byte chunks
  return CENET_OK;
}

extern "C" int cenet_diffattn_heads_fwd_bf16(const cenet_diffattn_t* p, hipStream_t stream) {
  DiffArgs a;
  const int rc = da_fill(a, p);
  if (rc != CENET_OK) return rc;
  const int bh = a.B * a.H;
  if (a.hd == 4) {
    CENET_LAUNCH((dattn_fwd_kernel<16, 1, 3, false, true>), dim3(cdiv(a.N, 128), bh), dim3(256), stream, a);
  } else if (a.hd <= 16) {
    // one 32-query tile per wave; bounded to three workgroups per CU, the kernel takes 122 registers and runs four (two tiles
    // per wave: 198 registers, two workgroups)
    CENET_LAUNCH((dattn_fwd_kernel<16, 1, 3, false>), dim3(cdiv(a.N, 128), bh), dim3(256), stream, a);
  } else if (a.hd <= 32) {
    CENET_LAUNCH((dattn_fwd_kernel<32, 1, 2, false>), dim3(cdiv(a.N, 128), bh), dim3(256), stream, a);
  } else if (a.hd == 40 && !da_hd40_p64()) {
    CENET_LAUNCH((dattn_fwd_kernel<48, 1, 1, false>), dim3(cdiv(a.N, 128), bh), dim3(256), stream, a);
  } else {
    CENET_LAUNCH((dattn_fwd_kernel<64, 1, 1, false>), dim3(cdiv(a.N, 128), bh), dim3(256), stream, a);
  }
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_diffattn_heads_bwd_bf16(const cenet_diffattn_t* p, hipStream_t stream) {
  DiffArgs a;
  const int rc = da_fill(a, p);
  if (rc != CENET_OK) return rc;
  if (!a.dU || !a.dq || !a.dk || !a.dv || !a.aug) return CENET_EINVAL;
  const dim3 grid(cdiv(a.N, 128), a.B * a.H);
  if (a.hd == 4) {
    CENET_LAUNCH((dattn_bwd_dq_kernel<16, false, true>), grid, dim3(256), stream, a);
    CENET_LAUNCH((dattn_bwd_dkv_kernel<16, false, true>), grid, dim3(256), stream, a);
  } else if (a.hd <= 16) {
    CENET_LAUNCH((dattn_bwd_dq_kernel<16, false>), grid, dim3(256), stream, a);
    CENET_LAUNCH((dattn_bwd_dkv_kernel<16, false>), grid, dim3(256), stream, a);
  } else if (a.hd <= 32) {
    CENET_LAUNCH((dattn_bwd_dq_kernel<32, false>), grid, dim3(256), stream, a);
    CENET_LAUNCH((dattn_bwd_dkv_kernel<32, false>), grid, dim3(256), stream, a);
  } else if (a.hd == 40 && !da_hd40_p64()) {
    CENET_LAUNCH((dattn_bwd_dq_kernel<48, false>), grid, dim3(256), stream, a);
    CENET_LAUNCH((dattn_bwd_dkv_kernel<48, false>), grid, dim3(256), stream, a);
  } else {
    CENET_LAUNCH((dattn_bwd_dq_kernel<64, false>), grid, dim3(256), stream, a);
    CENET_LAUNCH((dattn_bwd_dkv_kernel<64, false>), grid, dim3(256), stream, a);
  }
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// ---- plain self-attention with head dimension 64 or 128 through the pair tiles (ONE softmax over both halves) ----------------
// q, k, v [B, N, H*hd] (token-major), U / dU [B, H, N, hd], lse [B, H, N]; ws: cenet_attn64_ws_bytes.  The caller passes
// hd = 64 or 128; inside, a head is a "pair" of two hd/2-wide halves (DiffArgs.hd = 32 / 64).  Used by the Non-local blocks of
// the 56x56 (C = 64, N = 3136) and 28x28 (C = 128, N = 784) decoder levels (nlb.py:117-138).
extern "C" long cenet_attn64_ws_bytes(int B, int H, int N) { return (long)B * H * N * 16 * 2; }

static int da_fill64(DiffArgs& a, const cenet_diffattn_t* p) {
  if (!p || !p->q || !p->k || !p->v || !p->U || !p->lse) return CENET_EINVAL;
  if (p->B <= 0 || p->H <= 0 || p->N <= 0 || (p->hd != 64 && p->hd != 128)) return CENET_EUNSUPPORTED;
  a.q = (const bf*)p->q; a.k = (const bf*)p->k; a.v = (const bf*)p->v;
  a.U = (bf*)p->U; a.lse = p->lse; a.dU = (const bf*)p->dU;
  a.dq = (bf*)p->dq; a.dk = (bf*)p->dk; a.dv = (bf*)p->dv; a.aug = (bf*)p->ws;
  a.B = p->B; a.H = p->H; a.N = p->N; a.hd = p->hd / 2; a.scale = p->scale;  // a head = a "pair" of two hd/2-wide halves
  a.bmul = p->batch_mul > 0 ? p->batch_mul : 1;
  const uintptr_t m = (uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.U | (uintptr_t)a.dU | (uintptr_t)a.dq |
                      (uintptr_t)a.dk | (uintptr_t)a.dv | (uintptr_t)a.aug;
  if (m & 15) return CENET_EINVAL;
  return CENET_OK;
}

extern "C" int cenet_attn64_fwd_bf16(const cenet_diffattn_t* p, hipStream_t stream) {
  DiffArgs a;
  const int rc = da_fill64(a, p);
  if (rc != CENET_OK) return rc;
  // <32, 1, 2, true> is bounded to four workgroups per CU, not to the two of its MINB argument (da_fwd_wg_per_cu)
  static_assert(da_fwd_wg_per_cu(32, 2, true) == 4, "the single-softmax HDP = 32 forward is built for four workgroups per CU");
  if (a.hd == 32) CENET_LAUNCH((dattn_fwd_kernel<32, 1, 2, true>), dim3(cdiv(a.N, 128), a.B * a.H), dim3(256), stream, a);
  else CENET_LAUNCH((dattn_fwd_kernel<64, 1, 1, true>), dim3(cdiv(a.N, 128), a.B * a.H), dim3(256), stream, a);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_attn64_bwd_bf16(const cenet_diffattn_t* p, hipStream_t stream) {
  DiffArgs a;
  const int rc = da_fill64(a, p);
  if (rc != CENET_OK) return rc;
  if (!a.dU || !a.dq || !a.dk || !a.dv || !a.aug) return CENET_EINVAL;
  const dim3 grid(cdiv(a.N, 128), a.B * a.H);
  if (a.hd == 32) {
    CENET_LAUNCH((dattn_bwd_dq_kernel<32, true>), grid, dim3(256), stream, a);
    CENET_LAUNCH((dattn_bwd_dkv_kernel<32, true>), grid, dim3(256), stream, a);
  } else {
    CENET_LAUNCH((dattn_bwd_dq_kernel<64, true>), grid, dim3(256), stream, a);
    CENET_LAUNCH((dattn_bwd_dkv_kernel<64, true>), grid, dim3(256), stream, a);
  }
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Spatial-reduction attention (pvtv2.py:88-109), backward, bf16: head dimension 64, at most 64 keys (the 7x7 = 49 keys the
// reduction convs leave at every stage) under 49 ... 3136 queries.  ONE kernel instead of the dQ + dK/dV pair of
// attn_bf16.hip: the whole key / value set of a (batch, head) sits in LDS, a wave owns 32-query tiles and computes, per tile,
//   phase A (query = MFMA column, as dattn_bwd_dq):  S^T, dP^T -> dS^T -> dQ^T ; delta and lse as per-lane scalars;
//   phase B (key = MFMA column, as dattn_bwd_dkv):    S, dP recomputed from the tile's Q / dO images (two MFMA groups:
//            cheaper than transposing dS through LDS) -> dV^T += dO^T P, dK^T += Q^T dS, accumulated in registers over the wave's
//            tiles; the four waves meet in LDS and the workgroup adds one 64 x 128 fp32 block into dkv.
// q, o, dout, dq [B, Nq, C], kv [B, Nk, 2C] (k = columns 0..C, v = C..2C), head h = columns 64h..64h+63, lse [B, H, Nq]
// (natural log of the scaled scores, as the forward kernel leaves it), dkv [B, Nk, 2C] fp32, zero-filled by the caller.
// ---------------------------------------------------------------------------------------------------------------------------
struct SraArgs {
  const bf *q, *kv, *o, *dout;
  const float* lse;
  bf* dq;
  float* dkv;
  bf* dkv_bf;  // non-null: ONE workgroup per (batch, head) stores dK/dV as bf16 directly (no zero fill, atomics or cast pass)
  int B, H, Nq, Nk, C, tiles;  // tiles: 32-query tiles per wave
  float scale;
};

// K and V of a (batch, head) into their resident images: NKB * 64 rows x 8 chunks each, rows >= Nk zero.  One fetch in the sense
// of da_fetch / da_land: a thread owns 4 NKB chunk slots, loads them all back to back (a row >= Nk reads row Nk - 1 of the same
// tensor), and the zero fill is selected on the landed registers in front of the LDS writes — one memory round trip, not one
// per slot.  16 slots (NKB = 4) go as two batches of 8: 32 registers of chunks in flight beside the 49 of tile 0's rows, in an
// instance that runs two waves per SIMD.
template <int NKB, int KP>
__device__ __forceinline__ void sra_stage_kv(const bf* kb, const bf* vb, int Nk, int C, bf* KVimg, int tid) {
  constexpr int CPT = 4 * NKB, BATCH = CPT < 8 ? CPT : 8;
#pragma unroll
  for (int j0 = 0; j0 < CPT; j0 += BATCH) {
    DaChunk ch[BATCH];
    da_u4 pre[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int id = tid + 256 * (j0 + j), which = id / (NKB * 512), rem = id - which * (NKB * 512), row = rem >> 3, c8 = rem & 7;
      ch[j].g = (which ? vb : kb) + 8 * c8;
      ch[j].lrow = row;
      ch[j].loff = which * (NKB * 64 * KP) + row * KP + 8 * c8;  // (KVimg: the K image, the V image right behind it)
      ch[j].fill = 0u;
      da_fetch(ch[j], 0, Nk, 2 * C, pre[j]);
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) *(da_u4*)(KVimg + ch[j].loff) = da_land(ch[j], Nk, pre[j], -1);
  }
}

// One 32-query tile of a lane in registers: 64 features of q, dO and o as 4 chunks each (k-step ks: columns 16 ks + 8 hh) and the
// row's lse.  sra_fetch is a straight line of 13 loads from row qi (clamped by the caller: always a row of the tensor).
struct SraTile {
  da_u4 q[4], g[4], u[4];
  float lse;
};
__device__ __forceinline__ void sra_fetch(SraTile& x, const bf* qb, const bf* gb, const bf* ob, const float* lse, int qi, int C,
                                          int hh) {
  const long off = (long)qi * C + 8 * hh;
  x.lse = lse[qi];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    x.q[ks] = *(const da_u4*)(qb + off + 16 * ks);
    x.g[ks] = *(const da_u4*)(gb + off + 16 * ks);
    x.u[ks] = *(const da_u4*)(ob + off + 16 * ks);
  }
}
__device__ __forceinline__ void sra_fetch_q(da_u4 (&x)[4], const bf* qb, int qi, int C, int hh) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) x[ks] = *(const da_u4*)(qb + (long)qi * C + 8 * hh + 16 * ks);
}
__device__ __forceinline__ bf16x8 da_frag(const da_u4& r) {
  bf16x8 f;
  memcpy(&f, &r, 16);
  return f;
}

// NKB = 64-key blocks resident in LDS; DQ / DKV = which gradients this instance produces:
//   <1, true, true>   the whole backward of a (batch, head) with <= 64 keys (the 224x224 presets: 49 keys);
//   <4, true, false>  dQ over up to 256 resident keys (512x512 inputs: 256 keys under 4 096 .. 16 384 queries);
//   <1, false, true>  dK / dV of the 64-key block blockIdx.z (the same 256-key problems, one block of keys per workgroup:
//                     the softmax statistics come from the saved lse, so a block of keys needs nothing from the others).
template <int NKB, bool DQ, bool DKV>
__global__ __launch_bounds__(256, DKV ? 1 : 2) void sra_bwd_kernel(SraArgs a) {
  constexpr int KP = 72, AP = 40;                     // image pitches (elements)
  constexpr int KVIMG = NKB * 64 * KP, QIMG = 32 * KP + 64, AIMG = 32 * AP;
  constexpr int WIMG = 2 * QIMG + AIMG;               // per-wave: Q image, dO image, statistics image
  constexpr int IMG_EL = (DQ ? 2 * KVIMG : 0) + (DKV ? 4 * WIMG : 0);
  // the dK/dV reduction reuses the images: four 128 x 64 fp32 blocks side by side, one per wave, rows pitched by RP floats (one
  // workgroup per CU owns the CU's 160 KB)
  constexpr int RP = 65, RED = 128 * RP;
  constexpr int LDS_EL = DKV && 4 * RED * 2 > IMG_EL ? 4 * RED * 2 : IMG_EL;
  static_assert(LDS_EL * 2 <= 160 * 1024, "one CU's LDS");
  static_assert(NKB == 1 || !DKV, "dK / dV accumulators exist for one 64-key block");
  __shared__ __attribute__((aligned(16))) bf lds[LDS_EL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const cenet_bid bid = cenet_xcd_block();
  const int b = bid.y / a.H, h = bid.y - b * a.H;
  const int key0 = DQ ? 0 : 64 * bid.z;               // first key of this workgroup's block (dK / dV instances)
  const int C = a.C, Nq = a.Nq;
  const int Nk = DQ ? a.Nk : (a.Nk - key0 < 64 ? a.Nk - key0 : 64);  // keys this workgroup holds
  const float c = a.scale * DA_LOG2E;
  const bf* qb = a.q + (long)b * Nq * C + h * 64;
  const bf* ob = a.o + (long)b * Nq * C + h * 64;
  const bf* gb = a.dout + (long)b * Nq * C + h * 64;
  const bf* kb = a.kv + ((long)b * a.Nk + key0) * 2 * C + h * 64;
  const bf* vb = kb + C;
  bf* Kimg = lds;
  bf* Vimg = lds + KVIMG;
  bf* Qimg = lds + (DQ ? 2 * KVIMG : 0) + wave * WIMG;
  bf* Gimg = Qimg + QIMG;
  bf* Aimg = Gimg + QIMG;
  const float* lb = a.lse + ((long)b * a.H + h) * Nq;
  const int q00 = (bid.x * 4 + wave) * 32 * a.tiles;
  // tile 0's rows go first: they land with the K / V chunks behind them
  SraTile nx;
  sra_fetch(nx, qb, gb, ob, lb, q00 + r < Nq ? q00 + r : Nq - 1, C, hh);
  if (DQ) sra_stage_kv<NKB, KP>(kb, vb, Nk, C, Kimg, tid);
  // B fragments of K^T / V^T for phase B: key = 32 kt + r.  With DQ they are the rows of the resident images (da_rm(Kimg / Vimg,
  // KP, 32 kt + r, 16 ks, hh): the same 16 bytes, rows >= Nk zero there as well) and phase B reads them from LDS per tile —
  // their 64 registers hold the next tile's rows instead.  The dK/dV-only instance has no images and keeps them in registers.
  bf16x8 kfB[2][4], vfB[2][4];
  if (DKV && !DQ) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int key = 32 * kt + r;
        kfB[kt][ks] = da_ld8(kb + (long)(key < Nk ? key : 0) * 2 * C + 16 * ks + 8 * hh, key < Nk);
        vfB[kt][ks] = da_ld8(vb + (long)(key < Nk ? key : 0) * 2 * C + 16 * ks + 8 * hh, key < Nk);
      }
  }
  bf16x8 negB = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hh == 0) negB[0] = negB[1] = negB[2] = (short)0xBF80;
  f32x16 dK[2][2], dV[2][2];  // [key tile][feature tile]
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) dK[kt][dt] = dV[kt][dt] = da_zero();
  __syncthreads();
  da_loads_landed();

  for (int t = 0; t < a.tiles; ++t) {
    const int q0 = q00 + 32 * t;
    if (q0 >= Nq) break;  // (wave-uniform)
    const int qi = q0 + r < Nq ? q0 + r : Nq - 1;
    const bool qok = q0 + r < Nq;
    // ---- this tile's rows (fetched one trip ahead): B fragments for phase A, images for phase B ----
    bf16x8 qf[4], gf[4];
    float acc = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = da_frag(nx.q[ks]);
      gf[ks] = da_frag(nx.g[ks]);
      const bf16x8 uf = da_frag(nx.u[ks]);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += cenet_bf2f((unsigned short)gf[ks][j]) * cenet_bf2f((unsigned short)uf[j]);
      if (DKV) {
        bf16x8 qz = qf[ks], gz = gf[ks];
        if (!qok) qz = gz = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(Qimg + r * KP + 16 * ks + 8 * hh, &qz, 16);
        memcpy(Gimg + r * KP + 16 * ks + 8 * hh, &gz, 16);
      }
    }
    acc += __shfl_xor(acc, 32);
    const float delta = acc;
    const float lse = nx.lse;
    const float lse2 = lse * DA_LOG2E;
    // the next tile's rows, in flight across this tile's body.  Every trip fetches, the last one included (its rows are clamped
    // and nothing of it is used): under `if (more)` the registers would be carried around the branch and land behind a wait.
    sra_fetch(nx, qb, gb, ob, lb, q0 + 32 + r < Nq ? q0 + 32 + r : Nq - 1, C, hh);
    if (DKV) {  // statistics rows: lane half 0 writes lse / scale, half 1 writes delta (rows beyond Nq: lse / scale = 1e30 -> P = 0)
      unsigned short row8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      da_split3(hh == 0 ? (qok ? lse / a.scale : 1.0e30f) : (qok ? delta : 0.f), row8);
      memcpy(Aimg + r * AP + 8 * hh, row8, 16);
    }
    // ---- phase A: dQ ----
    f32x16 dq[2] = {da_zero(), da_zero()};
#pragma unroll
    for (int kt = 0; kt < (DQ ? 2 * NKB : 0); ++kt) {
      if (32 * kt >= Nk) continue;  // (uniform)
      const bf* Kt = Kimg + 32 * kt * KP;
      const bf* Vt = Vimg + 32 * kt * KP;
      f32x16 S = da_zero(), dP = da_zero();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        S = DA_MFMA(da_rm(Kt, KP, r, 16 * ks, hh), qf[ks], S);
        dP = DA_MFMA(da_rm(Vt, KP, r, 16 * ks, hh), gf[ks], dP);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float pv = da_exp2(S[i] * c - lse2);
        if (32 * kt + da_row(i, hh) >= Nk) pv = 0.f;
        S[i] = pv * (dP[i] - delta);
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) dq[dt] = DA_MFMA(da_tr(Kt, KP, s2, 32 * dt, lane), da_pack8(S, s2), dq[dt]);
    }
    if (DQ && qok) {
      bf* dp = a.dq + ((long)b * Nq + qi) * C + h * 64;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float o4[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) o4[i] = dq[dt][4 * g + i] * a.scale;
          st4v(dp + 32 * dt + 8 * g + 4 * hh, o4);
        }
    }
    if (!DKV) continue;
    // ---- phase B: dK, dV (images written above by this wave only: no workgroup barrier needed) ----
    // A wave's LDS instructions execute in program order, so its own stores above are visible to its loads below; the
    // compiler is told not to move LDS accesses across this point (the host checker runs lanes as fibers: its sync point).
    da_wave_sync();
    bf16x8 al = {0, 0, 0, 0, 0, 0, 0, 0}, ad = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hh == 0) {
      memcpy(&al, Aimg + r * AP, 16);
      memcpy(&ad, Aimg + r * AP + 8, 16);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if (32 * kt >= Nk) continue;
      f32x16 S = da_zero(), dP = da_zero();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        S = DA_MFMA(da_rm(Qimg, KP, r, 16 * ks, hh), DQ ? da_rm(Kimg, KP, 32 * kt + r, 16 * ks, hh) : kfB[kt][ks], S);    // S[query][key]
        dP = DA_MFMA(da_rm(Gimg, KP, r, 16 * ks, hh), DQ ? da_rm(Vimg, KP, 32 * kt + r, 16 * ks, hh) : vfB[kt][ks], dP);  // dP[query][key]
      }
      S = DA_MFMA(al, negB, S);
      dP = DA_MFMA(ad, negB, dP);
      const bool kok = 32 * kt + r < Nk;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float pv = kok ? da_exp2(S[i] * c) : 0.f;
        S[i] = pv;
        dP[i] = pv * dP[i];
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pB = da_pack8(S, s2), dsB = da_pack8(dP, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dV[kt][dt] = DA_MFMA(da_tr(Gimg, KP, s2, 32 * dt, lane), pB, dV[kt][dt]);
          dK[kt][dt] = DA_MFMA(da_tr(Qimg, KP, s2, 32 * dt, lane), dsB, dK[kt][dt]);
        }
      }
    }
  }
  if (!DKV) return;
  // ---- the four waves meet in LDS: red[key][0..63] = dK (unscaled), red[key][64..127] = dV ----
  // Each wave writes its block red[wave][feature 0..127][key 0..63], all four at once (rows pitched by RP = 65 floats: a
  // wave's 32 keys of one feature and, below, a wave's 64 features of one key both fall into distinct banks); then every
  // thread adds the four values of its elements in the order wave 0, 1, 2, 3 — the order in which the waves used to take
  // turns at one block, so the sum is the same float.
  float* red = (float*)lds;
  __syncthreads();  // every wave is done with the images
  {
    float* mine = red + wave * RED;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = 32 * kt + r, f = 32 * dt + da_row(i, hh);
          mine[f * RP + key] = dK[kt][dt][i];
          mine[(64 + f) * RP + key] = dV[kt][dt][i];
        }
  }
  __syncthreads();
  if (a.dkv_bf) {  // this workgroup saw every query of its (batch, head)
    bf* dkvb = a.dkv_bf + ((long)b * a.Nk + key0) * 2 * C + h * 64;
    for (int i = tid; i < Nk * 128; i += 256) {
      const int key = i >> 7, f = i & 127;
      const float* e = red + f * RP + key;
      const float v = ((e[0] + e[RED]) + e[2 * RED]) + e[3 * RED];
      if (f < 64) stf(dkvb + (long)key * 2 * C + f, v * a.scale);
      else stf(dkvb + (long)key * 2 * C + C + (f - 64), v);
    }
    return;
  }
  float* dkv = a.dkv + ((long)b * a.Nk + key0) * 2 * C + h * 64;
  for (int i = tid; i < Nk * 128; i += 256) {
    const int key = i >> 7, f = i & 127;  // 128 consecutive lanes = one key's 64 + 64 features: contiguous runs of 256 B
    const float* e = red + f * RP + key;
    const float v = ((e[0] + e[RED]) + e[2 * RED]) + e[3 * RED];
    if (f < 64) atomicAdd(&dkv[(long)key * 2 * C + f], v * a.scale);
    else atomicAdd(&dkv[(long)key * 2 * C + C + (f - 64)], v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Spatial-reduction attention FORWARD with the key / value set resident (same problem class as sra_bwd_kernel: head dimension
// 64, at most 64 keys): no key loop and no online softmax — a wave takes 32-query tiles, S^T = K Q^T for both key tiles in one
// go, the softmax over the <= 64 keys of a query is 32 registers + one exchange with lane ^ 32, and O^T = V^T P^T.  The streamed
// kernel (attn_bf16.hip, flashc_fwd) spent ~20 us per launch on 13-26 MB; this one is bound by reading q and writing o.
// q, o [B, Nq, 64 H]; kv [B, Nk, 128 H]; lse [B, H, Nq] = natural log of the sum of exp(scale * scores) (what the backward
// kernels expect).
// ---------------------------------------------------------------------------------------------------------------------------
struct SraFwdArgs {
  const bf *q, *kv;
  bf* o;
  float* lse;
  int B, H, Nq, Nk, C, tiles;
  float scale;
};

__global__ __launch_bounds__(256, 2) void sra_fwd_kernel(SraFwdArgs a) {
  constexpr int KP = 72, KVIMG = 64 * KP;
  __shared__ __attribute__((aligned(16))) bf lds[2 * KVIMG + 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const cenet_bid bid = cenet_xcd_block();
  const int b = bid.y / a.H, h = bid.y - b * a.H;
  const int C = a.C, Nq = a.Nq, Nk = a.Nk;
  const float c = a.scale * DA_LOG2E;
  const bf* qb = a.q + (long)b * Nq * C + h * 64;
  bf* ob = a.o + (long)b * Nq * C + h * 64;
  const bf* kb = a.kv + (long)b * Nk * 2 * C + h * 64;
  const bf* vb = kb + C;
  bf* Kimg = lds;
  bf* Vimg = lds + KVIMG;
  const int q00 = (bid.x * 4 + wave) * 32 * a.tiles;
  // the rows of a tile are fetched one trip ahead (tile 0: in front of the K / V chunks, landing with them), on every trip
  da_u4 nx[4];
  sra_fetch_q(nx, qb, q00 + r < Nq ? q00 + r : Nq - 1, C, hh);
  sra_stage_kv<1, KP>(kb, vb, Nk, C, Kimg, tid);
  __syncthreads();
  da_loads_landed();
  for (int t = 0; t < a.tiles; ++t) {
    const int q0 = q00 + 32 * t;
    if (q0 >= Nq) break;  // (wave-uniform)
    const int qi = q0 + r < Nq ? q0 + r : Nq - 1;
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = da_frag(nx[ks]);
    sra_fetch_q(nx, qb, q0 + 32 + r < Nq ? q0 + 32 + r : Nq - 1, C, hh);
    f32x16 S[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      S[kt] = da_zero();
      if (32 * kt < Nk) {  // (uniform)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) S[kt] = DA_MFMA(da_rm(Kimg + 32 * kt * KP, KP, r, 16 * ks, hh), qf[ks], S[kt]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (32 * kt + da_row(i, hh) >= Nk) S[kt][i] = DA_NEG;
    }
    float mx = DA_NEG;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, S[kt][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mc = mx * c;
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float pv = da_exp2(S[kt][i] * c - mc);  // masked keys: exp2(-huge) = 0
        S[kt][i] = pv;
        l += pv;
      }
    l += __shfl_xor(l, 32);
    f32x16 O[2] = {da_zero(), da_zero()};
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if (32 * kt >= Nk) continue;
      const bf* Vt = Vimg + 32 * kt * KP;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pB = da_pack8(S[kt], s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) O[dt] = DA_MFMA(da_tr(Vt, KP, s2, 32 * dt, lane), pB, O[dt]);
      }
    }
    if (q0 + r < Nq) {
      const float inv = 1.f / l;
      bf* op = ob + (long)qi * C;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float o4[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) o4[i] = O[dt][4 * g + i] * inv;
          st4v(op + 32 * dt + 8 * g + 4 * hh, o4);
        }
      if (hh == 0) a.lse[((long)b * a.H + h) * Nq + qi] = mx * a.scale + logf(l);
    }
  }
}

extern "C" int cenet_sra_attn_fwd_bf16(const bf* q, const bf* kv, bf* o, float* lse, int B, int H, int Nq, int Nk, float scale,
                                       hipStream_t stream) {
  if (!q || !kv || !o || !lse || B <= 0 || H <= 0 || Nq <= 0) return CENET_EINVAL;
  if (!(Nk >= 1 && Nk <= 64)) return CENET_EUNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)o) & 15) != 0) return CENET_EINVAL;
  SraFwdArgs a;
  a.q = q; a.kv = kv; a.o = o; a.lse = lse; a.B = B; a.H = H; a.Nq = Nq; a.Nk = Nk; a.C = 64 * H; a.scale = scale;
  // two workgroups per CU: ~512 workgroups fill the chip once
  int tiles = 1;
  while (tiles < 8 && (long)cdiv(Nq, 128 * tiles) * B * H > 1024) ++tiles;
  a.tiles = tiles;
  CENET_LAUNCH(sra_fwd_kernel, dim3(cdiv(Nq, 128 * a.tiles), B * H), dim3(256), stream, a);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_sra_attn_bwd_supported(int hd, int Nk) { return hd == 64 && Nk >= 1 && Nk <= 64; }
// 64 < Nk <= 256 (the 512x512 presets: 256 keys): cenet_sra_attn_bwd_bf16 runs as two launches, dQ over all keys resident in
// LDS and dK / dV per 64-key block; the forward of these problems is the tiled kernel's (same lse convention)
extern "C" int cenet_sra_attn_bwd_blocks_supported(int hd, int Nk) { return hd == 64 && Nk > 64 && Nk <= 256; }

// 32-query tiles per wave: the kernel runs one workgroup per CU (484 registers), so more than 256 workgroups is a second
// round; measured best (B = 32) when a tile cost five serial memory round trips: 4 tiles at 3136 queries (42 us), 2 at 784 / 196
// (31 us), 1 at 49 (25 us).  With a tile's rows fetched one trip ahead the same launches take 27 / 19 / 13 us (DESIGN.md section 6,
// round 10); the rule was not retuned.
static int sra_tiles(int B, int H, int Nq) {
  int tiles = 1;
  while (tiles < 8 && (long)cdiv(Nq, 128 * tiles) * B * H > 256) ++tiles;
  return tiles;
}
extern "C" int cenet_sra_attn_bwd_tiles(int B, int H, int Nq) { return B > 0 && H > 0 && Nq > 0 ? sra_tiles(B, H, Nq) : 0; }
// 1 when the launch for this problem puts every query of a (batch, head) in ONE workgroup: dK/dV then need no cross-workgroup
// sum and cenet_sra_attn_bwd_direct_bf16 stores them as bf16 (the 14x14 and 7x7 stages of the ACDC preset)
extern "C" int cenet_sra_attn_bwd_direct_supported(int B, int H, int Nq, int Nk) {
  return cenet_sra_attn_bwd_supported(64, Nk) && B > 0 && H > 0 && Nq > 0 && cdiv(Nq, 128 * sra_tiles(B, H, Nq)) == 1;
}

static int sra_bwd_launch(const bf* q, const bf* kv, const bf* o, const bf* dout, const float* lse, bf* dq, float* dkv, bf* dkv_bf,
                          int B, int H, int Nq, int Nk, float scale, hipStream_t stream) {
  if (!q || !kv || !o || !dout || !lse || !dq || (!dkv && !dkv_bf) || B <= 0 || H <= 0 || Nq <= 0) return CENET_EINVAL;
  const bool blocks = cenet_sra_attn_bwd_blocks_supported(64, Nk);
  if (!cenet_sra_attn_bwd_supported(64, Nk) && !blocks) return CENET_EUNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)o | (uintptr_t)dout | (uintptr_t)dq) & 15) != 0) return CENET_EINVAL;
  SraArgs a;
  a.q = q; a.kv = kv; a.o = o; a.dout = dout; a.lse = lse; a.dq = dq; a.dkv = dkv; a.dkv_bf = dkv_bf;
  a.B = B; a.H = H; a.Nq = Nq; a.Nk = Nk; a.C = 64 * H; a.scale = scale;
  a.tiles = sra_tiles(B, H, Nq);
  if (blocks) {
    if (dkv_bf) return CENET_EUNSUPPORTED;  // dK / dV of a key block are summed over the query slices: fp32 accumulator
    // dQ: two workgroups per CU (no dK / dV accumulators), ~512 workgroups fill the chip once
    int tq = 1;
    while (tq < 8 && (long)cdiv(Nq, 128 * tq) * B * H > 512) ++tq;
    a.tiles = tq;
    CENET_LAUNCH((sra_bwd_kernel<4, true, false>), dim3(cdiv(Nq, 128 * tq), B * H), dim3(256), stream, a);
    const int nkb = cdiv(Nk, 64);
    int tk = 1;
    while (tk < 16 && (long)cdiv(Nq, 128 * tk) * B * H * nkb > 256) ++tk;
    a.tiles = tk;
    CENET_LAUNCH((sra_bwd_kernel<1, false, true>), dim3(cdiv(Nq, 128 * tk), B * H, nkb), dim3(256), stream, a);
    CENET_CHECK_LAUNCH();
    return CENET_OK;
  }
  if (dkv_bf && cdiv(Nq, 128 * a.tiles) != 1) return CENET_EUNSUPPORTED;
  CENET_LAUNCH((sra_bwd_kernel<1, true, true>), dim3(cdiv(Nq, 128 * a.tiles), B * H), dim3(256), stream, a);
  CENET_CHECK_LAUNCH();
  return CENET_OK;
}

extern "C" int cenet_sra_attn_bwd_bf16(const bf* q, const bf* kv, const bf* o, const bf* dout, const float* lse, bf* dq, float* dkv,
                                       int B, int H, int Nq, int Nk, float scale, hipStream_t stream) {
  if (!dkv) return CENET_EINVAL;
  return sra_bwd_launch(q, kv, o, dout, lse, dq, dkv, nullptr, B, H, Nq, Nk, scale, stream);
}

extern "C" int cenet_sra_attn_bwd_direct_bf16(const bf* q, const bf* kv, const bf* o, const bf* dout, const float* lse, bf* dq,
                                              bf* dkv, int B, int H, int Nq, int Nk, float scale, hipStream_t stream) {
  if (!dkv) return CENET_EINVAL;
  return sra_bwd_launch(q, kv, o, dout, lse, dq, nullptr, dkv, B, H, Nq, Nk, scale, stream);
}
