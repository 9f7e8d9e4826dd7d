// spline3.h — scipy.ndimage's order-3 spline arithmetic as device functions, shared by augment.hip (training-time augmentation) and
// volresize.hip (test-time volume resize).  Everything is fp64 in scipy's own operation order and WITHOUT fused multiply-adds: the
// pragma below holds for the rest of the translation unit that includes this header, which both users rely on.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

#define AUG_POLE (-0.26794919243112270647)  // sqrt(3) - 2

// one line of scipy's spline_filter1d(order=3), mirror boundary: c[0 .. n) at stride s, zn = pole^(n-1)
__device__ __forceinline__ void aug_prefilter_line(double* c, int n, long s, double zn) {
  if (n < 2) return;
  const double z = AUG_POLE;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  for (int i = 0; i < n; ++i) c[i * s] *= gain;
  double zi = z;
  double c0 = c[0] + zn * c[(n - 1) * s];
  for (int i = 1; i < n - 1; ++i) {
    c0 += (zi + zn * zn / zi) * c[i * s];
    zi *= z;
  }
  c[0] = c0 / (1.0 - zn * zn);
  for (int i = 1; i < n; ++i) c[i * s] += z * c[(i - 1) * s];
  c[(n - 1) * s] = (z * c[(n - 2) * s] + c[(n - 1) * s]) * z / (z * z - 1.0);
  for (int i = n - 2; i >= 0; --i) c[i * s] = z * (c[(i + 1) * s] - c[i * s]);
}

__device__ __forceinline__ void aug_w3(double t, double* w) {  // cubic B-spline weights of the taps floor - 1 .. floor + 2
  w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
  const double z = 1.0 - t;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[0] = z * z * z / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
}
__device__ __forceinline__ int aug_mirror(int idx, int n) {  // scipy NI_ZoomShift tap mapping (all non-grid modes)
  if (n <= 1) return 0;
  const int s2 = 2 * n - 2;
  if (idx < 0) {
    idx = s2 * (-idx / s2) + idx;
    idx = idx <= 1 - n ? idx + s2 : -idx;
  } else if (idx >= n) {
    idx -= s2 * (idx / s2);
    if (idx >= n) idx = s2 - idx;
  }
  return idx;
}

// the order-3 sample of the prefiltered image c [Ha, Wa] at (cy, cx), 0 <= cy <= Ha - 1 and 0 <= cx <= Wa - 1: 4 x 4 mirrored
// taps, rows outer, accumulated in scipy's order
__device__ __forceinline__ double aug_cubic_at(const double* __restrict__ c, int Ha, int Wa, double cy, double cx) {
  const int fy = (int)floor(cy), fx = (int)floor(cx);
  double wy[4], wx[4];
  aug_w3(cy - (double)fy, wy);
  aug_w3(cx - (double)fx, wx);
  int yy[4], xx[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    yy[a] = aug_mirror(fy - 1 + a, Ha);
    xx[a] = aug_mirror(fx - 1 + a, Wa);
  }
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += c[(long)yy[a] * Wa + xx[e]] * wy[a] * wx[e];
  return acc;
}
