// augment_ops.h — device helpers shared by augment_ops.hip (one-channel slices, the Synapse pipeline) and augment_image_ops.hip
// (multi-channel images, the skin pipeline): the counter-based generator, the stage limits and the tap order of
// scipy's symmetric correlate1d.  spline3.h turns fp contraction off for the translation unit that includes this header.
#pragma once
#include "common.h"
#include "spline3.h"  // aug_mirror; fp contraction off from here on

#define AOP_MAX_STAGES 8
#define AOP_DP 32      // doubles per (sample, stage)
#define AOP_MAX_RADIUS 16
#define AOP_TH 8
#define AOP_TW 32

// Philox4x32-10 (Salmon et al., SC'11; Random123): ten rounds, the key bumped by the Weyl constants between them
__host__ __device__ __forceinline__ void aop_philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (unsigned)p1;
    c[2] = n2;
    c[3] = (unsigned)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// one line of scipy's correlate1d with a symmetric kernel: centre first, then the pairs from the outermost inwards
#define AOP_SYMMETRIC_TAPS(AT)                                                  \
  double acc = (AT(0)) * w[0];                                                  \
  for (int ii = radius; ii > 0; --ii) acc += ((AT(-ii)) + (AT(ii))) * w[ii];
