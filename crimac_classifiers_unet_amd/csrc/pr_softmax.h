// The per-pixel softmax of the evaluation kernels, in ONE place: crimac_pr_histogram_classes (tiling.hip) bins the float16
// bit pattern of these probabilities and crimac_integrate_confusion (integrate.hip) thresholds / weights by the same
// float16 values, so a threshold read off the PR curve selects exactly the pixels the histogram counted.  The arithmetic
// is that of pr_histogram_kernel: the maximum by fmaxf in class order, expf of the differences, their sum in class order,
// one fp32 division per class, one round-to-nearest-even conversion to float16 (numpy's .astype(float16)).
#pragma once
#include "common.h"

// z[o] = expf(logit_o - max), den = their sum; px points at the pixel in class plane 0, `plane` elements separate the
// class planes (NCHW: H * W).  ncls <= 8; z[ncls ..] is not written.
__device__ __forceinline__ void pr_softmax_terms(const float* __restrict__ px, long plane, int ncls, float (&z)[8],
                                                 float& den) {
  float mx = -INFINITY;
  den = 0.f;
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < ncls) { z[o] = px[o * plane]; mx = fmaxf(mx, z[o]); }
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < ncls) { z[o] = expf(z[o] - mx); den += z[o]; }
}

// softmax[c] as the evaluation stores it: float16
__device__ __forceinline__ half_t pr_prob_f16(float zc, float den) { return (half_t)(zc / den); }
