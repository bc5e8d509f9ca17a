// Helpers shared by the kernels that PRODUCE an activation gradient `da` and take the BatchNorm-backward sums of the block
// it feeds on the way (elementwise.hip: crimac_unpool_add, crimac_head_bwd; meta.hip: crimac_head_meta_bwd), and the
// pixel-index split of the NCHW logits.
#pragma once
#include "common.h"

namespace {

// pixel index -> (image, pixel in image); 32-bit divide when the operands fit (a 64-bit divide is ~4x the
// instructions, noticeable in the one-pixel-per-thread kernels)
__device__ __forceinline__ void pix_split(long p, long HW, long& b, long& hw) {
  if (((p | HW) >> 31) == 0) {
    const unsigned q = (unsigned)p / (unsigned)HW;
    b = q;
    hw = (unsigned)p - q * (unsigned)HW;
  } else {
    b = p / HW;
    hw = p % HW;
  }
}

// Fused BatchNorm+ReLU backward sums (== bn_bwd_reduce on the tensor a kernel has just produced): the
// producer keeps sum dz / sum dz*xhat of its thread-fixed 8-channel chunk in registers while it still
// holds `da`; at the end they go through LDS into one of `replicas` fp64 accumulators [replicas][C].
struct BnbArgs {
  const void* y;          // saved conv output of the BatchNorm layer `da` feeds, [pixels][y_ld]
  long y_ld;
  const float* vec;       // rows mean, invstd, scale, shift; row stride `stride`
  long stride;
  double* sum_dz;
  double* sum_dzx;
  int replicas;
};
struct BnbConst { float sc[8], sh[8], mu[8], is[8]; };
__device__ __forceinline__ void bnb_load(const BnbArgs& a, int c0, BnbConst& k) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k.mu[j] = a.vec[c0 + j];
    k.is[j] = a.vec[a.stride + c0 + j];
    k.sc[j] = a.vec[2 * a.stride + c0 + j];
    k.sh[j] = a.vec[3 * a.stride + c0 + j];
  }
}
template <typename T>
__device__ __forceinline__ void bnb_accum(const BnbArgs& a, const BnbConst& k, long pix, int c0, const float (&g)[8],
                                          float (&d1)[8], float (&d2)[8]) {
  float yv[8];
  load8(reinterpret_cast<const T*>(a.y) + pix * a.y_ld + c0, yv);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float dz = (yv[j] * k.sc[j] + k.sh[j]) > 0.f ? g[j] : 0.f;
    d1[j] += dz;
    d2[j] += dz * (yv[j] - k.mu[j]) * k.is[j];
  }
}
// same with y already in registers
__device__ __forceinline__ void bnb_accum_v(const BnbConst& k, const float (&yv)[8], const float (&g)[8],
                                            float (&d1)[8], float (&d2)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float dz = (yv[j] * k.sc[j] + k.sh[j]) > 0.f ? g[j] : 0.f;
    d1[j] += dz;
    d2[j] += dz * (yv[j] - k.mu[j]) * k.is[j];
  }
}
// lds: [2][C] floats, zeroed and synchronised by the caller; every thread of the block calls this
__device__ __forceinline__ void bnb_flush(const BnbArgs& a, float* lds, int C, int c0, const float (&d1)[8],
                                          const float (&d2)[8], int nthreads) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    atomicAdd(&lds[c0 + j], d1[j]);
    atomicAdd(&lds[C + c0 + j], d2[j]);
  }
  __syncthreads();
  const long rep = (long)(blockIdx.x % (unsigned)a.replicas) * C;
  for (int c = threadIdx.x; c < C; c += nthreads) {
    atomicAdd(&a.sum_dz[rep + c], (double)lds[c]);
    atomicAdd(&a.sum_dzx[rep + c], (double)lds[C + c]);
  }
}

inline bool bnb_args_ok(const void* y, long y_ld, const float* vec, long stride, double* s0, double* s1, int replicas,
                        int C) {
  if (!s0) return true;                      // no fused reduction requested
  return y && vec && s1 && y_ld >= C && y_ld % 8 == 0 && stride >= C && replicas >= 1;
}

}  // namespace
