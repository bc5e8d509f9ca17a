// Decoder up-sampling of up_mode="upsample" (reference unet.py:47-56): nn.Upsample(bilinear, x2, align_corners=False)
// followed by conv1x1(cin, cout), on CDNA4 (gfx950), NHWC.
//
// Bilinear 2x gives every fine pixel a convex combination of at most 4 coarse pixels (weights 9/16, 3/16, 3/16, 1/16;
// clamped at the borders, the weights of a fine pixel always sum to 1), so it commutes with a 1x1 convolution plus
// bias:  conv1x1(up(x)) == up(conv1x1(x)).  Every contraction therefore runs on the COARSE grid, at a quarter of the
// reference's FLOPs, and only the cout-channel result is interpolated:
//   forward  z = W x + b (coarse GEMM, crimac_igemm_conv ntaps 1), y = up(z) into the up half of the concat buffer
//   backward dz = up^T(dy) (the adjoint: fine -> coarse, fp32 accumulation), dx = W^T dz, dW = dz^T x,
//            db = sum dz = sum dy (the adjoint preserves sums: the column sums the caller already takes)
// Storage (the `prec` argument): the 16-bit modes keep z / dz in their 16-bit type; the fp32-storage modes in fp32;
// CRIMAC_PREC_H3P reads plane-pair activations / output gradients (hp_t), keeps z and dz in fp32 and runs the two GEMMs
// on the F32H3 split (fp16 hi + lo of the fp32 operand, the arithmetic of the plane-pair contractions), so its weight
// planes are the F32H3 ones (crimac_pack_layers, kind 2).
#include "common.h"

namespace {

// PyTorch's source coordinate of fine index d (scale 2, align_corners=False): i0, i1 = min(i0 + 1, n - 1), weight l1 on
// i1 (area_pixel_compute_source_index, clamped at 0)
__device__ __forceinline__ void src_index(int d, int n, int& i0, int& i1, float& l1) {
  float s = 0.5f * ((float)d + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  l1 = s - (float)i0;
}

// weight of coarse index c in the interpolation of fine index d
__device__ __forceinline__ float up_weight(int d, int n, int c) {
  int i0, i1;
  float l1;
  src_index(d, n, i0, i1, l1);
  return (i0 == c ? 1.f - l1 : 0.f) + (i1 == c ? l1 : 0.f);
}

// y[b][fy][fx][c] = bilinear-2x of z [B][H][W][C] (z_ld), one thread per (fine pixel, 8 channels)
template <typename TZ, typename TO>
__global__ __launch_bounds__(256) void up2x_kernel(const TZ* __restrict__ z, long z_ld, int B, int H, int W, int C,
                                                   TO* __restrict__ out, long out_ld) {
  const int c8n = C / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)B * 4 * H * W * c8n;
  if (idx >= total) return;
  const int c = (int)(idx % c8n) * 8;
  const long pix = idx / c8n;
  const int fx = (int)(pix % (2 * W));
  const long t = pix / (2 * W);
  const int fy = (int)(t % (2 * H));
  const long b = t / (2 * H);
  int y0, y1, x0, x1;
  float ly, lx;
  src_index(fy, H, y0, y1, ly);
  src_index(fx, W, x0, x1, lx);
  const long base = b * H * W;
  float v00[8], v01[8], v10[8], v11[8], o[8];
  load8(z + (base + (long)y0 * W + x0) * z_ld + c, v00);
  load8(z + (base + (long)y0 * W + x1) * z_ld + c, v01);
  load8(z + (base + (long)y1 * W + x0) * z_ld + c, v10);
  load8(z + (base + (long)y1 * W + x1) * z_ld + c, v11);
  const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = hy * (hx * v00[i] + lx * v01[i]) + ly * (hx * v10[i] + lx * v11[i]);
  store8(out + pix * out_ld + c, o);
}

// dz[b][y][x][c] = sum over the (at most 4 x 4) fine pixels whose interpolation reads coarse (y, x), one thread per
// (coarse pixel, 8 channels); fp32 accumulation
template <typename TD, typename TZ>
__global__ __launch_bounds__(256) void up2x_adjoint_kernel(const TD* __restrict__ dy, long dy_ld, int B, int H, int W,
                                                           int C, TZ* __restrict__ dz, long dz_ld) {
  const int c8n = C / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)B * H * W * c8n;
  if (idx >= total) return;
  const int c = (int)(idx % c8n) * 8;
  const long pix = idx / c8n;
  const int x = (int)(pix % W);
  const long t = pix / W;
  const int y = (int)(t % H);
  const long b = t / H;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int Hf = 2 * H, Wf = 2 * W;
  for (int fy = 2 * y - 1; fy <= 2 * y + 2; ++fy) {
    if (fy < 0 || fy >= Hf) continue;
    const float wy = up_weight(fy, H, y);
    if (wy == 0.f) continue;
    for (int fx = 2 * x - 1; fx <= 2 * x + 2; ++fx) {
      if (fx < 0 || fx >= Wf) continue;
      const float wx = up_weight(fx, W, x);
      if (wx == 0.f) continue;
      float v[8];
      load8(dy + ((b * Hf + fy) * (long)Wf + fx) * dy_ld + c, v);
      const float w = wy * wx;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += w * v[i];
    }
  }
  store8(dz + pix * dz_ld + c, acc);
}

// plane-pair activations -> fp32 (the F32H3 GEMM splits them again, bit for bit: hi + lo is exact in fp32)
__global__ __launch_bounds__(256) void hp_to_f32_kernel(const hp_t* __restrict__ x, long x_ld, long M, int C,
                                                        float* __restrict__ out) {
  const int c8n = C / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * c8n) return;
  const int c = (int)(idx % c8n) * 8;
  const long p = idx / c8n;
  float v[8];
  load8(x + p * x_ld + c, v);
  store8(out + p * C + c, v);
}

// dw[f][s] += sum_p F[p][f] * S[p][s] on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation, for every
// storage type).  A workgroup owns a 64 x 64 (f, s) tile and one pixel range; 4 waves, a 32 x 32 quarter each.  The
// two operand slabs [WK pixels][64 channels] go through LDS as fp32; lane l of the MFMA reads A[f = l & 31][p = l >> 5]
// and B[p = l >> 5][s = l & 31], i.e. rows of the slabs as stored -- no transpose.  The tile is added to dw with fp32
// atomics at the end.
constexpr int WK = 32;             // pixels per LDS slab
constexpr int WPITCH = 64 + 4;     // floats per slab row

template <typename TF, typename TS>
__global__ __launch_bounds__(256) void wgrad1x1_kernel(const TF* __restrict__ f, long f_ld, int CF,
                                                       const TS* __restrict__ s, long s_ld, int CS, long M,
                                                       long pix_per_split, float* __restrict__ dw) {
  __shared__ float sf[WK][WPITCH];
  __shared__ float ss[WK][WPITCH];
  const int tiles_s = CS / 64;
  const int tile = blockIdx.x % ((CF / 64) * tiles_s);
  const long split = blockIdx.x / ((CF / 64) * tiles_s);
  const int f0 = (tile / tiles_s) * 64, s0 = (tile % tiles_s) * 64;
  const long p_begin = split * pix_per_split;
  const long p_end = p_begin + pix_per_split < M ? p_begin + pix_per_split : M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int ld_row = tid >> 3, ld_c = (tid & 7) * 8;      // staging: 32 rows x 8 groups of 8 channels
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (long p0 = p_begin; p0 < p_end; p0 += WK) {
    const long p = p0 + ld_row;
    float vf[8], vs[8];
    if (p < p_end) {
      load8(f + p * f_ld + f0 + ld_c, vf);
      load8(s + p * s_ld + s0 + ld_c, vs);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) vf[i] = vs[i] = 0.f;
    }
    __syncthreads();                 // (the previous slab has been read)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sf[ld_row][ld_c + i] = vf[i];
      ss[ld_row][ld_c + i] = vs[i];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < WK; k += 2) {
      const float a = sf[k + (lane >> 5)][wr * 32 + (lane & 31)];
      const float b = ss[k + (lane >> 5)][wc * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  }
  const int col = s0 + wc * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = f0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    atomicAdd(dw + (long)row * CS + col, acc[r]);
  }
}

template <typename TF, typename TS>
int launch_wgrad1x1(const void* f, long f_ld, int CF, const void* s, long s_ld, int CS, long M, float* dw,
                    hipStream_t st) {
  const int tiles = (CF / 64) * (CS / 64);
  // about four resident rounds of workgroups over the chip, but at least 512 pixels per split (one atomic pass each)
  long splits = (4L * crimac_cu_count() + tiles - 1) / tiles;
  const long max_splits = (M + 511) / 512;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  long per = (M + splits - 1) / splits;
  per = (per + WK - 1) / WK * WK;
  splits = (M + per - 1) / per;
  hipLaunchKernelGGL((wgrad1x1_kernel<TF, TS>), dim3((unsigned)(tiles * splits)), dim3(256), 0, st,
                     reinterpret_cast<const TF*>(f), f_ld, CF, reinterpret_cast<const TS*>(s), s_ld, CS, M, per, dw);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

inline unsigned grid_of(long threads) { return (unsigned)((threads + 255) / 256); }

// precisions of the entry points: every storage mode; the backward-only ones not F32H3 (its backward pass is called
// with F32X3, crimac_unet_hip.h) and none of them H3F_BWD
bool prec_ok(int prec, bool backward) {
  return prec >= CRIMAC_PREC_BF16 && prec <= CRIMAC_PREC_H3P && !(backward && prec == CRIMAC_PREC_F32H3);
}

}  // namespace

extern "C" int crimac_conv1x1_up2x(int prec, const void* x, long x_ld, int B, int H, int W, int Cin, int Cout,
                                   const void* w_hi, const void* w_lo, const float* bias, void* work, void* out,
                                   long out_ld, void* stream) {
  CRIMAC_REQUIRE(prec_ok(prec, false), "conv1x1_up2x: bad precision %d", prec);
  CRIMAC_REQUIRE(B > 0 && H > 0 && W > 0, "conv1x1_up2x: bad grid");
  CRIMAC_REQUIRE(Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0,
                 "conv1x1_up2x: Cin=%d and Cout=%d must be positive multiples of 64", Cin, Cout);
  CRIMAC_REQUIRE(x_ld >= Cin && x_ld % 8 == 0 && out_ld >= Cout && out_ld % 8 == 0,
                 "conv1x1_up2x: x_ld / out_ld must cover the channels and be multiples of 8");
  CRIMAC_REQUIRE(x && w_hi && work && out, "conv1x1_up2x: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const long M = (long)B * H * W;
  const long fine = 4 * M * (Cout / 8);
  if (prec == CRIMAC_PREC_H3P) {
    float* z = reinterpret_cast<float*>(work);
    float* x32 = z + M * Cout;
    hipLaunchKernelGGL(hp_to_f32_kernel, dim3(grid_of(M * (Cin / 8))), dim3(256), 0, st,
                       reinterpret_cast<const hp_t*>(x), x_ld, M, Cin, x32);
    CRIMAC_LAUNCH_CHECK();
    const int rc = crimac_igemm_conv(CRIMAC_PREC_F32H3, x32, Cin, B, H, W, H, W, Cin, Cout, 1, 1, 0, 1, w_hi, w_lo,
                                     bias, Cout, z, Cout, 0, 0, 0, stream);
    if (rc != CRIMAC_OK) return rc;
    hipLaunchKernelGGL((up2x_kernel<float, hp_t>), dim3(grid_of(fine)), dim3(256), 0, st, z, (long)Cout, B, H, W,
                       Cout, reinterpret_cast<hp_t*>(out), out_ld);
    CRIMAC_LAUNCH_CHECK();
    return CRIMAC_OK;
  }
  const int rc = crimac_igemm_conv(prec, x, x_ld, B, H, W, H, W, Cin, Cout, 1, 1, 0, 1, w_hi, w_lo, bias, Cout, work,
                                   Cout, 0, 0, 0, stream);
  if (rc != CRIMAC_OK) return rc;
  CRIMAC_FOR_STORAGE(prec, T, {
    hipLaunchKernelGGL((up2x_kernel<T, T>), dim3(grid_of(fine)), dim3(256), 0, st,
                       reinterpret_cast<const T*>(work), (long)Cout, B, H, W, Cout, reinterpret_cast<T*>(out), out_ld);
  });
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_up2x_adjoint(int prec, const void* dy, long dy_ld, int B, int H, int W, int C, void* dz,
                                   long dz_ld, void* stream) {
  CRIMAC_REQUIRE(prec_ok(prec, true), "up2x_adjoint: bad precision %d", prec);
  CRIMAC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "up2x_adjoint: bad shape");
  CRIMAC_REQUIRE(dy_ld >= C && dy_ld % 8 == 0 && dz_ld >= C && dz_ld % 8 == 0,
                 "up2x_adjoint: dy_ld / dz_ld must cover the channels and be multiples of 8");
  CRIMAC_REQUIRE(dy && dz, "up2x_adjoint: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const long threads = (long)B * H * W * (C / 8);
  CRIMAC_FOR_STORAGE2(prec, TF, TP, {
    hipLaunchKernelGGL((up2x_adjoint_kernel<TP, TF>), dim3(grid_of(threads)), dim3(256), 0, st,
                       reinterpret_cast<const TP*>(dy), dy_ld, B, H, W, C, reinterpret_cast<TF*>(dz), dz_ld);
  });
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_conv1x1_dgrad(int prec, const void* dz, long dz_ld, int B, int H, int W, int Cout, int Cin,
                                    const void* w_dg_hi, const void* w_dg_lo, void* dx, long dx_ld, void* stream) {
  CRIMAC_REQUIRE(prec_ok(prec, true), "conv1x1_dgrad: bad precision %d", prec);
  CRIMAC_REQUIRE(Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0,
                 "conv1x1_dgrad: Cin=%d and Cout=%d must be positive multiples of 64", Cin, Cout);
  // H3P: dz is fp32 (crimac_up2x_adjoint), the contraction runs on the F32H3 split with the F32H3 planes of kind 2
  return crimac_igemm_conv(prec == CRIMAC_PREC_H3P ? CRIMAC_PREC_F32H3 : prec, dz, dz_ld, B, H, W, H, W, Cout, Cin,
                           1, 1, 0, 1, w_dg_hi, w_dg_lo, nullptr, 0, dx, dx_ld, 0, 0, 0, stream);
}

extern "C" int crimac_conv1x1_wgrad(int prec, const void* dz, long dz_ld, int Cout, const void* x, long x_ld, int Cin,
                                    long M, float* dw, void* stream) {
  CRIMAC_REQUIRE(prec_ok(prec, true), "conv1x1_wgrad: bad precision %d", prec);
  CRIMAC_REQUIRE(Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0,
                 "conv1x1_wgrad: Cin=%d and Cout=%d must be positive multiples of 64", Cin, Cout);
  CRIMAC_REQUIRE(M > 0 && dz_ld >= Cout && dz_ld % 8 == 0 && x_ld >= Cin && x_ld % 8 == 0,
                 "conv1x1_wgrad: bad pixel count or strides");
  CRIMAC_REQUIRE(dz && x && dw, "conv1x1_wgrad: null pointer");
  hipStream_t st = (hipStream_t)stream;
  CRIMAC_FOR_STORAGE2(prec, TF, TP, { return launch_wgrad1x1<TF, TP>(dz, dz_ld, Cout, x, x_ld, Cin, M, dw, st); });
  return CRIMAC_OK;
}
