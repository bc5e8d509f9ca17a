// Narrow layers (start_filts 8, 16, 32; reference unet.py:35-49 at any width): the 3x3 convolution and the k2 s2
// transposed convolution for layers whose channel counts lie below the 64-channel MFMA tiles of conv3x3.hip / igemm.hip,
// on CDNA4 (gfx950), NHWC.
//
// Two forms of the 3x3 convolution, both persistent (the layer's weights staged in LDS once per workgroup, the input halo
// of a tile read once, every output written once, BatchNorm statistics reduced per tile and flushed with one fp64 atomic
// per channel):
//   * 16-bit storage (BF16 / FP16): conv3x3_narrow_mfma_kernel, v_mfma_f32_16x16x32_{bf16,f16}.  M = 16 pixels of an image
//     row, N = 16 output channels per fragment (N = 8 runs one fragment with 8 zero weight columns), K = the flattened
//     (tap, channel) index, 32 per step: one tap x 32 channels (Cin 32, 64), two taps x 16 (Cin 16) or four taps x 8
//     (Cin 8) -- every 8-element lane group lies inside one tap because Cin % 8 == 0, so Cin = 8 is not padded to 16: its
//     72 K values run as 3 steps with the last 24 weights zero.  Weights [N][K] and the halo [pixel][Cin] are LDS rows
//     padded by 16 bytes, each fragment one 16-byte LDS read.
//   * 4-byte storage (the fp32 modes and the plane pairs of H3P): conv3x3_narrow_kernel, fp32 VALU FMAs of the stored
//     operands against LDS-broadcast fp32 weight rows (2 pixels x N accumulators per thread): these are the parity modes,
//     whose fp32-equivalent results would need the 3-plane split (6 MFMAs per product) and 3x the LDS of the 16-bit form.
//     (DESIGN.md has the comparison of the two forms on the 16-bit modes.)
//
// Weights are read straight from the fp32 master tensors (no packed planes):
//   conv3x3 forward: w [N][w_cin][3][3] (input channels >= w_cin are zero: the padded first layer), x scale[n] when given
//                    (eval-mode BatchNorm folded in, the caller passes the folded bias);
//   conv3x3 input gradient (CRIMAC_NARROW_DGRAD): w [Cin][w_cin][3][3] of the layer, transposed and flipped, output
//                    channel n = layer input channel w_col0 + n;
//   transposed convolution: w [Cin][Cout][2][2] (nn.ConvTranspose2d).
// Storage types (common.h): inputs are the mode's MFMA-operand type (TP: plane pairs in H3P), outputs the fp32-side
// type (TF) or, with CRIMAC_EPI_OUT_PLANES (H3P), plane pairs.
#include "common.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int TW = 16, TH = 32;  // conv tile: 16 columns x 32 rows, a thread owns rows ty and ty + 16 of column tx
constexpr int HW_ = TW + 2, HH_ = TH + 2, HPIX = HW_ * HH_;
constexpr int CK = 8;            // input channels staged per step

struct NarrowConv {
  const void* in; long in_ld;
  int B, H, W, Cin;
  const float* w; int w_cin, w_col0, dgrad;
  const float* scale; const float* bias;
  void* out; long out_ld;
  int relu;
  double* s0; double* s1; int reps, stat_ld;
  int tiles_x, tiles_y; long ntiles;
};

template <typename TI, typename TO, int N>
__global__ __launch_bounds__(NT) void conv3x3_narrow_kernel(NarrowConv p) {
  extern __shared__ float lds[];
  float* ws = lds;                               // [9][Cin][N]
  float* xs = ws + 9 * p.Cin * N;                // [CK][HPIX]
  float* red = xs + CK * HPIX;                   // [4 waves][2N]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = tid % TW, ty = tid / TW;
  for (int i = tid; i < 9 * p.Cin * N; i += NT) {
    const int n = i % N, k = (i / N) % p.Cin, t = i / (N * p.Cin);
    float v;
    if (p.dgrad) {
      v = p.w[((long)k * p.w_cin + p.w_col0 + n) * 9 + (8 - t)];
    } else {
      v = k < p.w_cin ? p.w[((long)n * p.w_cin + k) * 9 + t] : 0.f;
      if (p.scale) v *= p.scale[n];
    }
    ws[i] = v;
  }
  const TI* in = reinterpret_cast<const TI*>(p.in);
  TO* out = reinterpret_cast<TO*>(p.out);
  for (long tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int bx = (int)(tile % p.tiles_x), by = (int)((tile / p.tiles_x) % p.tiles_y);
    const int b = (int)(tile / ((long)p.tiles_x * p.tiles_y));
    const int x0 = bx * TW, y0 = by * TH;
    float acc[2][N];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int n = 0; n < N; ++n) acc[r][n] = 0.f;
    for (int c0 = 0; c0 < p.Cin; c0 += CK) {
      __syncthreads();                           // (weights staged / previous chunk consumed)
      for (int i = tid; i < HPIX; i += NT) {
        const int gy = y0 + i / HW_ - 1, gx = x0 + i % HW_ - 1;
        float v[8];
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
          load8(in + (((long)b * p.H + gy) * p.W + gx) * p.in_ld + c0, v);
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) xs[k * HPIX + i] = v[k];
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int dy = t / 3, dx = t % 3;
#pragma unroll
        for (int k = 0; k < CK; ++k) {
          const float a0 = xs[k * HPIX + (ty + dy) * HW_ + tx + dx];
          const float a1 = xs[k * HPIX + (ty + 16 + dy) * HW_ + tx + dx];
          const f32x4* wr = reinterpret_cast<const f32x4*>(ws + (t * p.Cin + c0 + k) * N);
#pragma unroll
          for (int n4 = 0; n4 < N / 4; ++n4) {
            const f32x4 w4 = wr[n4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc[0][n4 * 4 + j] = fmaf(a0, w4[j], acc[0][n4 * 4 + j]);
              acc[1][n4 * 4 + j] = fmaf(a1, w4[j], acc[1][n4 * 4 + j]);
            }
          }
        }
      }
    }
    // epilogue: bias, ReLU, store, statistics of the stored value
    float cs1[N], cs2[N];
#pragma unroll
    for (int n = 0; n < N; ++n) cs1[n] = cs2[n] = 0.f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int gy = y0 + ty + 16 * r, gx = x0 + tx;
      const bool ok = gy < p.H && gx < p.W;
#pragma unroll
      for (int n8 = 0; n8 < N / 8; ++n8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float u = acc[r][n8 * 8 + j] + (p.bias ? p.bias[n8 * 8 + j] : 0.f);
          if (p.relu) u = fmaxf(u, 0.f);
          v[j] = u;
          const float s = storage_round<TO>(u);
          cs1[n8 * 8 + j] += ok ? s : 0.f;
          cs2[n8 * 8 + j] += ok ? s * s : 0.f;
        }
        if (ok) store8(out + (((long)b * p.H + gy) * p.W + gx) * p.out_ld + n8 * 8, v);
      }
    }
    if (p.s0) {
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const float t1 = wave_sum(cs1[n]), t2 = wave_sum(cs2[n]);
        if (lane == 0) {
          red[wave * 2 * N + n] = t1;
          red[wave * 2 * N + N + n] = t2;
        }
      }
      __syncthreads();
      if (tid < 2 * N) {
        const float s = red[tid] + red[2 * N + tid] + red[4 * N + tid] + red[6 * N + tid];
        const long rep = (long)(tile % p.reps) * p.stat_ld;
        if (tid < N) atomicAdd(&p.s0[rep + tid], (double)s);
        else atomicAdd(&p.s1[rep + tid - N], (double)s);
      }
    }
  }
}

template <typename TI, typename TO, int N>
int conv_launch(const NarrowConv& p, hipStream_t st) {
  const size_t lds = (size_t)(9 * p.Cin * N + CK * HPIX + 8 * N) * sizeof(float);
  static unsigned long long attr_devs = 0;
  if (crimac_first_use_on_device(&attr_devs))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_narrow_kernel<TI, TO, N>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  const long per_cu = (long)(160 * 1024 / lds) < 4 ? (long)(160 * 1024 / lds) : 4;
  long grid = crimac_cu_count() * (per_cu > 0 ? per_cu : 1);
  if (grid > p.ntiles) grid = p.ntiles;
  hipLaunchKernelGGL((conv3x3_narrow_kernel<TI, TO, N>), dim3((unsigned)grid), dim3(NT), lds, st, p);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

template <typename TI, typename TO>
int conv_launch_n(const NarrowConv& p, int N, hipStream_t st) {
  switch (N) {
    case 8: return conv_launch<TI, TO, 8>(p, st);
    case 16: return conv_launch<TI, TO, 16>(p, st);
    case 32: return conv_launch<TI, TO, 32>(p, st);
    default: return conv_launch<TI, TO, 64>(p, st);
  }
}

// ---- 16-bit storage: MFMA form -----------------------------------------------------------------------------------------
constexpr int MT = 16;                            // tile 16 x 16 pixels; wave w owns image rows 4w .. 4w + 3
constexpr int MHW = MT + 2, MPIX = MHW * MHW;

template <typename T16, int N>
__global__ __launch_bounds__(NT) void conv3x3_narrow_mfma_kernel(NarrowConv p) {
  constexpr int NB = (N + 15) / 16, NP = NB * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Cin = p.Cin, K = 9 * Cin, S = (K + 31) / 32, Kp = S * 32;
  const int wpitch = Kp + 8, xpitch = Cin + 8;    // (halves; +16 bytes per row against bank-aligned strides)
  unsigned short* ws = reinterpret_cast<unsigned short*>(smem);                  // [NP][wpitch]
  unsigned short* xs = ws + NP * wpitch;                                           // [MPIX][xpitch]
  float* red = reinterpret_cast<float*>(xs + MPIX * xpitch);                       // [4 waves][2 NP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  for (int i = tid; i < NP * Kp; i += NT) {
    const int n = i / Kp, k = i % Kp, t = k / Cin, c = k % Cin;
    float v = 0.f;
    if (n < N && t < 9) {
      if (p.dgrad) {
        v = p.w[((long)c * p.w_cin + p.w_col0 + n) * 9 + (8 - t)];
      } else if (c < p.w_cin) {
        v = p.w[((long)n * p.w_cin + c) * 9 + t];
        if (p.scale) v *= p.scale[n];
      }
    }
    ws[n * wpitch + k] = E16<T16>::bits(v);
  }
  float bias[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) bias[nb] = (p.bias && nb * 16 + fr < N) ? p.bias[nb * 16 + fr] : 0.f;
  const T16* in = reinterpret_cast<const T16*>(p.in);
  T16* out = reinterpret_cast<T16*>(p.out);
  const int c8n = Cin / 8;
  for (long tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int bx = (int)(tile % p.tiles_x), by = (int)((tile / p.tiles_x) % p.tiles_y);
    const int b = (int)(tile / ((long)p.tiles_x * p.tiles_y));
    const int x0 = bx * MT, y0 = by * MT;
    __syncthreads();                             // (weights staged / previous halo consumed)
    for (int i = tid; i < MPIX * c8n; i += NT) {
      const int px = i / c8n, c8 = i % c8n;
      const int gy = y0 + px / MHW - 1, gx = x0 + px % MHW - 1;
      u16x8 v = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
        v = *reinterpret_cast<const u16x8*>(in + (((long)b * p.H + gy) * p.W + gx) * p.in_ld + c8 * 8);
      *reinterpret_cast<u16x8*>(xs + px * xpitch + c8 * 8) = v;
    }
    __syncthreads();
    f32x4 acc[4][NB];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[r][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const int k0 = s * 32 + fq * 8, t = k0 / Cin, c = k0 - t * Cin;
      bf16x8 bw[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bw[nb] = *reinterpret_cast<const bf16x8*>(ws + (nb * 16 + fr) * wpitch + k0);
      const bool valid = t < 9;
      const int dy = valid ? t / 3 : 0, dx = valid ? t % 3 : 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + ((wave * 4 + r + dy) * MHW + fr + dx) * xpitch + (valid ? c : 0));
        // (past the last tap the weights are zero, the A read stays inside the halo)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[r][nb] = E16<T16>::mfma16(af, bw[nb], acc[r][nb]);
      }
    }
    // accumulator element i of fragment (r, nb): pixel x0 + fq * 4 + i of row y0 + 4 * wave + r, channel nb * 16 + fr
    float cs1[NB], cs2[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) cs1[nb] = cs2[nb] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gy = y0 + wave * 4 + r;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int n = nb * 16 + fr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gx = x0 + fq * 4 + i;
          float v = acc[r][nb][i] + bias[nb];
          if (p.relu) v = fmaxf(v, 0.f);
          const T16 q = (T16)v;
          const bool ok = gy < p.H && gx < p.W && n < N;
          if (ok) out[(((long)b * p.H + gy) * p.W + gx) * p.out_ld + n] = q;
          const float vs = (float)q;
          cs1[nb] += ok ? vs : 0.f;
          cs2[nb] += ok ? vs * vs : 0.f;
        }
      }
    }
    if (p.s0) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        float t1 = cs1[nb], t2 = cs2[nb];
        t1 += __shfl_xor(t1, 16, 64); t1 += __shfl_xor(t1, 32, 64);
        t2 += __shfl_xor(t2, 16, 64); t2 += __shfl_xor(t2, 32, 64);
        if (lane < 16) {
          red[wave * 2 * NP + nb * 16 + lane] = t1;
          red[wave * 2 * NP + NP + nb * 16 + lane] = t2;
        }
      }
      __syncthreads();
      if (tid < 2 * NP && (tid % NP) < N) {
        const float sum = red[tid] + red[2 * NP + tid] + red[4 * NP + tid] + red[6 * NP + tid];
        const long rep = (long)(tile % p.reps) * p.stat_ld;
        if (tid < NP) atomicAdd(&p.s0[rep + tid], (double)sum);
        else atomicAdd(&p.s1[rep + tid - NP], (double)sum);
      }
    }
  }
}

template <typename T16, int N>
int mfma_launch(NarrowConv p, hipStream_t st) {
  constexpr int NP = (N + 15) / 16 * 16;
  const int Kp = (9 * p.Cin + 31) / 32 * 32;
  const size_t lds = (size_t)NP * (Kp + 8) * 2 + (size_t)MPIX * (p.Cin + 8) * 2 + 8 * NP * sizeof(float);
  static unsigned long long attr_devs = 0;
  if (crimac_first_use_on_device(&attr_devs))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_narrow_mfma_kernel<T16, N>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  p.tiles_x = cdiv(p.W, MT); p.tiles_y = cdiv(p.H, MT); p.ntiles = (long)p.B * p.tiles_x * p.tiles_y;
  const long per_cu = (long)(160 * 1024 / lds) < 4 ? (long)(160 * 1024 / lds) : 4;
  long grid = crimac_cu_count() * (per_cu > 0 ? per_cu : 1);
  if (grid > p.ntiles) grid = p.ntiles;
  hipLaunchKernelGGL((conv3x3_narrow_mfma_kernel<T16, N>), dim3((unsigned)grid), dim3(NT), lds, st, p);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

template <typename T16>
int mfma_launch_n(const NarrowConv& p, int N, hipStream_t st) {
  switch (N) {
    case 8: return mfma_launch<T16, 8>(p, st);
    case 16: return mfma_launch<T16, 16>(p, st);
    case 32: return mfma_launch<T16, 32>(p, st);
    default: return mfma_launch<T16, 64>(p, st);
  }
}

// ---- transposed convolution k2 s2 -------------------------------------------------------------------------------------
// forward: one thread = one coarse pixel, all four outputs (2y + a, 2x + b) from one read of its input; weights [q][k][n]
// in LDS
template <typename TI, typename TO, int N>
__global__ __launch_bounds__(NT) void upconv_narrow_fwd_kernel(const TI* __restrict__ in, long in_ld, int B, int H, int W,
                                                               int Cin, const float* __restrict__ w,
                                                               const float* __restrict__ bias, TO* __restrict__ out,
                                                               long out_ld) {
  extern __shared__ float wq[];                  // [4][Cin][N]
  for (int i = threadIdx.x; i < 4 * Cin * N; i += NT) {
    const int n = i % N, k = (i / N) % Cin, q = i / (N * Cin);
    wq[i] = w[((long)k * N + n) * 4 + q];
  }
  __syncthreads();
  const long M = (long)B * H * W;
  const long pix = (long)blockIdx.x * NT + threadIdx.x;
  if (pix >= M) return;
  float acc[4][N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float b0 = bias ? bias[n] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q][n] = b0;
  }
  for (int c0 = 0; c0 < Cin; c0 += 8) {
    float v[8];
    load8(in + pix * in_ld + c0, v);
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4* wr = reinterpret_cast<const f32x4*>(wq + (q * Cin + c0 + k) * N);
#pragma unroll
        for (int n4 = 0; n4 < N / 4; ++n4) {
          const f32x4 w4 = wr[n4];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[q][n4 * 4 + j] = fmaf(v[k], w4[j], acc[q][n4 * 4 + j]);
        }
      }
  }
  const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    TO* o = out + (((long)b * 2 * H + 2 * y + (q >> 1)) * 2 * W + 2 * x + (q & 1)) * out_ld;
#pragma unroll
    for (int n8 = 0; n8 < N / 8; ++n8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = acc[q][n8 * 8 + j];
      store8(o + n8 * 8, v);
    }
  }
}

// input gradient: one thread = one coarse pixel, all Cin outputs; weights [q][n][k] in LDS
template <typename TI, typename TO, int CI>
__global__ __launch_bounds__(NT) void upconv_narrow_dgrad_kernel(const TI* __restrict__ dy, long dy_ld, int B, int H, int W,
                                                                 int N, const float* __restrict__ w, TO* __restrict__ dx,
                                                                 long dx_ld) {
  extern __shared__ float wt[];                  // [4][N][CI]
  for (int i = threadIdx.x; i < 4 * N * CI; i += NT) {
    const int k = i % CI, n = (i / CI) % N, q = i / (CI * N);
    wt[i] = w[((long)k * N + n) * 4 + q];
  }
  __syncthreads();
  const long M = (long)B * H * W;
  const long pix = (long)blockIdx.x * NT + threadIdx.x;
  if (pix >= M) return;
  const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
  float acc[CI];
#pragma unroll
  for (int k = 0; k < CI; ++k) acc[k] = 0.f;
  for (int q = 0; q < 4; ++q) {
    const TI* src = dy + (((long)b * 2 * H + 2 * y + (q >> 1)) * 2 * W + 2 * x + (q & 1)) * dy_ld;
    for (int n0 = 0; n0 < N; n0 += 8) {
      float v[8];
      load8(src + n0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4* wr = reinterpret_cast<const f32x4*>(wt + (q * N + n0 + j) * CI);
#pragma unroll
        for (int k4 = 0; k4 < CI / 4; ++k4) {
          const f32x4 w4 = wr[k4];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[k4 * 4 + i] = fmaf(v[j], w4[i], acc[k4 * 4 + i]);
        }
      }
    }
  }
  TO* o = dx + pix * dx_ld;
#pragma unroll
  for (int k8 = 0; k8 < CI / 8; ++k8) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = acc[k8 * 8 + i];
    store8(o + k8 * 8, v);
  }
}

bool narrow_n_ok(int n) { return n == 8 || n == 16 || n == 32; }

}  // namespace

// Storage-type pair of a narrow launch: TI = the mode's operand type, TO = its fp32-side type or plane pairs
#define CRIMAC_NARROW_TYPES(prec, planes_out, TI, TO, ...)                                       \
  do {                                                                                          \
    if ((prec) == CRIMAC_PREC_BF16) { using TI = bf16_t; using TO = bf16_t; __VA_ARGS__; }       \
    else if ((prec) == CRIMAC_PREC_FP16) { using TI = half_t; using TO = half_t; __VA_ARGS__; }  \
    else if ((prec) == CRIMAC_PREC_H3P && (planes_out)) { using TI = hp_t; using TO = hp_t; __VA_ARGS__; } \
    else if ((prec) == CRIMAC_PREC_H3P) { using TI = hp_t; using TO = float; __VA_ARGS__; }       \
    else { using TI = float; using TO = float; __VA_ARGS__; }                                    \
  } while (0)

extern "C" int crimac_conv3x3_narrow(int prec, const void* in, long in_ld, int B, int H, int W, int Cin, int N,
                                     const float* w, int w_cin, int w_col0, int flags, const float* scale,
                                     const float* bias, void* out, long out_ld, double* stat_sum, double* stat_sumsq,
                                     int stat_replicas, int stat_ld, void* stream) {
  CRIMAC_REQUIRE(prec >= CRIMAC_PREC_BF16 && prec <= CRIMAC_PREC_MAX, "conv3x3_narrow: bad precision %d", prec);
  const bool dgrad = (flags & CRIMAC_NARROW_DGRAD) != 0;
  CRIMAC_REQUIRE(narrow_n_ok(N) || (N == 64 && Cin <= 32),
                 "conv3x3_narrow: N=%d must be 8, 16 or 32 (64 with Cin <= 32: the forward of a 32 -> 64 layer)", N);
  CRIMAC_REQUIRE(Cin > 0 && Cin % 8 == 0 && Cin <= 64, "conv3x3_narrow: Cin=%d must be a multiple of 8 up to 64", Cin);
  CRIMAC_REQUIRE((flags & ~(CRIMAC_EPI_RELU | CRIMAC_EPI_OUT_PLANES | CRIMAC_NARROW_DGRAD)) == 0,
                 "conv3x3_narrow: unknown flags %d", flags);
  CRIMAC_REQUIRE(!(flags & CRIMAC_EPI_OUT_PLANES) || prec == CRIMAC_PREC_H3P,
                 "conv3x3_narrow: plane-pair output is an H3P option");
  CRIMAC_REQUIRE(in && w && out && B > 0 && H > 0 && W > 0, "conv3x3_narrow: bad arguments");
  CRIMAC_REQUIRE(in_ld >= Cin && in_ld % 8 == 0 && out_ld >= N && out_ld % 8 == 0,
                 "conv3x3_narrow: bad pixel strides (in_ld=%ld out_ld=%ld)", in_ld, out_ld);
  CRIMAC_REQUIRE(dgrad ? (w_cin > 0 && w_col0 >= 0 && w_col0 + N <= w_cin && !scale && !bias)
                       : (w_cin > 0 && w_cin <= Cin && w_col0 == 0),
                 "conv3x3_narrow: weight shape (w_cin=%d, w_col0=%d) does not fit Cin=%d N=%d", w_cin, w_col0, Cin, N);
  CRIMAC_REQUIRE(!stat_sum || (stat_sumsq && stat_replicas >= 1 && stat_ld >= N),
                 "conv3x3_narrow: statistics need both accumulators, replicas >= 1 and stat_ld >= N");
  NarrowConv p;
  p.in = in; p.in_ld = in_ld; p.B = B; p.H = H; p.W = W; p.Cin = Cin;
  p.w = w; p.w_cin = w_cin; p.w_col0 = w_col0; p.dgrad = dgrad; p.scale = scale; p.bias = bias;
  p.out = out; p.out_ld = out_ld; p.relu = flags & CRIMAC_EPI_RELU;
  p.s0 = stat_sum; p.s1 = stat_sumsq; p.reps = stat_replicas > 0 ? stat_replicas : 1; p.stat_ld = stat_ld;
  p.tiles_x = cdiv(W, TW); p.tiles_y = cdiv(H, TH); p.ntiles = (long)B * p.tiles_x * p.tiles_y;
  hipStream_t st = (hipStream_t)stream;
  if (prec == CRIMAC_PREC_BF16) return mfma_launch_n<bf16_t>(p, N, st);
  if (prec == CRIMAC_PREC_FP16) return mfma_launch_n<half_t>(p, N, st);
  if (prec == CRIMAC_PREC_H3P)
    return (flags & CRIMAC_EPI_OUT_PLANES) ? conv_launch_n<hp_t, hp_t>(p, N, st) : conv_launch_n<hp_t, float>(p, N, st);
  return conv_launch_n<float, float>(p, N, st);
}

extern "C" int crimac_upconv2x2_narrow(int prec, const void* in, long in_ld, int B, int H, int W, int Cin, int Cout,
                                       const float* w, const float* bias, void* out, long out_ld, int flags,
                                       void* stream) {
  CRIMAC_REQUIRE(prec >= CRIMAC_PREC_BF16 && prec <= CRIMAC_PREC_MAX, "upconv2x2_narrow: bad precision %d", prec);
  CRIMAC_REQUIRE(narrow_n_ok(Cout), "upconv2x2_narrow: Cout=%d must be 8, 16 or 32", Cout);
  CRIMAC_REQUIRE(Cin > 0 && Cin % 8 == 0 && Cin <= 64, "upconv2x2_narrow: Cin=%d must be a multiple of 8 up to 64", Cin);
  CRIMAC_REQUIRE((flags & ~CRIMAC_EPI_OUT_PLANES) == 0 && (!flags || prec == CRIMAC_PREC_H3P),
                 "upconv2x2_narrow: flags %d (plane-pair output is an H3P option)", flags);
  CRIMAC_REQUIRE(in && w && out && B > 0 && H > 0 && W > 0, "upconv2x2_narrow: bad arguments");
  CRIMAC_REQUIRE(in_ld >= Cin && in_ld % 8 == 0 && out_ld >= Cout && out_ld % 8 == 0,
                 "upconv2x2_narrow: bad pixel strides (in_ld=%ld out_ld=%ld)", in_ld, out_ld);
  const long M = (long)B * H * W;
  const dim3 grid((unsigned)cdiv(M, NT));
  const size_t lds = (size_t)4 * Cin * Cout * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  CRIMAC_NARROW_TYPES(prec, flags, TI, TO, {
    switch (Cout) {
      case 8: hipLaunchKernelGGL((upconv_narrow_fwd_kernel<TI, TO, 8>), grid, dim3(NT), lds, st, (const TI*)in, in_ld, B, H,
                                 W, Cin, w, bias, (TO*)out, out_ld); break;
      case 16: hipLaunchKernelGGL((upconv_narrow_fwd_kernel<TI, TO, 16>), grid, dim3(NT), lds, st, (const TI*)in, in_ld, B,
                                  H, W, Cin, w, bias, (TO*)out, out_ld); break;
      default: hipLaunchKernelGGL((upconv_narrow_fwd_kernel<TI, TO, 32>), grid, dim3(NT), lds, st, (const TI*)in, in_ld, B,
                                  H, W, Cin, w, bias, (TO*)out, out_ld); break;
    }
  });
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_upconv2x2_dgrad_narrow(int prec, const void* dy, long dy_ld, int B, int H, int W, int Cout, int Cin,
                                             const float* w, void* dx, long dx_ld, void* stream) {
  CRIMAC_REQUIRE(prec >= CRIMAC_PREC_BF16 && prec <= CRIMAC_PREC_MAX, "upconv2x2_dgrad_narrow: bad precision %d", prec);
  CRIMAC_REQUIRE(Cout > 0 && Cout % 8 == 0 && Cout <= 64, "upconv2x2_dgrad_narrow: Cout=%d must be a multiple of 8 up to 64",
                 Cout);
  CRIMAC_REQUIRE(Cin == 16 || Cin == 32 || Cin == 64, "upconv2x2_dgrad_narrow: Cin=%d must be 16, 32 or 64", Cin);
  CRIMAC_REQUIRE(dy && w && dx && B > 0 && H > 0 && W > 0, "upconv2x2_dgrad_narrow: bad arguments");
  CRIMAC_REQUIRE(dy_ld >= Cout && dy_ld % 8 == 0 && dx_ld >= Cin && dx_ld % 8 == 0,
                 "upconv2x2_dgrad_narrow: bad pixel strides (dy_ld=%ld dx_ld=%ld)", dy_ld, dx_ld);
  const long M = (long)B * H * W;
  const dim3 grid((unsigned)cdiv(M, NT));
  const size_t lds = (size_t)4 * Cout * Cin * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  CRIMAC_NARROW_TYPES(prec, 0, TI, TO, {
    switch (Cin) {
      case 16: hipLaunchKernelGGL((upconv_narrow_dgrad_kernel<TI, TO, 16>), grid, dim3(NT), lds, st, (const TI*)dy, dy_ld, B,
                                  H, W, Cout, w, (TO*)dx, dx_ld); break;
      case 32: hipLaunchKernelGGL((upconv_narrow_dgrad_kernel<TI, TO, 32>), grid, dim3(NT), lds, st, (const TI*)dy, dy_ld, B,
                                  H, W, Cout, w, (TO*)dx, dx_ld); break;
      default: hipLaunchKernelGGL((upconv_narrow_dgrad_kernel<TI, TO, 64>), grid, dim3(NT), lds, st, (const TI*)dy, dy_ld, B,
                                  H, W, Cout, w, (TO*)dx, dx_ld); break;
    }
  });
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}
