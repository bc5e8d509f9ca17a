// Late metadata injection (reference: UNet_LateMetInject, crimac_unet/models/unet.py:346-391, and
// MetaPostProcessing, unet.py:140-166) for CDNA4 (gfx950).
//
//   m       = W3 . relu(W2 . relu(W1 . meta + b1) + b2) + b3          per pixel, meta [B][Cm][H][W] fp32 (NCHW, as
//                                                                    the reference Dataset hands it over)
//   logits  = conv_final([x | m])  =  Wf[:, :64] . x  +  Wf[:, 64] * m  +  bf         (torch.cat((x, m), 1), :386-388)
//
// The 64-channel part of the head is crimac_head_fwd / crimac_head_bwd (elementwise.hip) on the first 64 columns of
// conv_final.weight; the kernels here add the metadata column and its 3-layer perceptron.  All of it is HBM-bound
// fp32 work on [B*H*W] pixels (Cm <= 8 input planes, one output plane): one thread per pixel, the 1.2 K perceptron
// weights in LDS (broadcast reads), hidden activations in registers.  The weight gradients of the 32 x 32 layer are an
// outer-product sum over pixels: every 256-pixel block stages (dh2, h1) in LDS and each thread accumulates four of
// the 1024 products over the block's pixels; workgroup partials go out by fp32 atomics once per workgroup.
#include "common.h"
#include "bnb_sums.h"
#include "meta_planes.h"

namespace {

constexpr int HID = 32;          // MetaPostProcessing.hidden_channels_1/2 (unet.py:147-148)
constexpr int MAX_CM = 8;        // get_in_channels (pipeline.py:413-425) yields at most 7
constexpr int HEAD_C = 64;       // channels in front of conv_final (unet.py:342: start_filts of the configured net)

struct MlpW {
  const float *w1, *b1, *w2, *b2, *w3, *b3;      // [32][Cm], [32], [32][32], [32], [1][32], [1]
};

__device__ __forceinline__ void load_weights(const MlpW& w, int Cm, float* s) {
  // LDS image: w1 [32][MAX_CM] | b1 [32] | w2 [32][32] | b2 [32] | w3 [32] | b3 [1]
  for (int i = threadIdx.x; i < HID * MAX_CM; i += blockDim.x) {
    const int j = i / MAX_CM, c = i % MAX_CM;
    s[i] = c < Cm ? w.w1[j * Cm + c] : 0.f;
  }
  float* p = s + HID * MAX_CM;
  for (int i = threadIdx.x; i < HID; i += blockDim.x) p[i] = w.b1[i];
  p += HID;
  for (int i = threadIdx.x; i < HID * HID; i += blockDim.x) p[i] = w.w2[i];
  p += HID * HID;
  for (int i = threadIdx.x; i < HID; i += blockDim.x) p[i] = w.b2[i];
  p += HID;
  for (int i = threadIdx.x; i < HID; i += blockDim.x) p[i] = w.w3[i];
  p += HID;
  if (threadIdx.x == 0) p[0] = w.b3[0];
}
constexpr int W_FLOATS = HID * MAX_CM + HID + HID * HID + HID + HID + 1;

__device__ __forceinline__ float mlp_forward(const float* s, const float (&x)[MAX_CM], float (&h1)[HID], float (&h2)[HID]) {
  const float *w1 = s, *b1 = s + HID * MAX_CM, *w2 = b1 + HID, *b2 = w2 + HID * HID, *w3 = b2 + HID, *b3 = w3 + HID;
#pragma unroll
  for (int j = 0; j < HID; ++j) {
    float a = b1[j];
#pragma unroll
    for (int c = 0; c < MAX_CM; ++c) a += w1[j * MAX_CM + c] * x[c];
    h1[j] = fmaxf(a, 0.f);
  }
  float m = b3[0];
#pragma unroll
  for (int j = 0; j < HID; ++j) {
    float a = b2[j];
#pragma unroll
    for (int i = 0; i < HID; ++i) a += w2[j * HID + i] * h1[i];
    h2[j] = fmaxf(a, 0.f);
    m += w3[j] * h2[j];
  }
  return m;
}

__global__ __launch_bounds__(256) void meta_mlp_fwd_kernel(const float* __restrict__ meta, int Cm, long npix, long HW,
                                                           MlpW w, float* __restrict__ m_out) {
  __shared__ float s[W_FLOATS];
  load_weights(w, Cm, s);
  __syncthreads();
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    const long b = p / HW, hw = p - b * HW;
    float x[MAX_CM], h1[HID], h2[HID];
#pragma unroll
    for (int c = 0; c < MAX_CM; ++c) x[c] = c < Cm ? meta[(b * Cm + c) * HW + hw] : 0.f;
    m_out[p] = mlp_forward(s, x, h1, h2);
  }
}

// logits[b][o][hw] += wm[o] * m[b*HW + hw]   (+ softmax over the classes)
template <int NC>
__global__ __launch_bounds__(256) void meta_inject_fwd_kernel(const float* __restrict__ m, const float* __restrict__ wm,
                                                              float* __restrict__ logits, long npix, long HW,
                                                              int softmax) {
  float wv[NC];
#pragma unroll
  for (int o = 0; o < NC; ++o) wv[o] = wm[o];
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    const long b = p / HW, hw = p - b * HW;
    const float mv = m[p];
    float z[NC];
#pragma unroll
    for (int o = 0; o < NC; ++o) z[o] = logits[(b * NC + o) * HW + hw] + wv[o] * mv;
    if (softmax) {
      float mx = z[0];
#pragma unroll
      for (int o = 1; o < NC; ++o) mx = fmaxf(mx, z[o]);
      float den = 0.f;
#pragma unroll
      for (int o = 0; o < NC; ++o) { z[o] = expf(z[o] - mx); den += z[o]; }
#pragma unroll
      for (int o = 0; o < NC; ++o) z[o] /= den;
    }
#pragma unroll
    for (int o = 0; o < NC; ++o) logits[(b * NC + o) * HW + hw] = z[o];
  }
}

// Backward of the metadata column and of the perceptron:
//   dwm[o] += sum_p dl[o][p] * m[p];   dm[p] = sum_o dl[o][p] * wm[o];   then the three Linear layers.
template <int NC>
__global__ __launch_bounds__(256) void meta_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ meta, int Cm,
                                                       long npix, long HW, const float* __restrict__ wm, MlpW w,
                                                       float* dwm, float* gw1, float* gb1, float* gw2, float* gb2,
                                                       float* gw3, float* gb3) {
  // dynamic LDS (116 KB): weights | h1 | dh2 | dh1 of the block's pixels (row pitch 33: conflict-free column walks) |
  // metadata inputs | reduction scratch
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* s = reinterpret_cast<float*>(smem_raw);
  float (*sh1)[HID + 1] = reinterpret_cast<float (*)[HID + 1]>(s + ((W_FLOATS + 3) & ~3));
  float (*sd2)[HID + 1] = sh1 + 256;
  float (*sd1)[HID + 1] = sd2 + 256;
  float (*sx)[MAX_CM + 1] = reinterpret_cast<float (*)[MAX_CM + 1]>(sd1 + 256);
  float* red = reinterpret_cast<float*>(sx + 256);
  load_weights(w, Cm, s);
  const float *w2 = s + HID * MAX_CM + HID, *w3 = w2 + HID * HID + HID;
  float wv[NC];
#pragma unroll
  for (int o = 0; o < NC; ++o) wv[o] = wm[o];
  const int t = threadIdx.x;
  // this thread's four entries of dW2 [j][i0..i0+3], its entries of dW1 [j1][c] (t < 32 * MAX_CM), and of the vectors
  const int j2 = t >> 3, i0 = (t & 7) * 4;
  float a2[4] = {0.f, 0.f, 0.f, 0.f}, a1 = 0.f, av = 0.f;       // av: gb1/gb2/gw3 by thread role (below)
  const int j1 = t / MAX_CM, c1 = t % MAX_CM;
  float dwm_acc[NC], gb3_acc = 0.f;
#pragma unroll
  for (int o = 0; o < NC; ++o) dwm_acc[o] = 0.f;
  __syncthreads();
  for (long p0 = (long)blockIdx.x * 256; p0 < npix; p0 += (long)gridDim.x * 256) {
    const long p = p0 + t;
    const bool ok = p < npix;
    float x[MAX_CM], h1[HID], h2[HID];
    float dm = 0.f, mval = 0.f;
    if (ok) {
      const long b = p / HW, hw = p - b * HW;
#pragma unroll
      for (int c = 0; c < MAX_CM; ++c) x[c] = c < Cm ? meta[(b * Cm + c) * HW + hw] : 0.f;
      mval = mlp_forward(s, x, h1, h2);
#pragma unroll
      for (int o = 0; o < NC; ++o) {
        const float g = dl[(b * NC + o) * HW + hw];
        dm += g * wv[o];
        dwm_acc[o] += g * mval;
      }
    } else {
#pragma unroll
      for (int c = 0; c < MAX_CM; ++c) x[c] = 0.f;
#pragma unroll
      for (int j = 0; j < HID; ++j) { h1[j] = 0.f; h2[j] = 0.f; }
    }
    gb3_acc += dm;
    float dh2[HID], dh1[HID];
#pragma unroll
    for (int i = 0; i < HID; ++i) dh1[i] = 0.f;
#pragma unroll
    for (int j = 0; j < HID; ++j) {
      dh2[j] = h2[j] > 0.f ? dm * w3[j] : 0.f;
#pragma unroll
      for (int i = 0; i < HID; ++i) dh1[i] += w2[j * HID + i] * dh2[j];
    }
#pragma unroll
    for (int i = 0; i < HID; ++i) {
      dh1[i] = h1[i] > 0.f ? dh1[i] : 0.f;
      sh1[t][i] = h1[i];
      sd1[t][i] = dh1[i];
      sd2[t][i] = dh2[i];
    }
#pragma unroll
    for (int c = 0; c < MAX_CM; ++c) sx[t][c] = x[c];
    // gw3[j] += dm * h2[j]: fold over the block through the dh2 image later would lose h2; do it by wave shuffles
    // of the 32 values is expensive -- instead reuse sd1 row-major AFTER the outer products (below).
    __syncthreads();
    // outer products over the block's 256 pixels
    for (int q = 0; q < 256; ++q) {
      const float d2 = sd2[q][j2];
#pragma unroll
      for (int k = 0; k < 4; ++k) a2[k] += d2 * sh1[q][i0 + k];
    }
    if (t < HID * MAX_CM) {
      for (int q = 0; q < 256; ++q) a1 += sd1[q][j1] * sx[q][c1];
    }
    // vectors: threads 0..31 -> gb2[j] = sum dh2[j]; 32..63 -> gb1[j] = sum dh1[j]
    if (t < HID) {
      for (int q = 0; q < 256; ++q) av += sd2[q][t];
    } else if (t < 2 * HID) {
      for (int q = 0; q < 256; ++q) av += sd1[q][t - HID];
    }
    __syncthreads();
    // gw3[j] += dm * h2[j]: stage (dm * h2) in sd2 and let threads 64..95 sum the columns
#pragma unroll
    for (int j = 0; j < HID; ++j) sd2[t][j] = dm * h2[j];
    __syncthreads();
    if (t >= 2 * HID && t < 3 * HID) {
      for (int q = 0; q < 256; ++q) av += sd2[q][t - 2 * HID];
    }
    __syncthreads();
  }
  // workgroup partials -> global
#pragma unroll
  for (int k = 0; k < 4; ++k) atomicAdd(&gw2[j2 * HID + i0 + k], a2[k]);
  if (t < HID * MAX_CM && c1 < Cm) atomicAdd(&gw1[j1 * Cm + c1], a1);
  if (t < HID) atomicAdd(&gb2[t], av);
  else if (t < 2 * HID) atomicAdd(&gb1[t - HID], av);
  else if (t < 3 * HID) atomicAdd(&gw3[t - 2 * HID], av);
  // dwm, gb3: wave reduce, then LDS, then one atomic each
  float v[NC + 1];
#pragma unroll
  for (int o = 0; o < NC; ++o) v[o] = wave_sum(dwm_acc[o]);
  v[NC] = wave_sum(gb3_acc);
  if ((t & 63) == 0)
    for (int o = 0; o <= NC; ++o) red[(t >> 6) * 8 + o] = v[o];
  __syncthreads();
  if (t <= NC) {
    const float sum = red[t] + red[8 + t] + red[16 + t] + red[24 + t];
    if (t < NC) atomicAdd(&dwm[t], sum);
    else atomicAdd(&gb3[0], sum);
  }
}


// ---- the late-injection head's forward in one pass ----------------------------------------------------------------
// (unet.py:386-388; pipeline.py:170-174, :210-216): head_fwd64_kernel's lane layout (elementwise.hip) -- a group of
// 8 lanes takes 8 consecutive pixels, a transposing butterfly leaves lane s with the sums of pixel s -- so every thread
// ends up owning ONE pixel, for which it then evaluates the perceptron (weights in LDS, loaded once per workgroup) and
// the metadata column.  The fp32 operations of a pixel are those of crimac_head_fwd, crimac_meta_mlp_fwd and
// crimac_meta_inject_fwd in that order (head sum + bias, + wm * m, softmax): bit for bit the chain's logits, without the
// [B*H*W] plane m and without reading the logits back.  w is conv_final.weight as it stands: [NC][65], column 64 = wm.
template <typename T, int NC, typename TR>
__global__ __launch_bounds__(256) void head_meta_fwd_kernel(const T* __restrict__ x, long x_ld, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ meta,
                                                            int Cm, MlpW mw, float* __restrict__ logits, long npix, long HW,
                                                            int softmax, const float* __restrict__ bn_scale,
                                                            const float* __restrict__ bn_shift) {
  __shared__ float s[W_FLOATS];
  load_weights(mw, Cm, s);
  const int sub = threadIdx.x & 7;
  float bsc[8], bsh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bsc[j] = bn_scale ? bn_scale[sub * 8 + j] : 1.f;
    bsh[j] = bn_scale ? bn_shift[sub * 8 + j] : 0.f;
  }
  float wr[NC][8], bz[NC], wv[NC];
#pragma unroll
  for (int o = 0; o < NC; ++o) {
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[o][j] = w[o * (HEAD_C + 1) + sub * 8 + j];
    bz[o] = bias[o];
    wv[o] = w[o * (HEAD_C + 1) + HEAD_C];
  }
  const bool b4 = (sub & 4) != 0, b2 = (sub & 2) != 0, b1 = (sub & 1) != 0;
  const long step = (long)gridDim.x * 256;
  __syncthreads();
  for (long g0 = (long)blockIdx.x * 256 + (threadIdx.x & ~7); g0 < npix; g0 += step) {
    float a[8][NC];
    float v[8][8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (g0 + u < npix) load8s(x + (g0 + u) * x_ld + sub * 8, v[u]);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (bn_scale) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = storage_round<TR>(fmaxf(v[u][j] * bsc[j] + bsh[j], 0.f));
      }
#pragma unroll
      for (int o = 0; o < NC; ++o) {
        float s_ = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s_ = __builtin_fmaf(v[u][j], wr[o][j], s_);
        a[u][o] = s_;
      }
    }
    float r4[4][NC], r2[2][NC], z[NC];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int o = 0; o < NC; ++o) {
        const float mine = b4 ? a[u + 4][o] : a[u][o], theirs = b4 ? a[u][o] : a[u + 4][o];
        r4[u][o] = mine + __shfl_xor(theirs, 4, 64);
      }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int o = 0; o < NC; ++o) {
        const float mine = b2 ? r4[u + 2][o] : r4[u][o], theirs = b2 ? r4[u][o] : r4[u + 2][o];
        r2[u][o] = mine + __shfl_xor(theirs, 2, 64);
      }
#pragma unroll
    for (int o = 0; o < NC; ++o) {
      const float mine = b1 ? r2[1][o] : r2[0][o], theirs = b1 ? r2[0][o] : r2[1][o];
      z[o] = mine + __shfl_xor(theirs, 1, 64) + bz[o];
    }
    const long p = g0 + sub;
    if (p < npix) {
      const long b = p / HW, hw = p - b * HW;
      float xm[MAX_CM], h1[HID], h2[HID];
#pragma unroll
      for (int c = 0; c < MAX_CM; ++c) xm[c] = c < Cm ? meta[(b * Cm + c) * HW + hw] : 0.f;
      // (the compiler must not carry the 1.3 K weights across iterations in registers: they stay in LDS, broadcast reads)
      asm volatile("" ::: "memory");
      const float mv = mlp_forward(s, xm, h1, h2);
#pragma unroll
      for (int o = 0; o < NC; ++o) z[o] = z[o] + wv[o] * mv;
      if (softmax) {
        float mx = z[0];
#pragma unroll
        for (int o = 1; o < NC; ++o) mx = fmaxf(mx, z[o]);
        float den = 0.f;
#pragma unroll
        for (int o = 0; o < NC; ++o) { z[o] = expf(z[o] - mx); den += z[o]; }
#pragma unroll
        for (int o = 0; o < NC; ++o) z[o] /= den;
      }
#pragma unroll
      for (int o = 0; o < NC; ++o) logits[(b * NC + o) * HW + hw] = z[o];
    }
  }
}


// Backward of the late-injection head: ONE pass over dlogits.  A workgroup takes 256 pixels per iteration.
// Phase A, one thread per pixel: the thread reads its NC dlogits once (kept in LDS for phase B), adds them to the bias
// gradient and runs the perceptron forward and backward.  Only h1 / dh1 (32 + 32 registers) live in registers: the second
// layer is walked unit by unit (forward a2_j, dh2_j, and dh1 += w2[j] * dh2_j in the same step, weights broadcast from
// LDS), and what the outer products need goes to the thread's LDS rows (pitch 33: conflict-free) as it is formed -- the
// fully unrolled form of meta_bwd_kernel with h2 / dh2 in registers as well needs 512 registers and 2.5 KB of scratch.
// Then the outer products over the block's 256 pixels, as meta_bwd_kernel.
// Phase B, 8 lanes per pixel and 32 pixels per pass as head_bwd_kernel: da = dlogits . W[:, :64] (stored, and taken into
// the BatchNorm-backward sums of the block it feeds), dW[:, :64] += dlogits x activation.
// Partials leave the workgroup once, by fp32 atomics, straight into conv_final.weight's [NC][65] gradient (column 64: the
// metadata column), its bias gradient and the six perceptron gradients: all outputs ACCUMULATE (the caller zeroes).
// T: storage type of dx and of bnb.y; TX: of x / of the activation rebuilt from y (as head_bwd_kernel).
constexpr int HMB_UNR = 2;                               // phase B: pixels in flight per lane group (as head_bwd_kernel)
constexpr int HMB_HEAD = 4 * HEAD_C + 4;                 // LDS floats of the head's weight partials (NC <= 4)
constexpr int HMB_FLOATS = ((W_FLOATS + 3) & ~3) + 4 * 256 * (HID + 1) + 256 * (MAX_CM + 1) + 64 + 4 * 256 + HMB_HEAD +
                           2 * HEAD_C;
static_assert(HMB_FLOATS * sizeof(float) <= 160 * 1024, "head_meta_bwd: LDS");
template <typename T, int NC, bool BNB, typename TX>
__global__ __launch_bounds__(256) void head_meta_bwd_kernel(const float* __restrict__ dl, const TX* __restrict__ x, long x_ld,
                                                            const float* __restrict__ w, T* __restrict__ dx, long dx_ld,
                                                            float* dw, float* db, const float* __restrict__ meta, int Cm,
                                                            MlpW mw, float* gw1, float* gb1, float* gw2, float* gb2,
                                                            float* gw3, float* gb3, long npix, long HW, BnbArgs bnb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* s = reinterpret_cast<float*>(smem_raw);
  float (*sh1)[HID + 1] = reinterpret_cast<float (*)[HID + 1]>(s + ((W_FLOATS + 3) & ~3));
  float (*sd2)[HID + 1] = sh1 + 256;
  float (*sd1)[HID + 1] = sd2 + 256;
  float (*sm2)[HID + 1] = sd1 + 256;                                // dm * h2: the terms of gw3
  float (*sx)[MAX_CM + 1] = reinterpret_cast<float (*)[MAX_CM + 1]>(sm2 + 256);
  float* red = reinterpret_cast<float*>(sx + 256);                  // [4 waves][16]
  float (*sg)[256] = reinterpret_cast<float (*)[256]>(red + 64);    // dlogits of the block's pixels, [class][pixel]
  float* lds_head = reinterpret_cast<float*>(sg + 4);               // [NC][64]
  float* lds_bnb = lds_head + HMB_HEAD;                             // [2][64]
  const int t = threadIdx.x;
  for (int i = t; i < HMB_HEAD + 2 * HEAD_C; i += 256) lds_head[i] = 0.f;
  load_weights(mw, Cm, s);
  const float *w1 = s, *b1 = s + HID * MAX_CM, *w2 = b1 + HID, *b2 = w2 + HID * HID, *w3 = b2 + HID, *b3 = w3 + HID;
  // phase A roles in the outer products (meta_bwd_kernel)
  const int j2 = t >> 3, i0 = (t & 7) * 4;
  float a2[4] = {0.f, 0.f, 0.f, 0.f}, a1 = 0.f, av = 0.f;
  const int j1 = t / MAX_CM, c1 = t % MAX_CM;
  float wv[NC], dwm_acc[NC], gb_acc[NC], gb3_acc = 0.f;
  // phase B roles (head_bwd_kernel): channel chunk sub of pixel slot t >> 3
  const int sub = t & 7, slot = t >> 3;
  float wr[NC][8], gw[NC][8];
#pragma unroll
  for (int o = 0; o < NC; ++o) {
    wv[o] = w[o * (HEAD_C + 1) + HEAD_C];
    dwm_acc[o] = 0.f;
    gb_acc[o] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { wr[o][j] = w[o * (HEAD_C + 1) + sub * 8 + j]; gw[o][j] = 0.f; }
  }
  BnbConst k;
  float d1[8], d2[8];
  if constexpr (BNB) {
    bnb_load(bnb, sub * 8, k);
#pragma unroll
    for (int j = 0; j < 8; ++j) { d1[j] = 0.f; d2[j] = 0.f; }
  }
  __syncthreads();
  for (long p0 = (long)blockIdx.x * 256; p0 < npix; p0 += (long)gridDim.x * 256) {
    {
      const long p = p0 + t;
      const bool ok = p < npix;
      float xm[MAX_CM], g[NC], dm = 0.f;
#pragma unroll
      for (int c = 0; c < MAX_CM; ++c) xm[c] = 0.f;
#pragma unroll
      for (int o = 0; o < NC; ++o) g[o] = 0.f;
      if (ok) {
        long b, hw;
        pix_split(p, HW, b, hw);
#pragma unroll
        for (int c = 0; c < MAX_CM; ++c)
          if (c < Cm) xm[c] = meta[(b * Cm + c) * HW + hw];
#pragma unroll
        for (int o = 0; o < NC; ++o) g[o] = dl[(b * NC + o) * HW + hw];
      }
#pragma unroll
      for (int o = 0; o < NC; ++o) {
        sg[o][t] = g[o];
        gb_acc[o] += g[o];
        dm += g[o] * wv[o];
      }
      gb3_acc += dm;
      float h1[HID], dh1[HID];
#pragma unroll
      for (int j = 0; j < HID; ++j) {
        float a = b1[j];
#pragma unroll
        for (int c = 0; c < MAX_CM; ++c) a += w1[j * MAX_CM + c] * xm[c];
        h1[j] = ok ? fmaxf(a, 0.f) : 0.f;
        dh1[j] = 0.f;
      }
      float mval = b3[0];
#pragma unroll 2
      for (int j = 0; j < HID; ++j) {
        float a = b2[j];
#pragma unroll
        for (int i = 0; i < HID; ++i) a += w2[j * HID + i] * h1[i];
        const float h2j = ok ? fmaxf(a, 0.f) : 0.f;
        mval += w3[j] * h2j;
        const float dh2j = h2j > 0.f ? dm * w3[j] : 0.f;
#pragma unroll
        for (int i = 0; i < HID; ++i) dh1[i] += w2[j * HID + i] * dh2j;
        sd2[t][j] = dh2j;
        sm2[t][j] = dm * h2j;
      }
#pragma unroll
      for (int o = 0; o < NC; ++o) dwm_acc[o] += g[o] * mval;          // (g = 0 outside the tensor)
#pragma unroll
      for (int i = 0; i < HID; ++i) {
        sh1[t][i] = h1[i];
        sd1[t][i] = h1[i] > 0.f ? dh1[i] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < MAX_CM; ++c) sx[t][c] = xm[c];
      __syncthreads();
      // outer products over the block's 256 pixels
      for (int q = 0; q < 256; ++q) {
        const float dq = sd2[q][j2];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) a2[kk] += dq * sh1[q][i0 + kk];
      }
      if (t < HID * MAX_CM) {
        for (int q = 0; q < 256; ++q) a1 += sd1[q][j1] * sx[q][c1];
      }
      // vectors: threads 0..31 -> gb2, 32..63 -> gb1, 64..95 -> gw3
      if (t < HID) {
        for (int q = 0; q < 256; ++q) av += sd2[q][t];
      } else if (t < 2 * HID) {
        for (int q = 0; q < 256; ++q) av += sd1[q][t - HID];
      } else if (t < 3 * HID) {
        for (int q = 0; q < 256; ++q) av += sm2[q][t - 2 * HID];
      }
    }
    // phase B: the 64-channel head on the same 256 pixels
    for (int r0 = 0; r0 < 256; r0 += 32 * HMB_UNR) {
      float g[HMB_UNR][NC], v[HMB_UNR][8], yv[HMB_UNR][8];
      bool ok[HMB_UNR];
#pragma unroll
      for (int u = 0; u < HMB_UNR; ++u) {
        const int q = r0 + u * 32 + slot;
        const long pu = p0 + q;
        ok[u] = pu < npix;
        if (ok[u]) {
#pragma unroll
          for (int o = 0; o < NC; ++o) g[u][o] = sg[o][q];
          if (x) load8s(x + pu * x_ld + sub * 8, v[u]);
          if constexpr (BNB) load8s(reinterpret_cast<const T*>(bnb.y) + pu * bnb.y_ld + sub * 8, yv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < HMB_UNR; ++u) {
        if (!ok[u]) continue;
        const long pu = p0 + r0 + u * 32 + slot;
        float o8[8];
        if constexpr (BNB) {
          if (!x) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[u][j] = storage_round<TX>(fmaxf(yv[u][j] * k.sc[j] + k.sh[j], 0.f));
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float sum = 0.f;
#pragma unroll
          for (int o = 0; o < NC; ++o) { sum += g[u][o] * wr[o][j]; gw[o][j] += g[u][o] * v[u][j]; }
          o8[j] = sum;
        }
        if constexpr (BNB) {
#pragma unroll
          for (int j = 0; j < 8; ++j) o8[j] = storage_round<T>(o8[j]);      // the sums see dx as it is stored
        }
        store8(dx + pu * dx_ld + sub * 8, o8);
        if constexpr (BNB) bnb_accum_v(k, yv[u], o8, d1, d2);
      }
    }
    __syncthreads();              // the LDS rows and sg are rewritten by the next iteration
  }
  // workgroup partials -> global
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) atomicAdd(&gw2[j2 * HID + i0 + kk], a2[kk]);
  if (t < HID * MAX_CM && c1 < Cm) atomicAdd(&gw1[j1 * Cm + c1], a1);
  if (t < HID) atomicAdd(&gb2[t], av);
  else if (t < 2 * HID) atomicAdd(&gb1[t - HID], av);
  else if (t < 3 * HID) atomicAdd(&gw3[t - 2 * HID], av);
#pragma unroll
  for (int o = 0; o < NC; ++o)
#pragma unroll
    for (int j = 0; j < 8; ++j) atomicAdd(&lds_head[o * HEAD_C + sub * 8 + j], gw[o][j]);
  // column 64 of dW, the bias gradient, gb3: wave reduce, then LDS, then one atomic each
  float r[2 * NC + 1];
#pragma unroll
  for (int o = 0; o < NC; ++o) { r[o] = wave_sum(dwm_acc[o]); r[NC + o] = wave_sum(gb_acc[o]); }
  r[2 * NC] = wave_sum(gb3_acc);
  if ((t & 63) == 0)
    for (int o = 0; o <= 2 * NC; ++o) red[(t >> 6) * 16 + o] = r[o];
  __syncthreads();
  for (int i = t; i < NC * HEAD_C; i += 256) atomicAdd(&dw[(i / HEAD_C) * (HEAD_C + 1) + i % HEAD_C], lds_head[i]);
  if (t <= 2 * NC) {
    const float sum = red[t] + red[16 + t] + red[32 + t] + red[48 + t];
    if (t < NC) atomicAdd(&dw[t * (HEAD_C + 1) + HEAD_C], sum);
    else if (t < 2 * NC) atomicAdd(&db[t - NC], sum);
    else atomicAdd(&gb3[0], sum);
  }
  if constexpr (BNB) bnb_flush(bnb, lds_bnb, HEAD_C, sub * 8, d1, d2, 256);
}

// ---- metadata planes of a crop (batch/dataset.py:288-351, get_crop_memmap): the per-pixel formula is
// meta_plane_values (meta_planes.h), shared with the gather of crimac_gather_patches_memm_meta (tiling.hip) -----------------
struct MetaPlaneArgs {
  const int* centres;            // [P][2] (range idx, ping idx)
  int P, H, W;
  MetaPlaneSrc src;
  float* out;                    // [P][Cm][H][W]
  int Cm;
};

__global__ __launch_bounds__(256) void meta_planes_kernel(MetaPlaneArgs a) {
  const long HW = (long)a.H * a.W, total = (long)a.P * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int p = (int)(i / HW);
    const int rem = (int)(i - p * HW);
    const int y = rem / a.W, x = rem - y * a.W;
    MetaPlaneSrc s = a.src;
    if (!s.resolve(p)) continue;                 // (the table form: a patch without a source is skipped; no barrier here)
    float v[CRIMAC_MAX_META_PLANES];
    meta_plane_values(s, a.centres[2 * p], a.centres[2 * p + 1], a.H, a.W, y, x, v);
    float* o = a.out + ((long)p * a.Cm) * HW + rem;
    for (int c = 0; c < a.Cm; ++c) o[c * HW] = v[c];
  }
}
}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int crimac_meta_mlp_fwd(const float* meta, int Cm, int B, int H, int W, const float* w1, const float* b1,
                                   const float* w2, const float* b2, const float* w3, const float* b3, float* m,
                                   void* stream) {
  CRIMAC_REQUIRE(meta && w1 && b1 && w2 && b2 && w3 && b3 && m && B > 0 && H > 0 && W > 0, "meta_mlp_fwd: bad arguments");
  CRIMAC_REQUIRE(Cm >= 1 && Cm <= MAX_CM, "meta_mlp_fwd: %d metadata channels (1..%d supported)", Cm, MAX_CM);
  const long HW = (long)H * W, npix = B * HW;
  long blocks = (npix + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(meta_mlp_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, ST, meta, Cm, npix, HW,
                     MlpW{w1, b1, w2, b2, w3, b3}, m);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_meta_inject_fwd(const float* m, const float* wm, float* logits, int B, int H, int W, int ncls,
                                      int softmax, void* stream) {
  CRIMAC_REQUIRE(m && wm && logits && B > 0 && H > 0 && W > 0, "meta_inject_fwd: bad arguments");
  CRIMAC_REQUIRE(ncls >= 2 && ncls <= 4, "meta_inject_fwd: ncls=%d unsupported (2..4)", ncls);
  const long HW = (long)H * W, npix = B * HW;
  long blocks = (npix + 255) / 256;
  if (blocks > 2048) blocks = 2048;
#define MI(NC) hipLaunchKernelGGL(meta_inject_fwd_kernel<NC>, dim3((unsigned)blocks), dim3(256), 0, ST, m, wm, logits, npix, HW, softmax)
  if (ncls == 2) MI(2); else if (ncls == 3) MI(3); else MI(4);
#undef MI
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_meta_bwd(const float* dlogits, const float* meta, int Cm, int B, int H, int W, int ncls,
                               const float* wm, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* w3, const float* b3, float* dwm, float* gw1, float* gb1, float* gw2,
                               float* gb2, float* gw3, float* gb3, void* stream) {
  CRIMAC_REQUIRE(dlogits && meta && wm && w1 && b1 && w2 && b2 && w3 && b3 && dwm && gw1 && gb1 && gw2 && gb2 && gw3 &&
                     gb3 && B > 0 && H > 0 && W > 0,
                 "meta_bwd: bad arguments");
  CRIMAC_REQUIRE(Cm >= 1 && Cm <= MAX_CM, "meta_bwd: %d metadata channels (1..%d supported)", Cm, MAX_CM);
  CRIMAC_REQUIRE(ncls >= 2 && ncls <= 4, "meta_bwd: ncls=%d unsupported (2..4)", ncls);
  const long HW = (long)H * W, npix = B * HW;
  long blocks = (npix + 255) / 256;
  if (blocks > 512) blocks = 512;
  const MlpW w{w1, b1, w2, b2, w3, b3};
  const size_t lds = sizeof(float) * (((W_FLOATS + 3) & ~3) + 3 * 256 * (HID + 1) + 256 * (MAX_CM + 1) + 64);
  static unsigned long long attr_devs = 0;
  if (crimac_first_use_on_device(&attr_devs)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&meta_bwd_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&meta_bwd_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&meta_bwd_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
#define MB(NC) hipLaunchKernelGGL(meta_bwd_kernel<NC>, dim3((unsigned)blocks), dim3(256), lds, ST, dlogits, meta, Cm, npix, HW, wm, w, dwm, gw1, gb1, gw2, gb2, gw3, gb3)
  if (ncls == 2) MB(2); else if (ncls == 3) MB(3); else MB(4);
#undef MB
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}


// ---- the late-injection head's forward in one launch: crimac_head_fwd + crimac_meta_mlp_fwd + crimac_meta_inject_fwd on
// conv_final.weight [ncls][65] as it stands -----------------------------------------------------------------------------
#define HEAD_META_COMMON(name)                                                                                          \
  CRIMAC_REQUIRE(prec >= CRIMAC_PREC_BF16 && prec <= CRIMAC_PREC_MAX, name ": bad precision %d", prec);                  \
  CRIMAC_REQUIRE(Cm >= 1 && Cm <= MAX_CM, name ": %d metadata channels (1..%d supported)", Cm, MAX_CM);                  \
  CRIMAC_REQUIRE(ncls >= 2 && ncls <= 4, name ": ncls=%d unsupported (2..4)", ncls)

template <typename T, typename TR>
static int head_meta_fwd_launch(const void* x, long x_ld, const float* w, const float* b, const float* meta, int Cm,
                                const MlpW& mw, float* logits, long npix, long HW, int ncls, int softmax,
                                const float* bn_scale, const float* bn_shift, hipStream_t st) {
  long blocks = (npix + 255) / 256;
  if (blocks > 1024) blocks = 1024;
#define HMF(NC)                                                                                                       \
  hipLaunchKernelGGL((head_meta_fwd_kernel<T, NC, TR>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, x_ld, w, b, \
                     meta, Cm, mw, logits, npix, HW, softmax, bn_scale, bn_shift)
  if (ncls == 2) HMF(2); else if (ncls == 3) HMF(3); else HMF(4);
#undef HMF
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_head_meta_fwd(int prec, const void* x, long x_ld, const float* w, const float* b, const float* meta,
                                    int Cm, const float* w1, const float* b1, const float* w2, const float* b2,
                                    const float* w3, const float* b3, float* logits, int B, int H, int W, int ncls,
                                    int softmax, const float* bn_scale, const float* bn_shift, void* stream) {
  HEAD_META_COMMON("head_meta_fwd");
  CRIMAC_REQUIRE(x && w && b && meta && w1 && b1 && w2 && b2 && w3 && b3 && logits && B > 0 && H > 0 && W > 0,
                 "head_meta_fwd: bad arguments");
  CRIMAC_REQUIRE(x_ld >= HEAD_C && x_ld % 8 == 0, "head_meta_fwd: bad pixel stride %ld", x_ld);
  CRIMAC_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "head_meta_fwd: bn_scale and bn_shift go together");
  const long HW = (long)H * W, npix = B * HW;
  const MlpW mw{w1, b1, w2, b2, w3, b3};
  if (prec == CRIMAC_PREC_H3P) {        // (as crimac_head_fwd: the fp32 conv output + BatchNorm on the fly, or the plane pairs)
    if (bn_scale) return head_meta_fwd_launch<float, hp_t>(x, x_ld, w, b, meta, Cm, mw, logits, npix, HW, ncls, softmax, bn_scale, bn_shift, ST);
    return head_meta_fwd_launch<hp_t, hp_t>(x, x_ld, w, b, meta, Cm, mw, logits, npix, HW, ncls, softmax, bn_scale, bn_shift, ST);
  }
  CRIMAC_FOR_STORAGE(prec, T, return (head_meta_fwd_launch<T, T>(x, x_ld, w, b, meta, Cm, mw, logits, npix, HW, ncls, softmax,
                                                                 bn_scale, bn_shift, ST)));
}


template <typename T, typename TX, int NC, bool BNB>
static int head_meta_bwd_launch(const float* dl, const void* x, long x_ld, const float* w, void* dx, long dx_ld, float* dw,
                                float* db, const float* meta, int Cm, const MlpW& mw, float* const* g, long npix, long HW,
                                const BnbArgs& bnb, hipStream_t st) {
  long blocks = (npix + 255) / 256;
  if (blocks > 512) blocks = 512;
  const size_t lds = sizeof(float) * HMB_FLOATS;
  static unsigned long long attr_devs = 0;          // (one per instantiation)
  if (crimac_first_use_on_device(&attr_devs))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&head_meta_bwd_kernel<T, NC, BNB, TX>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL((head_meta_bwd_kernel<T, NC, BNB, TX>), dim3((unsigned)blocks), dim3(256), lds, st, dl, (const TX*)x,
                     x_ld, w, (T*)dx, dx_ld, dw, db, meta, Cm, mw, g[0], g[1], g[2], g[3], g[4], g[5], npix, HW, bnb);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_head_meta_bwd(int prec, const float* dlogits, const void* x, long x_ld, const float* w, void* dx,
                                    long dx_ld, float* dw, float* db, const float* meta, int Cm, const float* w1,
                                    const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                                    float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3, int B, int H,
                                    int W, int ncls, const void* bnb_y, long bnb_y_ld, const float* bnb_vec,
                                    long bnb_stride, double* stat_sum, double* stat_sumsq, int stat_replicas,
                                    void* stream) {
  HEAD_META_COMMON("head_meta_bwd");
  CRIMAC_REQUIRE(dlogits && w && dx && dw && db && meta && w1 && b1 && w2 && b2 && w3 && b3 && gw1 && gb1 && gw2 && gb2 &&
                     gw3 && gb3 && B > 0 && H > 0 && W > 0,
                 "head_meta_bwd: bad arguments");
  CRIMAC_REQUIRE(x || (bnb_y && stat_sum), "head_meta_bwd: x may only be NULL together with the fused BatchNorm sums");
  CRIMAC_REQUIRE((!x || (x_ld >= HEAD_C && x_ld % 8 == 0)) && dx_ld >= HEAD_C && dx_ld % 8 == 0,
                 "head_meta_bwd: bad pixel strides");
  CRIMAC_REQUIRE(bnb_args_ok(bnb_y, bnb_y_ld, bnb_vec, bnb_stride, stat_sum, stat_sumsq, stat_replicas, HEAD_C),
                 "head_meta_bwd: bad arguments of the fused BatchNorm-backward sums");
  const long HW = (long)H * W, npix = B * HW;
  const MlpW mw{w1, b1, w2, b2, w3, b3};
  float* const g[6] = {gw1, gb1, gw2, gb2, gw3, gb3};
  const BnbArgs bnb{bnb_y, bnb_y_ld, bnb_vec, bnb_stride, stat_sum, stat_sumsq, stat_replicas};
#define HMB(NC)                                                                                                          \
  (bnb.sum_dz ? head_meta_bwd_launch<T, TX, NC, true>(dlogits, x, x_ld, w, dx, dx_ld, dw, db, meta, Cm, mw, g, npix, HW, bnb, ST) \
              : head_meta_bwd_launch<T, TX, NC, false>(dlogits, x, x_ld, w, dx, dx_ld, dw, db, meta, Cm, mw, g, npix, HW, bnb, ST))
#define HMB_NC (ncls == 2 ? HMB(2) : ncls == 3 ? HMB(3) : HMB(4))
  // (the four storage forms crimac_head_bwd takes; CRIMAC_PREC_H3F_BWD is refused above: the head runs in the forward's mode)
  if (prec == CRIMAC_PREC_BF16) { using T = bf16_t; using TX = bf16_t; return HMB_NC; }
  if (prec == CRIMAC_PREC_FP16) { using T = half_t; using TX = half_t; return HMB_NC; }
  if (prec == CRIMAC_PREC_H3P) { using T = float; using TX = hp_t; return HMB_NC; }
  { using T = float; using TX = float; return HMB_NC; }
#undef HMB_NC
#undef HMB
}


// Metadata planes of P crops (reference batch/dataset.py:288-351, the `meta` half of get_crop_memmap's result): what the
// reference's Dataset builds per patch in numpy DataLoader workers, built on the GPU from the echogram's three per-ping
// vectors.  flags: bit 0 portion_year, 1 portion_day (two planes: sin, cos), 2 time_diff, 3 depth_rel,
// 4 depth_abs_surface, 5 depth_abs_seabed; the planes come out in that order, out [P][Cm][H][W] fp32.
static int meta_planes_run(const char* name, const MetaPlaneSrc& m, const int* centres, int P, int H, int W, float* out,
                           void* stream) {
  CRIMAC_REQUIRE(centres && out && P > 0 && H > 0 && W > 0 && m.flags > 0 && m.flags < 64, "%s: bad arguments", name);
  CRIMAC_REQUIRE(m.metas || !(m.flags & 2) || (m.portion_day && m.n_day > 0), "%s: portion_day needs its vector", name);
  CRIMAC_REQUIRE(m.metas || !(m.flags & 4) || (m.time_diff && m.n_td > 0), "%s: time_diff needs its vector", name);
  CRIMAC_REQUIRE(m.metas || !(m.flags & 56) || (m.seabed && m.n_sb > 0), "%s: the depth planes need the seabed vector", name);
  MetaPlaneArgs a{centres, P, H, W, m, out, meta_plane_count(m.flags)};
  const long total = (long)P * H * W;
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(meta_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_meta_planes(const int* centres, int P, int H, int W, int flags, double portion_year,
                                  const double* portion_day, int n_day, const double* time_diff, int n_td,
                                  const long long* seabed, int n_sb, float* out, void* stream) {
  return meta_planes_run("meta_planes", MetaPlaneSrc{flags, portion_year, portion_day, n_day, time_diff, n_td, seabed, n_sb},
                         centres, P, H, W, out, stream);
}

// crimac_meta_planes for batches that span memmap echograms: the scalar and the vectors of patch p from metas[src[p]].
extern "C" int crimac_meta_planes_multi(const crimac_memm_meta_desc* metas, int n_desc, const int* src, const int* centres,
                                        int P, int H, int W, int flags, float* out, void* stream) {
  CRIMAC_REQUIRE(metas && src && n_desc > 0, "meta_planes_multi: needs the metadata table and src");
  return meta_planes_run("meta_planes_multi", MetaPlaneSrc{flags, 0.0, nullptr, 0, nullptr, 0, nullptr, 0, metas, n_desc, src},
                         centres, P, H, W, out, stream);
}
