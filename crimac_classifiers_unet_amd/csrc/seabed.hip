// Seabed-line estimate of a memmap echogram on the GPU (CDNA4 / gfx950): the streaming part of the reference's
// Echogram.get_seabed (data/data_reader.py:433-507) for an echogram without a stored seabed.npy.
//
// Reference, per frequency plane d [range][ping] (non-finite samples set to 0 first, :449-451, :465):
//   grad_1 = convolve2d(d, [[1,2,1],[0,0,0],[-1,-2,-1]], 'same'),  grad_2 = convolve2d(d, [[1,5,1],[-2,-10,-2],[1,5,1]], 'same')
//   (true convolutions: the filters are flipped, zero padding; float32 data x int64 filter -> float64 sums), i.e. with
//     S1(r) = d[r][p-1] + 2 d[r][p] + d[r][p+1]        S2(r) = d[r][p-1] + 5 d[r][p] + d[r][p+1]
//     grad_1[r][p] = S1(r+1) - S1(r-1)                 grad_2[r][p] = S2(r-1) - 2 S2(r) + S2(r+1)
//   score = heaviside(grad_1, 0) * grad_2;   argmax(score[n:, p]) (first occurrence)            (:453-458, :468)
//   sb_max = max(d[n:, p])                                                                      (:476)
// One wave per (frequency, ping) column of the chunk layout [F][Pc][R] (range contiguous): lanes stride the range and
// read the three neighbouring columns (coalesced; the rows r - 1 and r + 1 come from the L1 lines the row r loads
// brought in), each lane keeps a running (score, row) pair, and a butterfly reduction breaks ties towards the lower row.
// Every product (x 2, x 5 in fp64 of a float32 value) is exact, so fused multiply-adds change nothing; the order of the
// additions is the one written here (tests/test_gpu_seabed.py restates it in numpy).
#include "common.h"

namespace {

constexpr int kWaves = 4;          // columns (waves) per workgroup: consecutive pings of one frequency share their L1 lines

__device__ __forceinline__ double clean(const float* __restrict__ col, int r) {
  const float v = col[r];
  return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 0.0 : (double)v;      // inf / NaN -> 0
}

struct RowSums { double s1, s2; };

// S1 / S2 of row r of the column `c` with neighbours `l`, `rt` (nullptr: outside the echogram, zeros); r outside
// [0, R): zeros.
__device__ __forceinline__ RowSums row_sums(const float* __restrict__ l, const float* __restrict__ c,
                                            const float* __restrict__ rt, int r, int R) {
  if (r < 0 || r >= R) return {0.0, 0.0};
  const double a = l ? clean(l, r) : 0.0, b = clean(c, r), d = rt ? clean(rt, r) : 0.0;
  return {(a + 2.0 * b) + d, (a + 5.0 * b) + d};
}

__global__ __launch_bounds__(kWaves * 64) void seabed_columns_kernel(
    const float* __restrict__ data, long Pc, int R, int first, long owned, int n, int* __restrict__ idx,
    float* __restrict__ colmax, long out_ld, long groups) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = blockIdx.x / groups;
  const long j = (blockIdx.x - f * groups) * kWaves + wave;          // owned ping of this wave (wave-uniform)
  if (j >= owned) return;
  const long p = first + j;                                          // its column in the chunk
  const float* c = data + (f * Pc + p) * (long)R;
  const float* l = p > 0 ? c - R : nullptr;
  const float* rt = p + 1 < Pc ? c + R : nullptr;
  double best = -__builtin_inf();
  int best_r = 0x7fffffff;
  float mx = -__builtin_inff();
  for (int r = n + lane; r < R; r += 64) {
    const RowSums up = row_sums(l, c, rt, r - 1, R), me = row_sums(l, c, rt, r, R), dn = row_sums(l, c, rt, r + 1, R);
    const double g1 = dn.s1 - up.s1;
    const double g2 = (up.s2 - 2.0 * me.s2) + dn.s2;
    const double score = g1 > 0.0 ? g2 : 0.0;
    if (score > best) { best = score; best_r = r; }                  // (rows ascend per lane: the first maximum stays)
    const float v = c[r];
    mx = fmaxf(mx, (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 0.f : v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int orow = __shfl_xor(best_r, o, 64);
    if (ob > best || (ob == best && orow < best_r)) { best = ob; best_r = orow; }
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    idx[f * out_ld + j] = best_r - n;
    colmax[f * out_ld + j] = mx;
  }
}

}  // namespace

extern "C" int crimac_seabed_columns(const float* data, int F, long Pc, int R, int has_left, int has_right, int n,
                                     int* idx, float* colmax, long out_ld, void* stream) {
  CRIMAC_REQUIRE(data && idx && colmax && F > 0 && Pc > 0 && R > 0, "seabed_columns: bad arguments");
  CRIMAC_REQUIRE(n >= 0 && n < R, "seabed_columns: row offset n=%d outside [0, R=%d)", n, R);
  CRIMAC_REQUIRE((has_left == 0 || has_left == 1) && (has_right == 0 || has_right == 1),
                 "seabed_columns: the halo flags are 0 or 1");
  const long owned = Pc - has_left - has_right;
  CRIMAC_REQUIRE(owned > 0, "seabed_columns: a chunk of %ld pings with %d halo pings owns none", Pc, has_left + has_right);
  CRIMAC_REQUIRE(out_ld >= owned, "seabed_columns: out_ld=%ld < %ld owned pings", out_ld, owned);
  const long groups = (owned + kWaves - 1) / kWaves;
  CRIMAC_REQUIRE(groups * F <= 2147483647L, "seabed_columns: too many columns for one launch");
  hipLaunchKernelGGL(seabed_columns_kernel, dim3((unsigned)(groups * F)), dim3(kWaves * 64), 0, (hipStream_t)stream,
                     data, Pc, R, has_left, owned, n, idx, colmax, out_ld, groups);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}
