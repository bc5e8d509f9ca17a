// Echo integration by predicted class (CDNA4 / gfx950): the reduction of a finished prediction chunk.
//
// The reference stops at the saved [2][range][pings] float16 probabilities (save_predict.py:212, :252); the next step of
// a survey -- sum the linear sv of one frequency over the pixels assigned to a class, per cell of (ping bin x range bin)
// -- is done downstream on the host.  Here both operands are already resident: pred [2][n_range][n_pings] (what
// crimac_scatter_patches_ex wrote, ping contiguous) and one frequency plane sv [data_pings][n_range] of the chunk's data
// (range contiguous).
//
// A stream of 8-12 bytes per pixel with one transposed operand.  ONE kernel body and one finish kernel serve every entry
// point: integrate_freqs_kernel<TP, VEC_SV, VEC_PRED, SEABED, NF> holds the accumulators of NF frequency planes, and
// crimac_integrate_classes / _layers / _edges are its NF = 1 instantiations on one plane (launch_pass1 is the one place
// that turns (pred_f16, seabed, vec_sv, vec_pred, n_freqs) into an instantiation).  Pass 1: a workgroup owns (cell, split):
// it walks tiles split, split + S, ... of the cell's 64 x 64 tiles (pings fastest).  Per tile the sv rows go through an LDS
// tile [64 pings][64 rows + 1] -- read from global along the range, read back along the pings -- while pred is read from
// global along the pings by the thread that consumes it, so both global reads are coalesced (16 bytes per lane when the
// extents and the base addresses allow it, 4 bytes otherwise).  sv outside the cell is staged as 0, which the pixel rule
// (finite and > 0) then drops like any other empty sample.  Each thread keeps fp64 sums and 64-bit counts over its tiles in
// tile order; lanes are combined by a butterfly, the four waves in wave order by thread 0, and the six results go to the
// (cell, split) slot of the scratch.  Pass 2 (integrate_finish_kernel): one thread per (frequency, cell) adds its S slots in
// split order and does a plain read-add-write of the cell's six outputs.  No atomics anywhere: launches that touch the same
// cell are ordered by the stream, S depends on the shapes alone, so the result is bit-reproducible for a given chunking.
//
// crimac_integrate_layers (the SEABED instantiations of the same kernel): ping p of the launch has a row limit
// L[p] = clamp(seabed[p] + seabed_offset, 0, n_range) and rows >= L[p] count nowhere.  Surface reference: the cells above,
// each ping's rows cut at its limit.  Seabed reference: column l of the accumulator is layer l, rows [L[p] - (l + 1) *
// range_bin, L[p] - l * range_bin) of ping p -- counted from the limit, so the layer follows the relief.  The workgroup
// stays (ping bin, layer, split): it first reduces min and max of L over its ping span, walks the tiles of that row
// bounding box and keeps a pixel when its row lies in its ping's own interval [lo, hi), which the tile's 64 pings hold in
// LDS (written once per tile, read into registers by the four pings a thread consumes).  With relief above range_bin the
// boxes of neighbouring layers overlap and those tiles are read once per layer.  S is bounded by the tiles of the whole
// column, whatever the seabed values: a workgroup whose split finds no tile writes a zero slot.
//
// crimac_integrate_freqs (NF = 1, 4 or CRIMAC_INTEGRATE_MAX_FREQS by n_freqs): several planes of one source in one pass over
// the predictions; see the kernel.
//
// crimac_integrate_edges (the same kernels once more): the ping extent of cell pb is [edges[pb], edges[pb + 1]) of a device
// table instead of [pb * ping_bin, (pb + 1) * ping_bin).  The workgroup reads its two edges in the prologue (cell_of), where
// the index depends on blockIdx alone -- two scalar loads per workgroup, nothing per pixel.  The host reads its own copy of
// the table for the cells the launch touches and their widest extent, which bounds S as ping_bin does.
//
// crimac_integrate_confusion (further down, its own two kernels): the sums of an EVALUATION batch -- logits, raw crops and
// transformed labels in patch layout -- split by the annotated class as well; crimac_integrate_confusion_multi: the same
// two kernels for a batch packed from several echograms.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "pr_softmax.h"

namespace {

constexpr int kTile = 64;                 // tile edge, pings and rows
constexpr int kPitch = kTile + 1;         // LDS row pitch in floats: the transposed read walks banks, not one bank
constexpr int kThreads = 256;
struct Slot { double sum[3]; long long cnt[3]; };
static_assert(sizeof(Slot) == CRIMAC_INTEGRATE_SLOT_BYTES, "scratch slot size is part of the ABI");

struct Geom {
  int n_range, range_bin, n_rb, splits, mode;
  long n_pings, sv_ping_off, ping_bin, ping_origin, n_pb_total, pb0;
  float thr0, thr1;
  // crimac_integrate_layers: the seabed line from the launch's ping 0 on, the offset of the limit, 0 surface / 1 seabed
  const int* seabed;
  int seabed_offset, reference;
  // crimac_integrate_edges: cell pb covers global pings [edges[pb], edges[pb + 1]); null: pb * ping_bin
  const long long* edges;
};

// the cell's extent in the launch's coordinates (rows; pings relative to pred column 0), clipped to the launch
struct Cell { int r0, r1; long p0, p1; };
__device__ __forceinline__ Cell cell_of(const Geom& g, long cell) {
  const long pb = g.pb0 + cell / g.n_rb;
  const int rb = (int)(cell % g.n_rb);
  Cell c;
  c.r0 = rb * g.range_bin;
  const long r1 = (long)c.r0 + g.range_bin;
  long p0, p1;
  if (g.edges) {                                                // (uniform: pb comes from blockIdx)
    p0 = (long)g.edges[pb] - g.ping_origin;
    p1 = (long)g.edges[pb + 1] - g.ping_origin;
  } else {
    p0 = pb * g.ping_bin - g.ping_origin;
    p1 = p0 + g.ping_bin;
  }
  c.r1 = (int)(r1 < g.n_range ? r1 : g.n_range);
  c.p0 = p0 > 0 ? p0 : 0;
  c.p1 = p1 < g.n_pings ? p1 : g.n_pings;
  return c;
}

// L[p]: the first row of ping p (relative to the launch) that counts nowhere
__device__ __forceinline__ int row_limit(const Geom& g, long p) {
  const long v = (long)g.seabed[p] + g.seabed_offset;
  return (int)(v < 0 ? 0 : v < g.n_range ? v : g.n_range);
}

template <typename TP> __device__ __forceinline__ float widen(TP v) { return (float)v; }

// four consecutive pings (VEC: one 16- or 8-byte load) or pings l, l + 16, l + 32, l + 48 of one row; 0 outside the array
template <typename TP, bool VEC>
__device__ __forceinline__ void load_pred(const TP* __restrict__ row, long p, long n_pings, float (&v)[4]) {
  if constexpr (VEC) {
    typedef TP vec4 __attribute__((ext_vector_type(4)));
    if (p < n_pings) {                                   // (p and n_pings are multiples of 4: all four or none)
      const vec4 x = __builtin_nontemporal_load(reinterpret_cast<const vec4*>(row + p));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = widen(x[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p + 16 * j < n_pings ? widen(__builtin_nontemporal_load(row + p + 16 * j)) : 0.f;
  }
}

// ---- the steps of a workgroup of integrate_freqs_kernel -------------------------------------------------------------------
// SEABED prologue of a workgroup: min and max of L over the cell's ping span cut the cell's rows to the box that can hold
// a counted pixel.  Returns `top`: with the seabed reference the layer ends `top` rows above the limit (0 otherwise).
__device__ __forceinline__ long seabed_box(const Geom& g, Cell& c, long cell, int t) {
  __shared__ int span_min[kThreads / 64], span_max[kThreads / 64];
  const int lane = t & 63, wave = t >> 6;
  long top = 0;
  int lmin = g.n_range, lmax = 0;                               // (every limit lies in [0, n_range])
  for (long p = c.p0 + t; p < c.p1; p += kThreads) {
    const int L = row_limit(g, p);
    lmin = L < lmin ? L : lmin;
    lmax = L > lmax ? L : lmax;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(lmin, o, 64), b = __shfl_xor(lmax, o, 64);
    lmin = a < lmin ? a : lmin;
    lmax = b > lmax ? b : lmax;
  }
  if (lane == 0) span_min[wave] = lmin, span_max[wave] = lmax;
  __syncthreads();
  for (int w = 0; w < kThreads / 64; ++w) {
    lmin = span_min[w] < lmin ? span_min[w] : lmin;
    lmax = span_max[w] > lmax ? span_max[w] : lmax;
  }
  if (g.reference == 1) {                                       // the row bounding box of the layer over the ping span
    top = (cell % g.n_rb) * g.range_bin;
    const long b0 = lmin - top - g.range_bin, b1 = lmax - top;
    c.r0 = (int)(b0 > 0 ? b0 : 0);
    c.r1 = (int)(b1 > 0 ? b1 : 0);
  } else {
    c.r1 = c.r1 < lmax ? c.r1 : lmax;                           // no ping of the span counts a row below
  }
  return top;
}

// SEABED: the rows [lo, hi) of ping p that count in the workgroup's cell (cell_r0, cell_r1: its rows before seabed_box)
__device__ __forceinline__ void row_interval(const Geom& g, long p, long top, int cell_r0, int cell_r1, int& lo, int& hi) {
  const long L = row_limit(g, p);
  if (g.reference == 1) {
    lo = (int)(L - top - g.range_bin > 0 ? L - top - g.range_bin : 0);
    hi = (int)(L - top > 0 ? L - top : 0);
  } else {
    lo = cell_r0;
    hi = (int)(L < cell_r1 ? L : cell_r1);
  }
}

// sv of the tile at (row tr, ping tp): global (along the range) -> registers; 0 outside the cell and outside the array
template <bool VEC_SV>
__device__ __forceinline__ void load_sv_tile(const float* __restrict__ sv, const Geom& g, const Cell& c, int tr, long tp, int t,
                                             float (&svr)[16]) {
  if constexpr (VEC_SV) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = t + kThreads * k, r = tr + 4 * (i & 15);
      const long p = tp + (i >> 4);
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (r < c.r1 && p >= c.p0 && p < c.p1)                  // (r, n_range multiples of 4: r < r1 <= n_range -> r + 3 < n_range)
        x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sv + (g.sv_ping_off + p) * g.n_range + r));
#pragma unroll
      for (int j = 0; j < 4; ++j) svr[4 * k + j] = (r + j >= c.r0 && r + j < c.r1) ? x[j] : 0.f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int i = t + kThreads * k, r = tr + (i & 63);
      const long p = tp + (i >> 6);
      svr[k] = (r >= c.r0 && r < c.r1 && p >= c.p0 && p < c.p1)
                   ? __builtin_nontemporal_load(sv + (g.sv_ping_off + p) * g.n_range + r) : 0.f;
    }
  }
}

// ... registers -> LDS tile [ping][row]
template <bool VEC_SV>
__device__ __forceinline__ void stage_sv_tile(float* tile, int t, const float (&svr)[16]) {
  if constexpr (VEC_SV) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = t + kThreads * k;
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(i >> 4) * kPitch + 4 * (i & 15) + j] = svr[4 * k + j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int i = t + kThreads * k;
      tile[(i >> 6) * kPitch + (i & 63)] = svr[k];
    }
  }
}

// a thread's six results: lanes by a butterfly, the waves in wave order by thread 0, into one slot of the scratch
__device__ __forceinline__ void reduce_to_slot(double s0, double s1, double s2, long long n0, long long n1, long long n2,
                                               Slot* wave_part, int t, Slot* __restrict__ out_slot) {
  const int lane = t & 63, wave = t >> 6;
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n0 += __shfl_xor(n0, o, 64);
    n1 += __shfl_xor(n1, o, 64);
    n2 += __shfl_xor(n2, o, 64);
  }
  if (lane == 0) wave_part[wave] = Slot{{s0, s1, s2}, {n0, n1, n2}};
  __syncthreads();
  if (t == 0) {
    Slot out = wave_part[0];
    for (int w = 1; w < kThreads / 64; ++w)
      for (int k = 0; k < 3; ++k) {
        out.sum[k] += wave_part[w].sum[k];
        out.cnt[k] += wave_part[w].cnt[k];
      }
    *out_slot = out;
  }
}

// ---- pass 1 of every entry point: the reduction for the launch's 1 .. NF frequency planes in one pass over the predictions
// The workgroup is (cell, split).  Per tile the predictions are read once and turned into the two class weights of each of
// the thread's 16 pixels (threshold mode: 1 or 0; probability mode: the stored value, 0 for a NaN or negative one), the
// seabed forms read their pings' row intervals once; then the sv tile of each frequency goes through LDS in turn and lands
// in that frequency's own six accumulators.  Two LDS tile buffers, used alternately, leave ONE barrier per (tile,
// frequency): a thread that writes buffer b again has passed the barrier of the stage in between, which every thread
// reaches only after it has read b; where registers allow it (kPrefetch) the global loads of the next frequency are issued
// right after the barrier and fly while the tile is consumed.  The accumulators are indexed by the unrolled frequency loop
// only, so they stay in registers.  A pixel adds `in ? sv * w : 0` to a class sum (w = 1 gives sv exactly), in tile, pixel,
// lane, wave and split order, whatever NF: frequency i of crimac_integrate_freqs gets the bits crimac_integrate_classes /
// _layers / _edges (NF = 1, plane offset 0) give on its plane.  Its slots are scratch[i * slots + blockIdx.x].
constexpr int kMaxFreqs = CRIMAC_INTEGRATE_MAX_FREQS;
struct Planes {
  int n;                   // frequencies of the launch
  long slots;              // cells * splits: the slots of one frequency
  long off[kMaxFreqs];     // elements from sv (plane 0) to the plane of frequency i
};

template <typename TP, bool VEC_SV, bool VEC_PRED, bool SEABED, int NF>
__global__ __launch_bounds__(kThreads) void integrate_freqs_kernel(const TP* __restrict__ pred, const float* __restrict__ sv,
                                                                   Geom g, Planes fq, Slot* __restrict__ scratch) {
  __shared__ float tile[2][kTile * kPitch];
  __shared__ Slot wave_part[kThreads / 64];
  __shared__ int row_lo[2][SEABED ? kTile : 1], row_hi[2][SEABED ? kTile : 1];
  const int t = threadIdx.x;
  const long cell = blockIdx.x / g.splits;
  const int split = (int)(blockIdx.x - cell * g.splits);
  Cell c = cell_of(g, cell);
  const int cell_r0 = c.r0, cell_r1 = c.r1;
  long top = 0;
  if constexpr (SEABED) top = seabed_box(g, c, cell, t);
  const int ra = c.r0 & ~3;
  const long pa = c.p0 & ~3L;
  const int nrt = c.r1 > c.r0 ? (c.r1 - ra + kTile - 1) / kTile : 0;
  const long npt = c.p1 > c.p0 ? (c.p1 - pa + kTile - 1) / kTile : 0;
  const long tiles = nrt * npt;
  const TP* pred0 = pred;
  const TP* pred1 = pred + (long)g.n_range * g.n_pings;
  const int row_in_group = t >> 4, l16 = t & 15;
  double s0[NF], s1[NF], s2[NF];
  long long n0[NF], n1[NF], n2[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) s0[f] = s1[f] = s2[f] = 0.0, n0[f] = n1[f] = n2[f] = 0;
  int stage = 0;                                              // LDS buffer of the next (tile, frequency): stage & 1

  for (long tl = split; tl < tiles; tl += g.splits) {
    const int tr = ra + (int)(tl / npt) * kTile;
    const long tp = pa + (tl % npt) * kTile;
    float svr[16];
    load_sv_tile<VEC_SV>(sv + fq.off[0], g, c, tr, tp, t, svr);
    // ---- pred -> the class weights of the 4 rows x 4 pings this thread consumes, once for all frequencies
    float w0[4][4], w1[4][4];
    const long pp = tp + (VEC_PRED ? 4 * l16 : l16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = tr + row_in_group + 16 * k;
      if (r < c.r1) {
        load_pred<TP, VEC_PRED>(pred0 + (long)r * g.n_pings, pp, g.n_pings, w0[k]);
        load_pred<TP, VEC_PRED>(pred1 + (long)r * g.n_pings, pp, g.n_pings, w1[k]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w0[k][j] = w1[k][j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a = w0[k][j], b = w1[k][j];
        if (g.mode == 0) {
          w0[k][j] = a >= g.thr0 ? 1.f : 0.f;
          w1[k][j] = b >= g.thr1 ? 1.f : 0.f;
        } else {
          w0[k][j] = a > 0.f ? a : 0.f;                       // (a NaN or negative weight counts as 0)
          w1[k][j] = b > 0.f ? b : 0.f;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    int lo = 0, hi = 0;                                       // SEABED: the rows of ping tp + t that count here
    if constexpr (SEABED) {
      if (t < kTile && tp + t >= c.p0 && tp + t < c.p1) row_interval(g, tp + t, top, cell_r0, cell_r1, lo, hi);
    }
    int plo[4], phi[4];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      if (f < fq.n) {                                         // (uniform)
        const int b = stage & 1;
        ++stage;
        if constexpr (SEABED) {
          if (f == 0 && t < kTile) row_lo[b][t] = lo, row_hi[b][t] = hi;
        }
        // the 16-byte form with few accumulators has registers to spare: the next plane's loads fly while this tile is consumed
        constexpr bool kPrefetch = VEC_SV && NF <= 4;
        if (!kPrefetch && f > 0) load_sv_tile<VEC_SV>(sv + fq.off[f], g, c, tr, tp, t, svr);
        stage_sv_tile<VEC_SV>(tile[b], t, svr);
        __syncthreads();
        if (kPrefetch && f + 1 < NF && f + 1 < fq.n) load_sv_tile<VEC_SV>(sv + fq.off[f + 1 < NF ? f + 1 : f], g, c, tr, tp, t, svr);
        if constexpr (SEABED) {
          if (f == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int pl = VEC_PRED ? 4 * l16 + j : l16 + 16 * j;
              plo[j] = row_lo[b][pl] - tr;                    // (relative to the tile's first row)
              phi[j] = row_hi[b][pl] - tr;
            }
          }
        }
        // ---- the pixel rule on this frequency's own sv
        int m0 = 0, m1 = 0, m2 = 0;                           // (counted pixels of the tile: 16 at most)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int rl = row_in_group + 16 * k;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int pl = VEC_PRED ? 4 * l16 + j : l16 + 16 * j;
            const float s = tile[b][pl * kPitch + rl];
            bool ok = s > 0.f && s < __builtin_inff();        // finite and > 0 (NaN fails both)
            if constexpr (SEABED) ok = ok && rl >= plo[j] && rl < phi[j];
            const float a = w0[k][j], b1 = w1[k][j];
            const double sd = ok ? (double)s : 0.0;
            const bool in0 = ok && a > 0.f, in1 = ok && b1 > 0.f;
            s0[f] += in0 ? sd * (double)a : 0.0;
            s1[f] += in1 ? sd * (double)b1 : 0.0;
            s2[f] += sd;
            m0 += in0;
            m1 += in1;
            m2 += ok;
          }
          __builtin_amdgcn_sched_barrier(0);                  // (four pixels at a time: their compare masks live in SGPRs)
        }
        n0[f] += m0;
        n1[f] += m1;
        n2[f] += m2;
      }
    }
  }
  // ---- lane -> wave -> workgroup per frequency, each in a fixed order
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if (f < fq.n) {
      if (f > 0) __syncthreads();                             // (thread 0 has read wave_part)
      reduce_to_slot(s0[f], s1[f], s2[f], n0[f], n1[f], n2[f], wave_part, t, scratch + f * fq.slots + blockIdx.x);
    }
  }
}

// Pass 2 of every entry point, one thread per (frequency, cell): the slots of that frequency in split order, then the plain
// read-add-write into its [3][n_pb_total][n_rb] slice.  One frequency: n = 1, f = 0 and the grid is ceil(cells / 256).
__global__ __launch_bounds__(kThreads) void integrate_finish_kernel(const Slot* __restrict__ scratch, Geom g, int n, long cells,
                                                                    double* __restrict__ acc, long long* __restrict__ cnt) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= cells * n) return;
  const long f = i / cells, cell = i - f * cells;
  const Slot* __restrict__ slots = scratch + (f * cells + cell) * g.splits;      // (a frequency's slots: cells * splits)
  Slot out = slots[0];
  for (int s = 1; s < g.splits; ++s)
    for (int k = 0; k < 3; ++k) {
      out.sum[k] += slots[s].sum[k];
      out.cnt[k] += slots[s].cnt[k];
    }
  const long pb = g.pb0 + cell / g.n_rb, rb = cell % g.n_rb;
  for (int k = 0; k < 3; ++k) {
    const long at = (((long)f * 3 + k) * g.n_pb_total + pb) * g.n_rb + rb;
    acc[at] += out.sum[k];
    cnt[at] += out.cnt[k];
  }
}

// what crimac_integrate_layers adds to the arguments of crimac_integrate_classes (null: that entry point)
struct SeabedArgs { const int* line; long first, len; int offset, reference, n_layers; };

// what crimac_integrate_edges gives in place of ping_bin (null: the uniform entry points)
struct EdgeArgs { const long long* dev; const long long* host; };

// what crimac_integrate_freqs adds: the planes of the source and the selected ones (null: one plane, the other entry points)
struct FreqArgs { long plane_stride; int n_planes; const int* channels; int n_freqs; };

// a run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{})
template <typename F> void with_flag(bool b, F&& f) { b ? f(std::true_type{}) : f(std::false_type{}); }

// Pass 1 of every entry point: (pred_f16, seabed, vec_sv, vec_pred) -> the instantiation of integrate_freqs_kernel, and NF by
// the accumulators it holds: 1 (the single-frequency entry points), 4 (the models' four) or CRIMAC_INTEGRATE_MAX_FREQS.
void launch_pass1(bool pred_f16, bool seabed, bool vec_sv, bool vec_pred, unsigned blocks, hipStream_t st, const void* pred,
                  const float* sv, const Geom& g, const Planes& fq, Slot* scratch) {
  with_flag(pred_f16, [&](auto f16) { with_flag(seabed, [&](auto sb) { with_flag(vec_sv, [&](auto vs) { with_flag(vec_pred, [&](auto vp) {
    using TP = std::conditional_t<decltype(f16)::value, half_t, float>;
    constexpr bool SB = decltype(sb)::value, VS = decltype(vs)::value, VP = decltype(vp)::value;
    const TP* p = static_cast<const TP*>(pred);
    const dim3 grid(blocks), block(kThreads);
    if (fq.n == 1) hipLaunchKernelGGL((integrate_freqs_kernel<TP, VS, VP, SB, 1>), grid, block, 0, st, p, sv, g, fq, scratch);
    else if (fq.n <= 4) hipLaunchKernelGGL((integrate_freqs_kernel<TP, VS, VP, SB, 4>), grid, block, 0, st, p, sv, g, fq, scratch);
    else hipLaunchKernelGGL((integrate_freqs_kernel<TP, VS, VP, SB, kMaxFreqs>), grid, block, 0, st, p, sv, g, fq, scratch);
  }); }); }); });
}

// The cells [pb0, pb1] of a checked host table that global pings [a, b) touch (pb1 < pb0: none) and their widest extent.
void cells_touched(const long long* e, long n_pb, long a, long b, long& pb0, long& pb1, long& widest) {
  const long long* first = std::upper_bound(e, e + n_pb + 1, (long long)a);     // the first edge > a
  const long long* last = std::lower_bound(e, e + n_pb + 1, (long long)b);      // the first edge >= b
  pb0 = first == e ? 0 : (long)(first - e) - 1;
  pb1 = (long)(last - e) - 1;
  pb1 = pb1 < n_pb - 1 ? pb1 : n_pb - 1;
  widest = 0;
  for (long pb = pb0; pb <= pb1; ++pb) widest = e[pb + 1] - e[pb] > widest ? (long)(e[pb + 1] - e[pb]) : widest;
}

// All four entry points: the argument checks, the geometry, the two launches.  `who` names the caller in the messages.
int integrate(const char* who, const SeabedArgs* sb, const EdgeArgs* ed, const FreqArgs* fa, const void* pred, int pred_f16, int n_range, long n_pings,
              const float* sv, long data_pings, long sv_ping_off, float thr_sandeel, float thr_other, int mode, long ping_bin,
              int range_bin, long ping_origin, long n_pb_total, double* acc, long long* cnt, void* scratch,
              long scratch_bytes, void* stream) {
  CRIMAC_REQUIRE(pred && sv && acc && cnt && scratch && (!fa || fa->channels), "%s: null pointer", who);
  if (fa) {
    CRIMAC_REQUIRE(fa->n_freqs >= 1 && fa->n_freqs <= kMaxFreqs, "%s: n_freqs=%d (1 .. CRIMAC_INTEGRATE_MAX_FREQS = %d)", who,
                   fa->n_freqs, kMaxFreqs);
    CRIMAC_REQUIRE(fa->n_planes >= 1, "%s: n_planes=%d", who, fa->n_planes);
    for (int i = 0; i < fa->n_freqs; ++i)
      CRIMAC_REQUIRE(fa->channels[i] >= 0 && fa->channels[i] < fa->n_planes, "%s: channels[%d]=%d of %d sv planes", who, i,
                     fa->channels[i], fa->n_planes);
  }
  CRIMAC_REQUIRE(pred_f16 == 0 || pred_f16 == 1, "%s: pred_f16 is 0 or 1", who);
  CRIMAC_REQUIRE(n_range > 0 && n_pings > 0, "%s: empty prediction array (%d x %ld)", who, n_range, n_pings);
  CRIMAC_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0 threshold, 1 probability)", who, mode);
  CRIMAC_REQUIRE(thr_sandeel > 0.f && thr_other > 0.f, "%s: thr = (%g, %g) must be > 0 (pixels the scatter "
                 "left at 0 belong to no class)", who, (double)thr_sandeel, (double)thr_other);
  CRIMAC_REQUIRE((ed || ping_bin > 0) && range_bin > 0, "%s: ping_bin=%ld, range_bin=%d must be positive", who, ping_bin,
                 range_bin);
  CRIMAC_REQUIRE(ping_bin <= 2147483647L && n_pb_total <= 2147483647L, "%s: ping_bin=%ld, n_pb_total=%ld "
                 "beyond 2^31 - 1", who, ping_bin, n_pb_total);
  CRIMAC_REQUIRE(sv_ping_off >= 0 && sv_ping_off + n_pings <= data_pings, "%s: sv columns [%ld, %ld) outside "
                 "the sv extent of %ld pings", who, sv_ping_off, sv_ping_off + n_pings, data_pings);
  CRIMAC_REQUIRE(ping_origin >= 0 && n_pb_total > 0 && (ed || ping_origin + n_pings <= n_pb_total * ping_bin),
                 "%s: pings [%ld, %ld) outside the accumulator's %ld bins of %ld pings", who, ping_origin,
                 ping_origin + n_pings, n_pb_total, ping_bin);
  // the source is n_planes planes of plane_stride elements: a plane [data_pings][n_range] must end inside its own stride
  CRIMAC_REQUIRE(!fa || (data_pings <= 9223372036854775807L / n_range && fa->plane_stride >= data_pings * n_range),
                 "%s: plane_stride=%ld: a plane of %ld pings x %d rows would leave the sv extent of %d planes", who,
                 fa ? fa->plane_stride : 0L, data_pings, n_range, fa ? fa->n_planes : 0);
  long pb0 = 0, pb1 = 0, widest = ping_bin;
  if (ed) {
    CRIMAC_REQUIRE(ed->dev && ed->host, "%s: null edge table", who);
    CRIMAC_REQUIRE(ed->host[0] >= 0, "%s: edges[0]=%lld is negative", who, ed->host[0]);
    for (long pb = 0; pb < n_pb_total; ++pb) {
      const long long w = ed->host[pb + 1] - ed->host[pb];      // (both >= 0 here: no overflow)
      CRIMAC_REQUIRE(w >= 0 && w <= 2147483647LL, "%s: edges[%ld]=%lld, edges[%ld]=%lld: the table must not decrease and "
                     "no cell is wider than 2^31 - 1 pings", who, pb, ed->host[pb], pb + 1, ed->host[pb + 1]);
    }
    cells_touched(ed->host, n_pb_total, ping_origin, ping_origin + n_pings, pb0, pb1, widest);
  } else {
    pb0 = ping_origin / ping_bin;
    pb1 = (ping_origin + n_pings - 1) / ping_bin;
  }
  const bool layers = sb && sb->reference == 1;
  if (sb) {
    CRIMAC_REQUIRE(sb->line, "%s: null seabed vector", who);
    CRIMAC_REQUIRE(sb->first >= 0 && sb->first + n_pings <= sb->len, "%s: pings [%ld, %ld) outside the seabed vector of "
                   "%ld pings", who, sb->first, sb->first + n_pings, sb->len);
    CRIMAC_REQUIRE(sb->reference == 0 || sb->reference == 1, "%s: reference %d (0 surface, 1 seabed)", who, sb->reference);
    CRIMAC_REQUIRE(!layers || (sb->n_layers >= 1 && (long)sb->n_layers * range_bin <= 2147483647L),
                   "%s: n_layers=%d with the seabed reference must be >= 1 (and n_layers * range_bin below 2^31)", who,
                   sb->n_layers);
  }
  Geom g;
  g.n_range = n_range;
  g.range_bin = range_bin;
  g.n_rb = layers ? sb->n_layers : (n_range + range_bin - 1) / range_bin;
  g.mode = mode;
  g.n_pings = n_pings;
  g.sv_ping_off = sv_ping_off;
  g.ping_bin = ping_bin;
  g.ping_origin = ping_origin;
  g.n_pb_total = n_pb_total;
  g.pb0 = pb0;
  g.thr0 = thr_sandeel;
  g.thr1 = thr_other;
  g.seabed = sb ? sb->line + sb->first : nullptr;
  g.seabed_offset = sb ? sb->offset : 0;
  g.reference = sb ? sb->reference : 0;
  g.edges = ed ? ed->dev : nullptr;
  if (pb1 < pb0) return CRIMAC_OK;                             // (an edge table none of whose cells the launch touches)
  const long cells = (pb1 - pb0 + 1) * g.n_rb;
  // tiles of a full cell (its origin may sit up to 3 short of a multiple of 4 in either direction); the row bounding box
  // of a seabed-referenced layer may be the whole column
  const long span_r = (range_bin < n_range && !layers ? range_bin : n_range) + 3, span_p = (widest < n_pings ? widest : n_pings) + 3;
  const long tiles = ((span_r + kTile - 1) / kTile) * ((span_p + kTile - 1) / kTile);
  const long want = (CRIMAC_INTEGRATE_SPLIT_WGS + cells - 1) / cells;
  g.splits = (int)(want < tiles ? want : tiles);
  CRIMAC_REQUIRE(cells * g.splits <= 2147483647L, "%s: %ld cells in one launch", who, cells);
  const long n_freqs = fa ? fa->n_freqs : 1;
  CRIMAC_REQUIRE(scratch_bytes >= n_freqs * cells * g.splits * (long)sizeof(Slot) && (uintptr_t)scratch % 8 == 0,
                 "%s: scratch of %ld bytes, this launch needs %ld (8-byte aligned; (cells + "
                 "CRIMAC_INTEGRATE_SPLIT_WGS) * CRIMAC_INTEGRATE_SLOT_BYTES%s always suffices)", who, scratch_bytes,
                 n_freqs * cells * g.splits * (long)sizeof(Slot), fa ? " * n_freqs" : "");
  bool vec_sv = n_range % 4 == 0 && (uintptr_t)sv % 16 == 0;
  const bool vec_pred = n_pings % 4 == 0 && (uintptr_t)pred % (pred_f16 ? 8 : 16) == 0;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)(cells * g.splits);
  Planes fq{};
  fq.n = (int)n_freqs;
  fq.slots = cells * g.splits;
  for (int i = 0; fa && i < fq.n; ++i) {
    fq.off[i] = fa->channels[i] * fa->plane_stride;
    vec_sv = vec_sv && (uintptr_t)(sv + fq.off[i]) % 16 == 0;      // the 16-byte reads only if EVERY selected plane allows them
  }
  launch_pass1(pred_f16, sb, vec_sv, vec_pred, blocks, st, pred, sv, g, fq, (Slot*)scratch);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(integrate_finish_kernel, dim3((unsigned)((cells * fq.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     (const Slot*)scratch, g, fq.n, cells, acc, cnt);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

// ---- crimac_integrate_confusion: the same sums split by the ANNOTATED class, from an evaluation batch --------------------
// All five operands of a pixel -- sv, the transformed label, three logits -- lie in patch layout [ph][pw], ping
// contiguous, so nothing is transposed and no LDS tile is needed: a workgroup owns (patch, i, j), the (i, j)-th cell of the
// (ncp x ncr) window of cells the patch can overlap, counted from the cell that holds its pixel (0, 0).  It walks the
// rectangle patch x cell x grid row by row with consecutive lanes on consecutive pings (4-byte loads, coalesced up to
// the row ends of the rectangle); the logits are read only for the pixels that count.  Thread -> lanes (butterfly) -> waves
// (in order, by thread 0) -> the (patch, i, j) slot of the scratch, as above.  A window cell outside the accumulator grid
// gets no workgroup work and no slot write: nothing is read for its pixels.
// Finish: one thread per slot.  The thread of the FIRST patch of the batch whose window holds the slot's cell owns that
// cell: it adds the cell's slots in patch order and does the plain read-add-write of its 18 outputs; the others leave.
// Who owns what depends on the origins alone, so the order of every sum is a function of the arguments.
//
// crimac_integrate_confusion_multi (the MULTI instantiations of the same two kernels): a batch packed from several
// echograms.  Patch p belongs to echogram src[p]; its workgroups take n_range from descs[src[p]], n_pb and the first word
// of the echogram's [3][3][n_pb][n_rb] block inside acc / cnt from shares[src[p]], and a patch whose src names no
// descriptor does no work.  Two patches of different echograms may have the same origin, so the finish keeps the src values
// next to the window origins in LDS: the owner of a cell is the first patch WITH THE SAME src whose window holds it, and it
// adds the slots of the patches with that src only, in patch order.  A (patch, cell) slot depends on the patch alone:
// every echogram gets the bits a single-source launch over its patches of the batch, in batch order, would have given it.
struct CSlot { Slot a[3]; };                                 // per annotated class: background, sandeel, other
static_assert(sizeof(CSlot) == CRIMAC_CONFUSION_SLOT_BYTES, "scratch slot size is part of the ABI");
constexpr int kConfusionMaxPatches = CRIMAC_CONFUSION_MAX_PATCHES;

struct CGeom {
  int P, C, channel, ph, pw, n_range, range_bin, n_rb, ncp, ncr, mode;
  long ping_bin, n_pb_total;
  float thr0, thr1;
  // crimac_integrate_confusion_multi: the echogram of every patch; n_range, n_rb and n_pb_total above are not read
  const crimac_memm_desc* descs;
  int n_desc;
  const int* src;
  const long long* shares;                                   // [n_desc][2] = (first word of the echogram's block, n_pb)
};

// the grid patch p accumulates into: one for the launch, or (MULTI) its echogram's; false: src[p] names no descriptor
struct CGrid { long n_range, n_rb, n_pb, first; };
template <bool MULTI>
__device__ __forceinline__ bool grid_of(const CGeom& g, int p, CGrid& out) {
  if constexpr (MULTI) {
    const int s = g.src[p];
    if (s < 0 || s >= g.n_desc) return false;
    out.n_range = g.descs[s].n_range;
    out.n_rb = (out.n_range + g.range_bin - 1) / g.range_bin;
    out.first = g.shares[2 * s];
    out.n_pb = g.shares[2 * s + 1];
  } else {
    out = CGrid{g.n_range, g.n_rb, g.n_pb_total, 0};
  }
  return true;
}

__device__ __forceinline__ long floor_div(long a, long b) {      // b > 0
  const long q = a / b;
  return q - (a % b != 0 && a < 0);
}

template <bool MULTI>
__global__ __launch_bounds__(kThreads) void confusion_cells_kernel(const float* __restrict__ logits,
                                                                   const float* __restrict__ raw,
                                                                   const short* __restrict__ labels,
                                                                   const int* __restrict__ origins, CGeom g,
                                                                   CSlot* __restrict__ scratch) {
  __shared__ CSlot wave_part[kThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = blockIdx.x % g.ncp, j = blockIdx.x / g.ncp % g.ncr, p = blockIdx.x / (g.ncp * g.ncr);
  CGrid e;
  if (!grid_of<MULTI>(g, p, e)) return;                                    // (uniform, as the next return)
  const long y0 = origins[2 * p], x0 = origins[2 * p + 1];
  const long pb = floor_div(x0, g.ping_bin) + i, rb = floor_div(y0, g.range_bin) + j;
  if (pb < 0 || pb >= e.n_pb || rb < 0 || rb >= e.n_rb) return;            // (uniform: nobody waits at the barrier)
  // the cell in patch coordinates, clipped to the patch and to rows below n_range (its pings lie inside the grid)
  long c0 = pb * g.ping_bin - x0, c1 = c0 + g.ping_bin, r0 = rb * g.range_bin - y0, r1 = r0 + g.range_bin;
  c0 = c0 > 0 ? c0 : 0;
  r0 = r0 > 0 ? r0 : 0;
  c1 = c1 < g.pw ? c1 : g.pw;
  r1 = r1 < g.ph ? r1 : g.ph;
  r1 = r1 < e.n_range - y0 ? r1 : e.n_range - y0;
  const int w = c1 > c0 ? (int)(c1 - c0) : 0, h = r1 > r0 ? (int)(r1 - r0) : 0;
  const int n = w * h;                                       // (<= ph * pw < 2^31)
  const long HW = (long)g.ph * g.pw;
  const short* __restrict__ lab_p = labels + p * HW;
  const float* __restrict__ sv_p = raw + ((long)p * g.C + g.channel) * HW;
  const float* __restrict__ logit_p = logits + (long)p * 3 * HW;
  double s[3][3] = {};
  int m[3][3] = {};                                          // (a thread sees n / 256 + 1 pixels at most)
  for (int k = t; k < n; k += kThreads) {
    const long at = (r0 + k / w) * g.pw + c0 + k % w;
    const int l = lab_p[at];
    const float sv = sv_p[at];
    // finite and > 0; the largest finite float is what the zarr crop's nan_to_num made of +Inf, so it is not finite here
    if (l < 0 || l > 2 || !(sv > 0.f && sv < 3.402823466e+38f)) continue;
    float z[8], den;
    pr_softmax_terms(logit_p + at, HW, 3, z, den);
    const float a = (float)pr_prob_f16(z[1], den), b = (float)pr_prob_f16(z[2], den);
    const double sd = (double)sv;
    bool in0, in1;
    double v0, v1;
    if (g.mode == 0) {
      in0 = a >= g.thr0, in1 = b >= g.thr1;
      v0 = in0 ? sd : 0.0, v1 = in1 ? sd : 0.0;
    } else {
      in0 = a > 0.f, in1 = b > 0.f;                          // (a NaN or negative weight counts as 0)
      v0 = in0 ? sd * (double)a : 0.0, v1 = in1 ? sd * (double)b : 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const bool is = l == c;
      s[c][0] += is ? v0 : 0.0;
      s[c][1] += is ? v1 : 0.0;
      s[c][2] += is ? sd : 0.0;
      m[c][0] += is && in0;
      m[c][1] += is && in1;
      m[c][2] += is;
    }
  }
  // ---- lane -> wave -> workgroup, each in a fixed order
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s[c][k] = wave_sum_d(s[c][k]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m[c][k] += __shfl_xor(m[c][k], o, 64);
    }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      wave_part[wave].a[c] = Slot{{s[c][0], s[c][1], s[c][2]}, {m[c][0], m[c][1], m[c][2]}};
  }
  __syncthreads();
  if (t == 0) {
    CSlot out = wave_part[0];
    for (int wv = 1; wv < kThreads / 64; ++wv)
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) {
          out.a[c].sum[k] += wave_part[wv].a[c].sum[k];
          out.a[c].cnt[k] += wave_part[wv].a[c].cnt[k];
        }
    scratch[blockIdx.x] = out;
  }
}

template <bool MULTI>
__global__ __launch_bounds__(kThreads) void confusion_finish_kernel(const CSlot* __restrict__ scratch,
                                                                    const int* __restrict__ origins, CGeom g,
                                                                    double* __restrict__ acc, long long* __restrict__ cnt) {
  // the first cell of every patch's window (MULTI: and the patch's echogram), once per workgroup
  __shared__ long pb0[kConfusionMaxPatches];
  __shared__ int rb0[kConfusionMaxPatches];
  __shared__ int src[MULTI ? kConfusionMaxPatches : 1];
  for (int q = threadIdx.x; q < g.P; q += kThreads) {
    rb0[q] = (int)floor_div(origins[2 * q], g.range_bin);
    pb0[q] = floor_div(origins[2 * q + 1], g.ping_bin);
    if constexpr (MULTI) src[q] = g.src[q];
  }
  __syncthreads();
  const long slot = (long)blockIdx.x * kThreads + threadIdx.x;
  const int per_patch = g.ncp * g.ncr;
  if (slot >= (long)g.P * per_patch) return;
  const int p = (int)(slot / per_patch), i = (int)(slot % g.ncp), j = (int)(slot / g.ncp % g.ncr);
  CGrid e;
  if (!grid_of<MULTI>(g, p, e)) return;                                    // (no workgroup wrote this slot)
  const long pb = pb0[p] + i, rb = (long)rb0[p] + j;
  if (pb < 0 || pb >= e.n_pb || rb < 0 || rb >= e.n_rb) return;            // (nor this one)
  for (int q = 0; q < p; ++q) {                                            // an earlier patch owns the cell
    if (MULTI && src[q] != src[p]) continue;                               // (of the same echogram)
    const long qi = pb - pb0[q], qj = rb - rb0[q];
    if (qi >= 0 && qi < g.ncp && qj >= 0 && qj < g.ncr) return;
  }
  CSlot out = scratch[slot];
  for (int q = p + 1; q < g.P; ++q) {
    if (MULTI && src[q] != src[p]) continue;
    const long qi = pb - pb0[q], qj = rb - rb0[q];
    if (qi < 0 || qi >= g.ncp || qj < 0 || qj >= g.ncr) continue;
    const CSlot& x = scratch[((long)q * g.ncr + qj) * g.ncp + qi];
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 3; ++k) {
        out.a[c].sum[k] += x.a[c].sum[k];
        out.a[c].cnt[k] += x.a[c].cnt[k];
      }
  }
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 3; ++k) {
      const long at = e.first + (((long)c * 3 + k) * e.n_pb + pb) * e.n_rb + rb;
      acc[at] += out.a[c].sum[k];
      cnt[at] += out.a[c].cnt[k];
    }
}

}  // namespace

// Both confusion entry points: the argument checks, the geometry, the two launches.  `g` arrives with the grid of the
// launch (single: n_range, n_pb_total) or with the echogram tables (multi: descs != NULL).
static int confusion(const char* who, CGeom g, const float* logits, int ncls, const float* raw, int C, int channel,
                     const short* labels, const int* origins, int P, int ph, int pw, long ping_bin, int range_bin,
                     float thr_sandeel, float thr_other, int mode, double* acc, long long* cnt, void* scratch,
                     long scratch_bytes, void* stream) {
  const bool multi = g.descs != nullptr;
  CRIMAC_REQUIRE(logits && raw && labels && origins && acc && cnt && scratch, "%s: null pointer", who);
  CRIMAC_REQUIRE(ncls == 3, "%s: ncls=%d: the planes are those of a 3-class model (background, sandeel, other)", who, ncls);
  CRIMAC_REQUIRE(P > 0 && P <= kConfusionMaxPatches, "%s: P=%d patches (1 .. CRIMAC_CONFUSION_MAX_PATCHES = %d per launch)",
                 who, P, kConfusionMaxPatches);
  CRIMAC_REQUIRE(ph > 0 && pw > 0 && ph <= 32768 && pw <= 32768, "%s: patch %d x %d (1 .. 32768 each)", who, ph, pw);
  CRIMAC_REQUIRE(C > 0 && channel >= 0 && channel < C, "%s: channel %d of %d sv planes", who, channel, C);
  CRIMAC_REQUIRE(multi || g.n_range > 0, "%s: n_range=%d", who, g.n_range);
  CRIMAC_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0 threshold, 1 probability)", who, mode);
  CRIMAC_REQUIRE(thr_sandeel > 0.f && thr_other > 0.f, "%s: thr = (%g, %g) must be > 0", who, (double)thr_sandeel,
                 (double)thr_other);
  CRIMAC_REQUIRE(ping_bin > 0 && range_bin > 0, "%s: ping_bin=%ld, range_bin=%d must be positive", who, ping_bin, range_bin);
  CRIMAC_REQUIRE(ping_bin <= 2147483647L && (multi || (g.n_pb_total > 0 && g.n_pb_total <= 2147483647L)),
                 "%s: ping_bin=%ld, n_pb_total=%ld outside 1 .. 2^31 - 1", who, ping_bin, g.n_pb_total);
  g.P = P;
  g.C = C;
  g.channel = channel;
  g.ph = ph;
  g.pw = pw;
  g.range_bin = range_bin;
  g.n_rb = multi ? 0 : (g.n_range + range_bin - 1) / range_bin;
  g.ncp = (int)((pw + ping_bin - 1) / ping_bin) + 1;
  g.ncr = (ph + range_bin - 1) / range_bin + 1;
  g.mode = mode;
  g.ping_bin = ping_bin;
  g.thr0 = thr_sandeel;
  g.thr1 = thr_other;
  const long slots = (long)P * g.ncp * g.ncr;
  CRIMAC_REQUIRE(slots <= 2147483647L, "%s: %ld (patch, cell) slots in one launch", who, slots);
  CRIMAC_REQUIRE(scratch_bytes >= slots * (long)sizeof(CSlot) && (uintptr_t)scratch % 8 == 0,
                 "%s: scratch of %ld bytes, this launch needs %ld (8-byte aligned; P * (ceil(pw / ping_bin) + 1) * "
                 "(ceil(ph / range_bin) + 1) * CRIMAC_CONFUSION_SLOT_BYTES)", who, scratch_bytes, slots * (long)sizeof(CSlot));
  const hipStream_t st = (hipStream_t)stream;
  const dim3 finish((unsigned)((slots + kThreads - 1) / kThreads));
  if (multi) hipLaunchKernelGGL(confusion_cells_kernel<true>, dim3((unsigned)slots), dim3(kThreads), 0, st, logits, raw, labels, origins, g, (CSlot*)scratch);
  else hipLaunchKernelGGL(confusion_cells_kernel<false>, dim3((unsigned)slots), dim3(kThreads), 0, st, logits, raw, labels, origins, g, (CSlot*)scratch);
  CRIMAC_LAUNCH_CHECK();
  if (multi) hipLaunchKernelGGL(confusion_finish_kernel<true>, finish, dim3(kThreads), 0, st, (const CSlot*)scratch, origins, g, acc, cnt);
  else hipLaunchKernelGGL(confusion_finish_kernel<false>, finish, dim3(kThreads), 0, st, (const CSlot*)scratch, origins, g, acc, cnt);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_integrate_confusion(const float* logits, int ncls, const float* raw, int C, int channel,
                                          const short* labels, const int* origins, int P, int ph, int pw, int n_range,
                                          long ping_bin, int range_bin, long n_pb_total, float thr_sandeel, float thr_other,
                                          int mode, double* acc, long long* cnt, void* scratch, long scratch_bytes,
                                          void* stream) {
  CGeom g{};
  g.n_range = n_range;
  g.n_pb_total = n_pb_total;
  return confusion("integrate_confusion", g, logits, ncls, raw, C, channel, labels, origins, P, ph, pw, ping_bin, range_bin,
                   thr_sandeel, thr_other, mode, acc, cnt, scratch, scratch_bytes, stream);
}

extern "C" int crimac_integrate_confusion_multi(const float* logits, int ncls, const float* raw, int C, int channel,
                                                const short* labels, const int* origins, const crimac_memm_desc* descs,
                                                int n_desc, const int* src, const long long* shares, int P, int ph, int pw,
                                                long ping_bin, int range_bin, float thr_sandeel, float thr_other, int mode,
                                                double* acc, long long* cnt, void* scratch, long scratch_bytes,
                                                void* stream) {
  CRIMAC_REQUIRE(descs && src && shares, "integrate_confusion_multi: null pointer (descs, src, shares)");
  CRIMAC_REQUIRE(n_desc > 0, "integrate_confusion_multi: n_desc=%d descriptors", n_desc);
  CGeom g{};
  g.descs = descs;
  g.n_desc = n_desc;
  g.src = src;
  g.shares = shares;
  return confusion("integrate_confusion_multi", g, logits, ncls, raw, C, channel, labels, origins, P, ph, pw, ping_bin,
                   range_bin, thr_sandeel, thr_other, mode, acc, cnt, scratch, scratch_bytes, stream);
}

extern "C" int crimac_integrate_classes(const void* pred, int pred_f16, int n_range, long n_pings, const float* sv,
                                        long data_pings, long sv_ping_off, float thr_sandeel, float thr_other, int mode,
                                        long ping_bin, int range_bin, long ping_origin, long n_pb_total, double* acc,
                                        long long* cnt, void* scratch, long scratch_bytes, void* stream) {
  return integrate("integrate_classes", nullptr, nullptr, nullptr, pred, pred_f16, n_range, n_pings, sv, data_pings, sv_ping_off, thr_sandeel,
                   thr_other, mode, ping_bin, range_bin, ping_origin, n_pb_total, acc, cnt, scratch, scratch_bytes, stream);
}

extern "C" int crimac_integrate_layers(const void* pred, int pred_f16, int n_range, long n_pings, const float* sv,
                                       long data_pings, long sv_ping_off, float thr_sandeel, float thr_other, int mode,
                                       long ping_bin, int range_bin, long ping_origin, long n_pb_total, const int* seabed,
                                       long seabed_first, long seabed_len, int seabed_offset, int reference, int n_layers,
                                       double* acc, long long* cnt, void* scratch, long scratch_bytes, void* stream) {
  const SeabedArgs sb{seabed, seabed_first, seabed_len, seabed_offset, reference, n_layers};
  return integrate("integrate_layers", &sb, nullptr, nullptr, pred, pred_f16, n_range, n_pings, sv, data_pings, sv_ping_off, thr_sandeel,
                   thr_other, mode, ping_bin, range_bin, ping_origin, n_pb_total, acc, cnt, scratch, scratch_bytes, stream);
}

extern "C" int crimac_integrate_edges(const void* pred, int pred_f16, int n_range, long n_pings, const float* sv,
                                      long data_pings, long sv_ping_off, float thr_sandeel, float thr_other, int mode,
                                      const long long* edges_dev, const long long* edges_host, int range_bin,
                                      long ping_origin, long n_pb_total, const int* seabed, long seabed_first,
                                      long seabed_len, int seabed_offset, int reference, int n_layers, double* acc,
                                      long long* cnt, void* scratch, long scratch_bytes, void* stream) {
  const SeabedArgs sb{seabed, seabed_first, seabed_len, seabed_offset, reference, n_layers};
  const EdgeArgs ed{edges_dev, edges_host};
  return integrate("integrate_edges", seabed ? &sb : nullptr, &ed, nullptr, pred, pred_f16, n_range, n_pings, sv, data_pings,
                   sv_ping_off, thr_sandeel, thr_other, mode, 0, range_bin, ping_origin, n_pb_total, acc, cnt, scratch,
                   scratch_bytes, stream);
}

extern "C" int crimac_integrate_freqs(const void* pred, int pred_f16, int n_range, long n_pings, const float* sv,
                                      long plane_stride, int n_planes, const int* channels, int n_freqs, long data_pings,
                                      long sv_ping_off, float thr_sandeel, float thr_other, int mode, long ping_bin,
                                      const long long* edges_dev, const long long* edges_host, int range_bin,
                                      long ping_origin, long n_pb_total, const int* seabed, long seabed_first,
                                      long seabed_len, int seabed_offset, int reference, int n_layers, double* acc,
                                      long long* cnt, void* scratch, long scratch_bytes, void* stream) {
  const SeabedArgs sb{seabed, seabed_first, seabed_len, seabed_offset, reference, n_layers};
  const EdgeArgs ed{edges_dev, edges_host};
  const FreqArgs fa{plane_stride, n_planes, channels, n_freqs};
  return integrate("integrate_freqs", seabed ? &sb : nullptr, edges_dev ? &ed : nullptr, &fa, pred, pred_f16, n_range, n_pings, sv,
                   data_pings, sv_ping_off, thr_sandeel, thr_other, mode, edges_dev ? 0 : ping_bin, range_bin, ping_origin,
                   n_pb_total, acc, cnt, scratch, scratch_bytes, stream);
}
