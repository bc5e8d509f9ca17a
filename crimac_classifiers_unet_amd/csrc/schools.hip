// Schools from the predictions (CDNA4 / gfx950): connected regions of one predicted class, with per-school statistics.
//
// The reference has schools on the annotation side only (Echogram.get_object_bounding_boxes); the predicted ones are
// found downstream on the host (threshold, scipy.ndimage.label, numpy sums).  Here the class plane pred [n_range][n_pings]
// (ping contiguous, what crimac_scatter_patches_ex wrote) and the sv planes [data_pings][n_range] (range contiguous) of the
// chunk are resident, and two entry points do it with a FIXED number of launches and no host synchronisation.
//
// crimac_schools_label -- union-find labelling (csrc/ccl.h), three kernels:
//   label_tiles_kernel   a workgroup labels one CCL_TILE_H x CCL_TILE_W tile in LDS: every foreground pixel joins its left /
//                        upper neighbours of the tile (atomicMin on LDS), then writes the GLOBAL index of its tile root;
//   merge_borders_kernel the first row and first column of every tile join their neighbours across the tile border
//                        (atomicMin on global memory; every parent is read by an agent-scope atomic load, so that no
//                        workgroup depends on a cache line another one has written during the launch);
//   flatten_kernel       labels[i] = the root of i.
//   Roots are the smallest index of their tree, so the final label is the component's first pixel in raster order.
//   label_tiles_kernel is ONE body; what a foreground pixel is, is its template parameter (PredFg: a probability plane,
//   crimac_schools_label; IdsFg: the raw annotation ids, crimac_schools_label_ids; BothFg: foreground in two label planes,
//   crimac_schools_label_both).  The overlap of two sets of schools labelled with one connectivity needs nothing else: a
//   component of the plane `A >= 0 && B >= 0` lies in exactly one school of A and one of B, so crimac_schools_stats of that
//   plane is a table of pair overlaps and crimac_schools_pair_anchors names the pair of every row.
//
// crimac_schools_stats -- the per-school table, in ascending anchor order:
//   count_kernel         key[anchor] += pixels (64-bit integer atomics, one add per run of equal labels of a wave), bit 62 set
//                        when a kept-edge column is touched;
//   rank_count / rank_scan / rank_assign   the schools that are KEPT get consecutive slots in anchor order (per-block counts,
//                        one workgroup scans them, per-block ranks); key[anchor] becomes the slot (-1: dropped);
//   moments_kernel       boxes, row and ping sums by 32 / 64-bit integer atomics (exact in any order), the edge columns
//                        translated to slots;
//   sv_kernel            the fp64 sums: ONE workgroup per school walks the school's bounding box in a fixed order (thread t
//                        takes pixels t, t + 1024, ... of the box, ping fastest), adds the sv of the pixels whose label is
//                        the school's anchor into per-thread fp64 accumulators, lanes by butterfly, waves in wave order.  No
//                        floating-point atomics: bit-reproducible, and the sum of one frequency does not depend on how many
//                        are summed with it.  Cost: the sum of the box areas -- a survey of many nested diagonal schools, whose
//                        boxes all cover most of the chunk, pays (schools x chunk area); so does one box per workgroup when a
//                        single school fills the chunk (one CU streams it).
#include "common.h"

#include "ccl.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSvThreads = 1024;
constexpr int kMaxFreqs = CRIMAC_SCHOOLS_MAX_FREQS;
constexpr int kTilePixels = CCL_TILE_W * CCL_TILE_H;
constexpr unsigned long long kEdgeBit = 1ull << 62;
constexpr unsigned long long kCountMask = kEdgeBit - 1;

struct LdsMem {
  int* s;
  int* err;
  __device__ __forceinline__ int load(int i) { return __hip_atomic_load(s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int fetch_min(int i, int v) { return atomicMin(s + i, v); }
  __device__ __forceinline__ void fail() { *err = 1; }
};

struct GlobalMem {
  int* L;
  int* err;
  __device__ __forceinline__ int load(int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int fetch_min(int i, int v) { return atomicMin(L + i, v); }
  __device__ __forceinline__ void fail() { *err = 1; }
};

// ---- the foreground rules of label_tiles_kernel ----------------------------------------------------------------------------
// fill_tile(fg, lab, ...) writes lab[i] = i for a foreground pixel i of the tile and -1 for every other one (outside the plane
// included).  The rules that read a plane laid out as the labels ([n_range][n_pings], ping fastest) give `at(linear index)`.
// PredFg: the stored value, widened exactly, >= threshold (NaN compares false)
template <typename TP>
struct PredFg {
  const TP* __restrict__ pred;
  float thr;
  __device__ __forceinline__ bool at(long i) const { return (float)pred[i] >= thr; }
};

// BothFg: foreground in two label planes at once (the overlap of two sets of schools)
struct BothFg {
  const int* __restrict__ a;
  const int* __restrict__ b;
  __device__ __forceinline__ bool at(long i) const { return a[i] >= 0 && b[i] >= 0; }
};

template <class Fg>
__device__ __forceinline__ void fill_tile(const Fg& fg, int* lab, int t, int r0, int p0, int n_range, int n_pings) {
#pragma unroll
  for (int k = 0; k < kTilePixels / kThreads; ++k) {
    const int i = t + kThreads * k, r = r0 + i / CCL_TILE_W, p = p0 + i % CCL_TILE_W;
    bool fg_px = false;
    if (r < n_range && p < n_pings) fg_px = fg.at((long)r * n_pings + p);
    lab[i] = fg_px ? i : -1;
  }
}

// IdsFg: raw annotation ids [ids_pings][n_range], RANGE fastest -- the tile read is a transposition.  The lanes run along
// range (16 consecutive int16 of one ping, 4 pings per wave and step) and write the tile's LDS transposed, so that the rest of
// the kernel sees the tile as the other rules leave it.  A wave reads 4 runs of 32 bytes per step and its LDS stores collide
// on the banks (stride CCL_TILE_W words); the rate of this read has NOT been measured.
struct IdsFg {
  const short* __restrict__ ids;
  long ping_off;                                   // column ping_off of ids is column 0 of the labels
  int select;
  __device__ __forceinline__ bool is_fg(int id) const {
    return select >= 0 ? id == select : (id != 0 && id != 27 && id != 1);          // (the ids labels.hip does not map to a class)
  }
};

__device__ __forceinline__ void fill_tile(const IdsFg& fg, int* lab, int t, int r0, int p0, int n_range, int n_pings) {
  static_assert(kThreads % CCL_TILE_H == 0 && CCL_TILE_W % (kThreads / CCL_TILE_H) == 0, "the transposed read covers the tile");
  const int lr = t % CCL_TILE_H, r = r0 + lr;
#pragma unroll
  for (int k = 0; k < kTilePixels / kThreads; ++k) {
    const int lp = t / CCL_TILE_H + (kThreads / CCL_TILE_H) * k, p = p0 + lp;
    bool fg_px = false;
    if (r < n_range && p < n_pings) fg_px = fg.is_fg(fg.ids[(fg.ping_off + p) * n_range + r]);
    const int i = lr * CCL_TILE_W + lp;
    lab[i] = fg_px ? i : -1;
  }
}

template <class Fg>
__global__ void __launch_bounds__(kThreads)
label_tiles_kernel(const Fg fg, int n_range, int n_pings, int connectivity, int tiles_p, int* __restrict__ labels, int* err) {
  __shared__ int lab[kTilePixels];
  const int t = threadIdx.x;
  const int r0 = (int)(blockIdx.x / tiles_p) * CCL_TILE_H, p0 = (int)(blockIdx.x % tiles_p) * CCL_TILE_W;
  fill_tile(fg, lab, t, r0, p0, n_range, n_pings);
  __syncthreads();
  int dummy = 0;
  LdsMem m{lab, &dummy};
#pragma unroll
  for (int k = 0; k < kTilePixels / kThreads; ++k) {
    const int i = t + kThreads * k, lr = i / CCL_TILE_W, lp = i % CCL_TILE_W;
    if (m.load(i) < 0) continue;                   // (-1 is never written after the fill: background stays background)
    ccl_back_neighbours(connectivity, [&](int dr, int dp) {
      const int nr = lr + dr, np = lp + dp;
      if (nr < 0 || np < 0 || np >= CCL_TILE_W) return;
      const int j = nr * CCL_TILE_W + np;
      if (m.load(j) >= 0) ccl_unite(m, i, j, kTilePixels);
    });
  }
  __syncthreads();
  int roots[kTilePixels / kThreads];
#pragma unroll
  for (int k = 0; k < kTilePixels / kThreads; ++k) {
    const int i = t + kThreads * k;
    roots[k] = lab[i] < 0 ? -1 : ccl_find(m, i, kTilePixels);
  }
  if (dummy) *err = 1;
#pragma unroll
  for (int k = 0; k < kTilePixels / kThreads; ++k) {
    const int i = t + kThreads * k, r = r0 + i / CCL_TILE_W, p = p0 + i % CCL_TILE_W;
    if (r < n_range && p < n_pings)
      labels[(long)r * n_pings + p] = roots[k] < 0 ? -1 : (r0 + roots[k] / CCL_TILE_W) * n_pings + p0 + roots[k] % CCL_TILE_W;
  }
}

// one workgroup per tile: its first row (threads 0 .. W - 1) and first column (threads W .. W + H - 1)
__global__ void __launch_bounds__(CCL_TILE_W + CCL_TILE_H)
merge_borders_kernel(int* labels, int n_range, int n_pings, int connectivity, int tiles_p, int* err) {
  const int t = threadIdx.x;
  const int r0 = (int)(blockIdx.x / tiles_p) * CCL_TILE_H, p0 = (int)(blockIdx.x % tiles_p) * CCL_TILE_W;
  const int r = t < CCL_TILE_W ? r0 : r0 + (t - CCL_TILE_W), p = t < CCL_TILE_W ? p0 + t : p0;
  if (r >= n_range || p >= n_pings) return;
  if (t == CCL_TILE_W) return;                     // (the corner pixel is thread 0's)
  const int i = r * n_pings + p;
  GlobalMem m{labels, err};
  if (m.load(i) < 0) return;
  const long bound = (long)n_range * n_pings;
  ccl_border_neighbours(r, p, connectivity, [&](int dr, int dp) {
    const int nr = r + dr, np = p + dp;
    if (nr < 0 || nr >= n_range || np < 0 || np >= n_pings) return;
    const int j = nr * n_pings + np;
    if (m.load(j) >= 0) ccl_unite(m, i, j, bound);
  });
}

__global__ void __launch_bounds__(kThreads)
flatten_kernel(int* labels, long n, int* err) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  GlobalMem m{labels, err};
  if (labels[i] < 0) return;
  const int root = ccl_find(m, (int)i, n);
  labels[i] = root;                                // (a reader that passes through i meets the old parent or the root)
}

// ---- statistics ----------------------------------------------------------------------------------------------------------
// A RUN: the lanes of a wave that follow each other with the same label in the same row.  The first lane of a run (`head`)
// acts for all of them: `len` lanes, pings p .. p + len - 1.
struct Run { bool head; int len; };
__device__ __forceinline__ Run run_of(int label, int p) {
  const int lane = __lane_id();
  const int prev = __shfl_up(label, 1, 64);
  const bool head = lane == 0 || prev != label || p == 0;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
  return {head, (above ? __builtin_ctzll(above) : 64) - lane};
}

__device__ __forceinline__ bool kept(unsigned long long key, long long min_pixels) {
  return (long long)(key & kCountMask) >= min_pixels || (key & kEdgeBit);
}

__global__ void __launch_bounds__(kThreads)
count_kernel(const int* __restrict__ labels, long n, int n_pings, int keep_left, int keep_right, unsigned long long* key) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const int p = i < n ? (int)(i % n_pings) : 0;
  const int label = i < n ? labels[i] : -2;
  const Run run = run_of(label, p);
  if (label < 0) return;
  if (run.head) atomicAdd(key + label, (unsigned long long)run.len);
  if ((keep_left && p == 0) || (keep_right && p == n_pings - 1)) atomicOr(key + label, kEdgeBit);
}

// is pixel i the anchor of a school that is kept?
__device__ __forceinline__ bool kept_anchor(const int* labels, const unsigned long long* key, long i, long n, long long min_pixels) {
  return i < n && labels[i] == (int)i && kept(key[i], min_pixels);
}

__global__ void __launch_bounds__(kThreads)
rank_count_kernel(const int* __restrict__ labels, const unsigned long long* __restrict__ key, long n, long long min_pixels,
                  int* __restrict__ block_cnt) {
  __shared__ int wave_cnt[kThreads / 64];
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long b = __ballot(kept_anchor(labels, key, i, n, min_pixels));
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kThreads / 64; ++w) s += wave_cnt[w];
    block_cnt[blockIdx.x] = s;
  }
}

// one workgroup: block_cnt -> exclusive prefix in place; found = the total
__global__ void __launch_bounds__(kSvThreads)
rank_scan_kernel(int* block_cnt, long nb, long long* found) {
  __shared__ long long wave_sum[kSvThreads / 64];
  __shared__ long long carry_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (long base = 0; base < nb; base += kSvThreads) {
    const long i = base + t;
    const long long v = i < nb ? block_cnt[i] : 0;
    long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long x = __shfl_up(incl, o, 64);
      if (lane >= o) incl += x;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    long long before = carry_s;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (i < nb) block_cnt[i] = (int)(before + incl - v);      // (< n < 2^31)
    __syncthreads();
    if (t == kSvThreads - 1) carry_s = before + incl;
    __syncthreads();
  }
  if (t == 0) found[0] = carry_s;
}

struct Table {
  int* anchor;
  long long* pixels;
  int* bbox;
  long long *row_sum, *ping_sum;
  double* sv_sum;
  long long* sv_pixels;
  long capacity;
};

__global__ void __launch_bounds__(kThreads)
rank_assign_kernel(const int* __restrict__ labels, unsigned long long* key, long n, long long min_pixels,
                   const int* __restrict__ block_off, Table tb) {
  __shared__ int wave_cnt[kThreads / 64];
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool anchor = i < n && labels[i] == (int)i;
  const unsigned long long k = anchor ? key[i] : 0ull;
  const bool keep = anchor && kept(k, min_pixels);
  const unsigned long long b = __ballot(keep);
  if (lane == 0) wave_cnt[wave] = __popcll(b);
  __syncthreads();
  if (!anchor) return;
  long long slot = -1;
  if (keep) {
    slot = block_off[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) slot += wave_cnt[w];
    if (slot < tb.capacity) {
      tb.anchor[slot] = (int)i;
      tb.pixels[slot] = (long long)(k & kCountMask);
      tb.bbox[4 * slot + 0] = 2147483647;
      tb.bbox[4 * slot + 1] = 0;
      tb.bbox[4 * slot + 2] = 2147483647;
      tb.bbox[4 * slot + 3] = 0;
      tb.row_sum[slot] = 0;
      tb.ping_sum[slot] = 0;
    }
  }
  key[i] = (unsigned long long)slot;               // from here on: the anchor's slot, -1 for a school that is dropped
}

__global__ void __launch_bounds__(kThreads)
moments_kernel(const int* __restrict__ labels, const unsigned long long* __restrict__ key, long n, int n_range, int n_pings,
               Table tb, int* __restrict__ edges) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const int p = i < n ? (int)(i % n_pings) : 0, r = i < n ? (int)(i / n_pings) : 0;
  const int label = i < n ? labels[i] : -2;
  const Run run = run_of(label, p);
  if (i >= n) return;
  const long long slot = label < 0 ? -1 : (long long)key[label];
  if (edges) {                                     // the first and the last ping column as school slots
    if (p == 0) edges[r] = (int)slot;
    if (p == n_pings - 1) edges[n_range + r] = (int)slot;
  }
  if (!run.head || slot < 0 || slot >= tb.capacity) return;
  atomicMin(tb.bbox + 4 * slot + 0, r);
  atomicMax(tb.bbox + 4 * slot + 1, r + 1);
  atomicMin(tb.bbox + 4 * slot + 2, p);
  atomicMax(tb.bbox + 4 * slot + 3, p + run.len);
  atomicAdd((unsigned long long*)tb.row_sum + slot, (unsigned long long)r * run.len);
  atomicAdd((unsigned long long*)tb.ping_sum + slot,
            (unsigned long long)run.len * (unsigned long long)(2 * (long long)p + run.len - 1) / 2ull);
}

struct Planes { long off[kMaxFreqs]; int n; };

__global__ void __launch_bounds__(kSvThreads)
sv_kernel(const int* __restrict__ labels, const float* __restrict__ sv, Planes fq, int n_range, int n_pings, long sv_ping_off,
          const long long* __restrict__ found, Table tb) {
  __shared__ double wsum[kSvThreads / 64][kMaxFreqs];
  __shared__ long long wcnt[kSvThreads / 64][kMaxFreqs];
  const long slot = blockIdx.x;
  if (slot >= found[0]) return;                    // (uniform: the whole workgroup leaves)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int anchor = tb.anchor[slot];
  const int r0 = tb.bbox[4 * slot], r1 = tb.bbox[4 * slot + 1], p0 = tb.bbox[4 * slot + 2], p1 = tb.bbox[4 * slot + 3];
  const int w = p1 - p0;
  const long area = (long)(r1 - r0) * w;
  double sum[kMaxFreqs];
  long long cnt[kMaxFreqs];
#pragma unroll
  for (int f = 0; f < kMaxFreqs; ++f) sum[f] = 0.0, cnt[f] = 0;
  for (long j = t; j < area; j += kSvThreads) {
    const int r = r0 + (int)(j / w), p = p0 + (int)(j % w);
    if (labels[(long)r * n_pings + p] != anchor) continue;
    const float* px = sv + (sv_ping_off + p) * n_range + r;
#pragma unroll
    for (int f = 0; f < kMaxFreqs; ++f) {
      if (f < fq.n) {
        const float x = px[fq.off[f]];
        if (x > 0.f && x < __builtin_inff()) sum[f] += (double)x, cnt[f] += 1;      // finite and > 0 (NaN fails both)
      }
    }
  }
#pragma unroll
  for (int f = 0; f < kMaxFreqs; ++f) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum[f] += __shfl_xor(sum[f], o, 64);
      cnt[f] += __shfl_xor(cnt[f], o, 64);
    }
    if (lane == 0) wsum[wave][f] = sum[f], wcnt[wave][f] = cnt[f];
  }
  __syncthreads();
  if (t < fq.n) {
    double s = 0.0;
    long long c = 0;
    for (int k = 0; k < kSvThreads / 64; ++k) s += wsum[k][t], c += wcnt[k][t];
    tb.sv_sum[t * tb.capacity + slot] = s;
    tb.sv_pixels[t * tb.capacity + slot] = c;
  }
}

inline long blocks_of(long n) { return (n + kThreads - 1) / kThreads; }

// what every labelling entry refuses about its plane and connectivity, before anything is launched
#define SCHOOLS_PLANE_REQUIRE(name)                                                                                          \
  CRIMAC_REQUIRE(n_range > 0 && n_pings > 0, name ": empty plane (%d x %ld)", n_range, n_pings);                              \
  CRIMAC_REQUIRE(n_pings <= 2147483647L / n_range, name ": %d x %ld pixels: the labels are 32-bit indices, "                 \
                 "n_range * n_pings must be below 2^31", n_range, n_pings);                                                  \
  CRIMAC_REQUIRE(connectivity == 4 || connectivity == 8, name ": connectivity=%d (4 or 8)", connectivity)

// the launches of every labelling entry: one 4-byte memset, tiles by the rule `fg`, borders, flatten
template <class Fg>
int label_plane(const Fg& fg, int n_range, long n_pings, int connectivity, int* labels, int* status, hipStream_t st) {
  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
    crimac_set_error("schools_label: hipMemsetAsync failed");
    return CRIMAC_ERR_LAUNCH;
  }
  const int np = (int)n_pings, tiles_p = (np + CCL_TILE_W - 1) / CCL_TILE_W;
  const long tiles = (long)tiles_p * ((n_range + CCL_TILE_H - 1) / CCL_TILE_H), n = (long)n_range * n_pings;
  hipLaunchKernelGGL(label_tiles_kernel<Fg>, dim3((unsigned)tiles), dim3(kThreads), 0, st, fg, n_range, np, connectivity,
                     tiles_p, labels, status);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(merge_borders_kernel, dim3((unsigned)tiles), dim3(CCL_TILE_W + CCL_TILE_H), 0, st, labels, n_range, np,
                     connectivity, tiles_p, status);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(flatten_kernel, dim3((unsigned)blocks_of(n)), dim3(kThreads), 0, st, labels, n, status);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

// row k of an overlap table lies in the schools a[anchor[k]] and b[anchor[k]]
__global__ void __launch_bounds__(kThreads)
pair_anchors_kernel(const int* __restrict__ anchor, const long long* __restrict__ found, long capacity,
                    const int* __restrict__ a, const int* __restrict__ b, int* __restrict__ pair) {
  const long k = (long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= capacity || k >= found[0]) return;
  const int at = anchor[k];
  pair[2 * k] = a[at];
  pair[2 * k + 1] = b[at];
}

}  // namespace

extern "C" int crimac_schools_label(const void* pred, int pred_f16, int n_range, long n_pings, float threshold,
                                    int connectivity, int* labels, int* status, void* stream) {
  CRIMAC_REQUIRE(pred && labels && status, "schools_label: null pointer");
  CRIMAC_REQUIRE(pred_f16 == 0 || pred_f16 == 1, "schools_label: pred_f16 is 0 or 1");
  SCHOOLS_PLANE_REQUIRE("schools_label");
  CRIMAC_REQUIRE(threshold > 0.f, "schools_label: threshold=%g must be > 0 (pixels the scatter left at 0 are background)",
                 (double)threshold);
  const hipStream_t st = (hipStream_t)stream;
  if (pred_f16) return label_plane(PredFg<half_t>{(const half_t*)pred, threshold}, n_range, n_pings, connectivity, labels, status, st);
  return label_plane(PredFg<float>{(const float*)pred, threshold}, n_range, n_pings, connectivity, labels, status, st);
}

extern "C" int crimac_schools_label_ids(const short* ids, long ids_pings, long ids_ping_off, int n_range, long n_pings,
                                        int select, int connectivity, int* labels, int* status, void* stream) {
  CRIMAC_REQUIRE(ids && labels && status, "schools_label_ids: null pointer");
  SCHOOLS_PLANE_REQUIRE("schools_label_ids");
  CRIMAC_REQUIRE(ids_ping_off >= 0 && ids_ping_off <= ids_pings && n_pings <= ids_pings - ids_ping_off,
                 "schools_label_ids: id columns [%ld, %ld) outside the id extent of %ld pings", ids_ping_off,
                 ids_ping_off + n_pings, ids_pings);
  CRIMAC_REQUIRE(select >= 0 || select == CRIMAC_SCHOOLS_IDS_IGNORED, "schools_label_ids: select=%d (an id >= 0, or "
                 "CRIMAC_SCHOOLS_IDS_IGNORED = %d)", select, CRIMAC_SCHOOLS_IDS_IGNORED);
  return label_plane(IdsFg{ids, ids_ping_off, select}, n_range, n_pings, connectivity, labels, status, (hipStream_t)stream);
}

extern "C" int crimac_schools_label_both(const int* a, const int* b, int n_range, long n_pings, int connectivity, int* labels,
                                         int* status, void* stream) {
  CRIMAC_REQUIRE(a && b && labels && status, "schools_label_both: null pointer");
  SCHOOLS_PLANE_REQUIRE("schools_label_both");
  return label_plane(BothFg{a, b}, n_range, n_pings, connectivity, labels, status, (hipStream_t)stream);
}

extern "C" int crimac_schools_pair_anchors(const int* anchor, const long long* found, long capacity, const int* a, const int* b,
                                           int* pair, void* stream) {
  CRIMAC_REQUIRE(anchor && found && a && b && pair, "schools_pair_anchors: null pointer");
  CRIMAC_REQUIRE(capacity >= 1 && capacity <= 2147483647L, "schools_pair_anchors: capacity=%ld (1 .. 2^31 - 1)", capacity);
  hipLaunchKernelGGL(pair_anchors_kernel, dim3((unsigned)blocks_of(capacity)), dim3(kThreads), 0, (hipStream_t)stream, anchor,
                     found, capacity, a, b, pair);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_schools_stats(const int* labels, int n_range, long n_pings, const float* sv, long plane_stride,
                                    int n_planes, const int* channels, int n_freqs, long data_pings, long sv_ping_off,
                                    long long min_pixels, int keep_left, int keep_right, long capacity, int* anchor,
                                    long long* pixels, int* bbox, long long* row_sum, long long* ping_sum, double* sv_sum,
                                    long long* sv_pixels, long long* found, int* edges, void* scratch, long scratch_bytes,
                                    void* stream) {
  CRIMAC_REQUIRE(labels && sv && channels && anchor && pixels && bbox && row_sum && ping_sum && sv_sum && sv_pixels && found &&
                 scratch, "schools_stats: null pointer");
  CRIMAC_REQUIRE(n_range > 0 && n_pings > 0 && n_pings <= 2147483647L / n_range, "schools_stats: %d x %ld pixels (positive, "
                 "n_range * n_pings below 2^31)", n_range, n_pings);
  CRIMAC_REQUIRE(n_freqs >= 1 && n_freqs <= kMaxFreqs, "schools_stats: n_freqs=%d (1 .. CRIMAC_SCHOOLS_MAX_FREQS = %d)",
                 n_freqs, kMaxFreqs);
  CRIMAC_REQUIRE(n_planes >= 1, "schools_stats: n_planes=%d", n_planes);
  for (int i = 0; i < n_freqs; ++i)
    CRIMAC_REQUIRE(channels[i] >= 0 && channels[i] < n_planes, "schools_stats: channels[%d]=%d of %d sv planes", i, channels[i],
                   n_planes);
  CRIMAC_REQUIRE(sv_ping_off >= 0 && sv_ping_off + n_pings <= data_pings, "schools_stats: sv columns [%ld, %ld) outside the sv "
                 "extent of %ld pings", sv_ping_off, sv_ping_off + n_pings, data_pings);
  CRIMAC_REQUIRE(data_pings <= 9223372036854775807L / n_range && plane_stride >= data_pings * n_range,
                 "schools_stats: plane_stride=%ld: a plane of %ld pings x %d rows would leave the sv extent", plane_stride,
                 data_pings, n_range);
  CRIMAC_REQUIRE(min_pixels >= 1, "schools_stats: min_pixels=%lld must be >= 1", min_pixels);
  CRIMAC_REQUIRE(capacity >= 1 && capacity <= 2147483647L, "schools_stats: capacity=%ld (1 .. 2^31 - 1)", capacity);
  const long n = (long)n_range * n_pings, nb = blocks_of(n);
  const long need = CRIMAC_SCHOOLS_SCRATCH_PIXEL_BYTES * n + 16;
  CRIMAC_REQUIRE(scratch_bytes >= need && (uintptr_t)scratch % 8 == 0, "schools_stats: scratch of %ld bytes, this launch needs "
                 "%ld (8-byte aligned; CRIMAC_SCHOOLS_SCRATCH_PIXEL_BYTES * n_range * n_pings + 16)", scratch_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* key = (unsigned long long*)scratch;
  int* block_cnt = (int*)(key + n);
  const int np = (int)n_pings;
  Table tb{anchor, pixels, bbox, row_sum, ping_sum, sv_sum, sv_pixels, capacity};
  Planes fq{};
  fq.n = n_freqs;
  for (int i = 0; i < n_freqs; ++i) fq.off[i] = channels[i] * plane_stride;
  if (hipMemsetAsync(key, 0, (size_t)n * 8, st) != hipSuccess) {
    crimac_set_error("schools_stats: hipMemsetAsync failed");
    return CRIMAC_ERR_LAUNCH;
  }
  const dim3 grid((unsigned)nb), block(kThreads);
  hipLaunchKernelGGL(count_kernel, grid, block, 0, st, labels, n, np, keep_left, keep_right, key);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_count_kernel, grid, block, 0, st, labels, (const unsigned long long*)key, n, min_pixels, block_cnt);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(kSvThreads), 0, st, block_cnt, nb, found);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_assign_kernel, grid, block, 0, st, labels, key, n, min_pixels, (const int*)block_cnt, tb);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(moments_kernel, grid, block, 0, st, labels, (const unsigned long long*)key, n, n_range, np, tb, edges);
  CRIMAC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sv_kernel, dim3((unsigned)capacity), dim3(kSvThreads), 0, st, labels, sv, fq, n_range, np, sv_ping_off,
                     (const long long*)found, tb);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}
