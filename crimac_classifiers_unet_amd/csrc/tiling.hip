// Tiled whole-survey inference plumbing on the GPU (CDNA4 / gfx950), HBM-bound byte movers.
//
// Reference: save_survey_predictions_zarr's per-patch host work (save_predict.py:160-209):
//   * DatasetGriddedReader.get_preload_data_labels -> new_get_crop_3d (dataset.py:192-205,
//     utils/np.py:361-375): gather a 256x256 crop around each grid centre from the preloaded chunk,
//     0 outside the chunk;
//   * remove_nan_inf + db_with_limits (remove_nan_inf.py:23-34, db_with_limits.py:20-24, :36-38):
//     non-finite -> 0, 10*log10(x + 1e-10) clamped to [-75, 0];
//   * fill_out_array (save_predict.py:41-65) with the validity rules of the test-time label
//     transforms (convert_label_indexing_unused_species, mask_label_seabed, mask_label_overlap,
//     remove_nan_inf): scatter softmax channels [SANDEEL, OTHER] of each patch's valid interior into
//     the chunk's [2, range, pings] output.
//
// The chunk stays resident in HBM in the reader's own (zarr) orientation [freq][ping][range] (range
// contiguous); the gather transposes through LDS so both the reads (along range) and the NHWC writes
// (along ping, 16 channels per pixel) are coalesced, and the dB transform, channel padding and
// bf16/fp32 conversion are fused into it -- the patch lands directly in the first conv's input layout.
#include "common.h"
#include "meta_planes.h"
#include "pr_softmax.h"

namespace {

constexpr int TS = 32;   // tile side

// Where the patches of a launch are read from.  descs == NULL: ONE source for all of them, given as scalars -- data
// [C][Wd][H] fp32, labels [Wd][H] int16 (or NULL).  Otherwise (batches that span memmap echograms,
// tiled_inference.predict_echograms_memm / evaluate_echograms_memm) src[p] picks patch p's crimac_memm_desc from a
// device-resident table, and data, labels and both extents are that echogram's.  A block works on one patch (blockIdx.z),
// so src[p], the descriptor load and the early return for a src[p] that names no descriptor are uniform over the block.
// Both forms run the same kernel, hence the same body: the same bits.
static_assert(sizeof(crimac_memm_desc) == 48, "crimac_memm_desc: six 64-bit fields (hip.MEMM_DESC_WORDS)");
struct PatchSrc {
  const float* data; int Wd, H; const short* labels;
  const crimac_memm_desc* descs; int n_desc; const int* src;
  __device__ __forceinline__ bool resolve(int p) {
    if (!descs) return true;
    const int i = src[p];
    if (i < 0 || i >= n_desc) return false;
    const crimac_memm_desc d = descs[i];
    data = d.data; Wd = (int)d.n_pings; H = (int)d.n_range; labels = d.labels;
    return true;
  }
  bool ok() const { return descs ? src && n_desc > 0 : data && Wd > 0 && H > 0; }      // (host: the launchers' check)
};
// meta.metas != NULL (crimac_gather_patches_memm_meta_multi): the metadata vectors of patch p come from a second table,
// indexed by the same src[p] and resolved where `from` is, uniformly over the block.
struct GatherSrc { PatchSrc from; int db_scaled; MetaPlaneSrc meta; const int* meta_centres; };

// data [C][Wd][H] fp32; centres [P][2] = (cy, cx_local) with cx_local relative to the chunk slice.
// border_labels != NULL (memm flavour, save_predict.py:222-265; the source's labels, a descriptor without labels gets no
// border rule): labels [Wd][H] int16 raw annotation ids covering the same extent as `data`; a pixel outside that extent,
// or whose raw label the test-time label transform maps to "ignore" (convert_label_indexing: negative ids), gets 0.0
// AFTER the dB transform in every channel
// (set_data_border_value, batch/data_transforms/set_data_border_value.py:20-23, last step of define_data_transform_test).
// meta.flags != 0 (early metadata injection, crimac_gather_patches_memm_meta): channels C .. C+Cm-1 of every pixel get
// the crop's metadata planes (meta_plane_values, crop centred on meta_centres[p] = (range idx, GLOBAL ping idx)), which
// neither the dB transform nor the border rule touches (batch/dataset.py:109: np.concatenate((data, meta)) after the
// data transform); db_scaled: db_with_limits_scaled (1 + dB / 75, define_data_transform_test(use_metadata=True)).
// PATCH_LABELS (crimac_gather_patches_memm_labels): the border rule is read off patch_labels [P][ph][pw] int16 instead --
// the labels of the patch AFTER the test-time label transform, which is what set_data_border_value sees
// (batch/dataset.py:229-235): a pixel whose transformed label is -100 gets 0.0, every other pixel its dB value, in or
// outside the extent of `data`.  The labels are those of get_crop_memmap's crop (crimac_gather_eval_crops, flavour 1), so
// the data crop takes its centre row too: H / 2 when the window covers the whole water column (dataset.py:259-261).
// The body of one block = one 32 x 32 tile of patch blockIdx.z; gather_patches_kernel hands it the source of that patch.
template <typename T, bool PATCH_LABELS>
__device__ __forceinline__ void gather_patch_tile(const float* __restrict__ data, int C, int Wd, int H,
                                                  const int* __restrict__ centres, int ph, int pw,
                                                  T* __restrict__ out, int ld,
                                                  const short* __restrict__ border_labels, int db_scaled,
                                                  const MetaPlaneSrc& meta, const int* __restrict__ meta_centres,
                                                  const short* __restrict__ patch_labels) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* tile = reinterpret_cast<float*>(smem_raw);      // [C][TS (x)][TS + 1 (y)]
  const int p = blockIdx.z;
  const int ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS;
  const int cy = PATCH_LABELS && H <= ph ? H / 2 : centres[2 * p], cx = centres[2 * p + 1];
  const int y_base = cy - ((ph + 1) / 2) + 1 + ty0;        // data row of tile row 0 (np.py:40-46)
  const int x_base = cx - ((pw + 1) / 2) + 1 + tx0;
  const int tx = threadIdx.x & 31, tr = threadIdx.x >> 5;  // tr 0..7
  // read phase: lanes run along range (contiguous in the chunk)
  bool border[4] = {false, false, false, false};
  if (border_labels) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x_base + tr + 8 * k, y = y_base + tx;
      const bool inside = x >= 0 && x < Wd && y >= 0 && y < H;
      border[k] = !inside || border_labels[(long)x * H + y] < 0;
    }
  }
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xi = tr + 8 * k;                 // tile column (ping)
      const int x = x_base + xi, y = y_base + tx;
      float v = 0.f;                             // boundary_val_data = 0 (dataset.py:195)
      if (x >= 0 && x < Wd && y >= 0 && y < H && (ty0 + tx) < ph && (tx0 + xi) < pw)
        v = data[((long)c * Wd + x) * H + y];
      if (!isfinite(v)) v = 0.f;                 // remove_nan_inf
      v = 10.f * log10f(v + 1e-10f);             // db_with_limits
      v = fminf(fmaxf(v, -75.f), 0.f);
      if (db_scaled) v = 1.f + v / 75.f;         // db_with_limits_scaled (db_with_limits.py:27-33)
      if (border[k]) v = 0.f;                    // set_data_border_value
      tile[(c * TS + xi) * (TS + 1) + tx] = v;
    }
  }
  __syncthreads();
  // write phase: lanes run along ping (contiguous pixels of the NHWC patch)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yi = tr + 8 * k;
    const int py = ty0 + yi, px = tx0 + tx;
    if (py >= ph || px >= pw) continue;
    T* dst = out + (((long)p * ph + py) * pw + px) * ld;
    // (lanes along ping: the labels of the patch are read as they are written, contiguously)
    const bool keep = !PATCH_LABELS || patch_labels[((long)p * ph + py) * pw + px] != -100;
    float mv[CRIMAC_MAX_META_PLANES];
    int Cm = 0;
    if (meta.flags) {
      meta_plane_values(meta, meta_centres[2 * p], meta_centres[2 * p + 1], ph, pw, py, px, mv);
      Cm = meta_plane_count(meta.flags);
    }
    for (int c0 = 0; c0 < ld; c0 += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = c0 + j;
        v[j] = ch < C ? (keep ? tile[(ch * TS + tx) * (TS + 1) + yi] : 0.f) : ch < C + Cm ? mv[ch - C] : 0.f;
      }
      store8(dst + c0, v);
    }
  }
}

template <typename T, bool PATCH_LABELS>
__global__ __launch_bounds__(256) void gather_patches_kernel(GatherSrc g, int C, const int* __restrict__ centres, int ph,
                                                             int pw, T* __restrict__ out, int ld,
                                                             const short* __restrict__ patch_labels) {
  PatchSrc& s = g.from;
  if (!s.resolve(blockIdx.z)) return;                      // (uniform over the block: nobody waits at the barrier)
  if (g.meta.flags && !g.meta.resolve(blockIdx.z)) return; // (so is this)
  gather_patch_tile<T, PATCH_LABELS>(s.data, C, s.Wd, s.H, centres, ph, pw, out, ld, PATCH_LABELS ? nullptr : s.labels,
                                     g.db_scaled, g.meta, g.meta_centres, patch_labels);
}

// probs [P][ncls][ph][pw] fp32; centres [P][2] global (cy, cx); out [2][H][n_chunk] fp32 (or fp16).
struct ScatterParams {
  const float* probs; int ncls; const int* centres; int P, ph, pw, overlap, start_ping, n_chunk, H;
  const short* labels;
  const unsigned char* seabed_mask; int mask_ping0, mask_pings;
  const int* seabed; int seabed_ping0, seabed_pings;     // seabed index per ping: replaces seabed_mask when given
  const float* data0; int data_ping0, data_pings;
  int seabed_pad;
  int seabed_rule;          // 0: zarr reader (pad shifts the mask inside the patch's slice), 1: Echogram (absolute rows)
  void* out; int out_f16;
};
__global__ __launch_bounds__(256) void scatter_patches_kernel(ScatterParams q) {
  const int ph = q.ph, pw = q.pw, overlap = q.overlap, H = q.H;
  const int iw = pw - 2 * overlap, ih = ph - 2 * overlap;
  const long per_patch = (long)ih * iw;
  const long total = per_patch * q.P;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int p = (int)(i / per_patch);
    const int r = (int)(i % per_patch);
    const int py = overlap + r / iw, px = overlap + r % iw;      // mask_label_overlap: rim excluded
    const int cy = q.centres[2 * p], cx = q.centres[2 * p + 1];
    const int y = cy - ph / 2 + 1 + py, x = cx - pw / 2 + 1 + px;   // patch_coord_to_data_coord
    const int xl = x - q.start_ping;
    if (y < 0 || y >= H || xl < 0 || xl >= q.n_chunk) continue;     // label crop out of range: -100
    int lab = q.labels ? (int)q.labels[(long)xl * H + y] : 0;
    if (lab < 0) continue;                                           // convert_label_indexing: -100
    if (lab == 0 && (q.seabed_mask || q.seabed)) {                   // mask_label_seabed (background only)
      // zarr reader: rows of the patch's own slice, shifted down by the pad inside the slice; Echogram: absolute
      const int y_top = q.seabed_rule == 0 ? max(cy - ph / 2 + 1, 0) : 0;
      if (y - y_top >= q.seabed_pad) {
        bool below = false;
        if (q.seabed) {
          const int xs = x - q.seabed_ping0;
          below = xs >= 0 && xs < q.seabed_pings && (y - q.seabed_pad) >= q.seabed[xs];
        } else {
          const int xm = x - q.mask_ping0;
          below = xm >= 0 && xm < q.mask_pings && q.seabed_mask[(long)xm * H + (y - q.seabed_pad)];
        }
        if (below) continue;
      }
    }
    if (q.data0) {                                                   // remove_nan_inf: ch 0 non-finite
      const int xd = x - q.data_ping0;
      if (xd >= 0 && xd < q.data_pings && !isfinite(q.data0[(long)xd * H + y])) continue;
    }
    const long src = (((long)p * q.ncls + 1) * ph + py) * pw + px;   // channel SANDEEL = 1
    const long d0 = ((long)0 * H + y) * q.n_chunk + xl, d1 = ((long)1 * H + y) * q.n_chunk + xl;
    if (q.out_f16) {                                                 // the reference stores float16 (save_predict.py:212, :252)
      reinterpret_cast<half_t*>(q.out)[d0] = (half_t)q.probs[src];
      reinterpret_cast<half_t*>(q.out)[d1] = (half_t)q.probs[src + (long)ph * pw];
    } else {
      reinterpret_cast<float*>(q.out)[d0] = q.probs[src];
      reinterpret_cast<float*>(q.out)[d1] = q.probs[src + (long)ph * pw];   // channel OTHER = 2
    }
  }
}

// scatter_patches_kernel for batches that span memmap echograms: the memm rules only (labels, seabed vector from ping 0,
// seabed_rule 1, no data0), the destination [2][n_range][n_pings], the labels, the seabed vector and the two extents
// taken from descs[src[p]] (PatchSrc's table; the grid and the rule set differ, so the kernel stays its own).
// blockIdx.y = patch.  Interiors of different patches are disjoint, within an echogram and across echograms: plain stores.
struct ScatterMultiParams {
  const float* probs; int ncls; const crimac_memm_desc* descs; int n_desc; const int* src; const int* centres;
  int ph, pw, overlap, seabed_pad, out_f16;
};
__global__ __launch_bounds__(256) void scatter_patches_multi_kernel(ScatterMultiParams q) {
  const int ph = q.ph, pw = q.pw, overlap = q.overlap;
  const int iw = pw - 2 * overlap, ih = ph - 2 * overlap;
  const int per_patch = ih * iw;
  const int p = blockIdx.y;
  const int s = q.src[p];
  if (s < 0 || s >= q.n_desc) return;
  const crimac_memm_desc d = q.descs[s];
  const long H = d.n_range, n_pings = d.n_pings;
  const int cy = q.centres[2 * p], cx = q.centres[2 * p + 1];
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < per_patch; r += gridDim.x * blockDim.x) {
    const int py = overlap + r / iw, px = overlap + r % iw;      // mask_label_overlap: rim excluded
    const int y = cy - ph / 2 + 1 + py, x = cx - pw / 2 + 1 + px;   // patch_coord_to_data_coord
    if (y < 0 || y >= H || x < 0 || x >= n_pings) continue;         // label crop out of range: -100
    const int lab = d.labels ? (int)d.labels[x * H + y] : 0;
    if (lab < 0) continue;                                           // convert_label_indexing: -100
    if (lab == 0 && d.seabed && y >= q.seabed_pad &&                 // mask_label_seabed (background only), absolute rows
        (y - q.seabed_pad) >= d.seabed[x])
      continue;
    const long sp = (((long)p * q.ncls + 1) * ph + py) * pw + px;    // channel SANDEEL = 1
    const long d0 = y * n_pings + x, d1 = (H + y) * n_pings + x;
    if (q.out_f16) {                                                 // the reference stores float16 (save_predict.py:252)
      reinterpret_cast<half_t*>(d.out)[d0] = (half_t)q.probs[sp];
      reinterpret_cast<half_t*>(d.out)[d1] = (half_t)q.probs[sp + (long)ph * pw];
    } else {
      reinterpret_cast<float*>(d.out)[d0] = q.probs[sp];
      reinterpret_cast<float*>(d.out)[d1] = q.probs[sp + (long)ph * pw];   // channel OTHER = 2
    }
  }
}

// Validation metrics (pipeline.py:242-341): histogram of the float16-rounded SANDEEL probability over
// the valid pixels, split by "label == SANDEEL".  The reference gathers every pixel's probability as
// float16 on the host and sorts them in sklearn's precision_recall_curve; float16 has < 15362
// non-negative values up to 1.0, so the two histograms hold exactly the same information.
__global__ __launch_bounds__(256) void pr_histogram_kernel(const float* __restrict__ logits, int ncls,
                                                           const void* __restrict__ labels, int lbytes,
                                                           long npix, long HW, unsigned int* hist_pos,
                                                           unsigned int* hist_neg) {
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    long l = lbytes == 8 ? ((const long long*)labels)[p] : lbytes == 4 ? ((const int*)labels)[p]
                                                                       : ((const short*)labels)[p];
    // set_label_ignore_val (pipeline.py:222-239): overlap / refined boundary / boundary / unused -> ignore
    if (l == -70 || l == -30 || l == -100 || l == -10) continue;
    const bool seabed = l == -50;            // below seabed: counts as background with probability 0
    float prob = 0.f;
    if (!seabed) {
      const long b = p / HW, hw = p % HW;
      float z[8], mx = -INFINITY, den = 0.f;
      for (int o = 0; o < ncls; ++o) { z[o] = logits[(b * ncls + o) * HW + hw]; mx = fmaxf(mx, z[o]); }
      for (int o = 0; o < ncls; ++o) { z[o] = expf(z[o] - mx); den += z[o]; }
      prob = z[1] / den;
    }
    const _Float16 h = (_Float16)prob;       // round-to-nearest-even, as numpy .astype(float16)
    unsigned short bits = *reinterpret_cast<const unsigned short*>(&h);
    // a probability is in [0, 1] = bit patterns 0 .. 0x3C00; a NaN (diverged network: 0x7E00 / 0xFE00) must not
    // index past the 16384 bins -> counted in the last bin, which no probability reaches (the host raises on it,
    // as sklearn's precision_recall_curve does on a NaN score)
    if (bits > 0x3C00) bits = CRIMAC_PR_NAN_BIN;
    atomicAdd((!seabed && l == 1) ? &hist_pos[bits] : &hist_neg[bits], 1u);
  }
}

// The same histograms for every foreground class selected by `mask` (bit c = class c), hist [ncls][2][CRIMAC_PR_BINS]:
// one softmax per pixel -- max, expf, the order of the sum and the division as above, so row 1 is that kernel's result.
// Evaluation data is skewed: every below-seabed pixel is bin 0 of `neg` of every class, and a probability under 2^-14 is
// a float16 subnormal, 6e-8 wide bins where most background pixels of a trained network collect.  So the counters of
// bins [0, PR_LDS_BINS) live in LDS, [selected class][pos, neg][bin]: a wave first adds the lanes that share the first
// active lane's counter as ONE LDS atomic (a run of seabed or background pixels is the whole wave), the other lanes add
// their own; the workgroup adds its non-zero counters to global memory once, at the end.  From 2^-14 up a float16 bin is
// no wider than 2^-10 of its value, pixels spread over many bins, and each takes one global atomic as above.
// Exact: 32-bit counters everywhere (a workgroup sees at most npix / gridDim.x + 256 pixels).
constexpr int PR_LDS_BINS = 1024;
__global__ __launch_bounds__(256) void pr_histogram_classes_kernel(const float* __restrict__ logits, int ncls,
                                                                   const void* __restrict__ labels, int lbytes,
                                                                   long npix, long HW, unsigned int mask,
                                                                   unsigned int* __restrict__ hist) {
  extern __shared__ unsigned int pr_low[];   // [popc(mask)][2][PR_LDS_BINS]
  const int n_low = __popc(mask) * 2 * PR_LDS_BINS;
  for (int i = threadIdx.x; i < n_low; i += 256) pr_low[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    long l = lbytes == 8 ? ((const long long*)labels)[p] : lbytes == 4 ? ((const int*)labels)[p]
                                                                       : ((const short*)labels)[p];
    if (l == -70 || l == -30 || l == -100 || l == -10) continue;
    const bool seabed = l == -50;
    float z[8], den = 0.f;
    if (!seabed) {
      const long b = p / HW, hw = p % HW;
      pr_softmax_terms(logits + b * ncls * HW + hw, HW, ncls, z, den);
    }
#pragma unroll
    for (int c = 1; c < 8; ++c) {
      if (!((mask >> c) & 1u)) continue;       // (uniform; the entry point admits bits 1 .. ncls-1 only)
      const _Float16 h = seabed ? (_Float16)0.f : pr_prob_f16(z[c], den);
      unsigned short bits = *reinterpret_cast<const unsigned short*>(&h);
      if (bits > 0x3C00) bits = CRIMAC_PR_NAN_BIN;
      const int side = (!seabed && l == c) ? 0 : 1;
      if (bits < PR_LDS_BINS) {
        const int key = ((__popc(mask & ((1u << c) - 1u)) * 2) + side) * PR_LDS_BINS + bits;
        const int first = __builtin_amdgcn_readfirstlane(key);
        const unsigned long long same = __ballot(key == first);
        if (key != first) atomicAdd(&pr_low[key], 1u);
        else if (lane == __ffsll(same) - 1) atomicAdd(&pr_low[key], (unsigned int)__popcll(same));
      } else {
        atomicAdd(&hist[((long)c * 2 + side) * CRIMAC_PR_BINS + bits], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_low; i += 256) {
    const unsigned int v = pr_low[i];
    if (!v) continue;
    unsigned int m = mask;                     // class of slot i / (2 * PR_LDS_BINS): that many set bits of the mask down
    for (int k = i / (2 * PR_LDS_BINS); k > 0; --k) m &= m - 1u;
    const int c = __ffs(m) - 1;
    atomicAdd(&hist[(long)c * 2 * CRIMAC_PR_BINS + (i / PR_LDS_BINS % 2) * CRIMAC_PR_BINS + i % PR_LDS_BINS], v);
  }
}

// RAW evaluation crops (the per-patch crop of the reference's gridded test Dataset, before any transform): for patch p
//   data_out [P][C][ph][pw] fp32 linear sv, labels_out [P][ph][pw] int16 raw annotation ids
// from the resident chunk data [C][Wd][H] / labels [Wd][H].  flavour 0 = get_crop_zarr (dataset.py:358-407): the patch
// is placed by patch_coord_to_data_coord (centre - size / 2 + 1), data 0 / label -100 outside, nan_to_num on the data
// (NaN -> 0, +-inf -> the largest finite value, here of fp32); flavour 1 = get_crop_memmap (dataset.py:254-287): placed
// by getGrid (centre - (size + 1) / 2 + 1), DATA_BOUNDARY_VAL 0 / LABEL_BOUNDARY_VAL -100 outside, every non-finite sample
// 0, and a water column not deeper than the patch puts the centre row at H / 2.
// A pure streaming transpose: one 32 x 32 tile per block and plane, lanes along range (contiguous in the chunk) when
// reading, along ping (contiguous in the crop) when writing; `vec`: 16-byte stores (pw % 8 == 0, 16-byte aligned bases).
// One block = one 32 x 32 tile of patch blockIdx.z.  With a descriptor table (flavour 1 only) the centre-row rule of a
// water column not deeper than the patch is the patch's own echogram's; a descriptor without data or labels is skipped.
//
// eval_crop_origin: the placement rule itself -- the (row, ping) of crop pixel (0, 0) in the coordinates of the centre --
// which crimac_eval_crop_origins hands to whoever must know where a crop's pixels lie (crimac_integrate_confusion).
__device__ __forceinline__ void eval_crop_origin(int cy, int cx, int ph, int pw, int H, int flavour, int& y0, int& x0) {
  if (flavour == 1 && H <= ph) cy = H / 2;                  // dataset.py:259-261
  y0 = cy - (flavour == 1 ? (ph + 1) / 2 : ph / 2) + 1;
  x0 = cx - (flavour == 1 ? (pw + 1) / 2 : pw / 2) + 1;
}

// `s`: H alone (crimac_eval_crop_origins) or the descriptor table (crimac_eval_crop_origins_multi: H is the n_range of the
// patch's own echogram, and a patch whose src names no descriptor gets no write)
__global__ __launch_bounds__(256) void eval_crop_origins_kernel(PatchSrc s, const int* __restrict__ centres, int P, int ph,
                                                                int pw, int flavour, int* __restrict__ origins) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P || !s.resolve(p)) return;
  int y0, x0;
  eval_crop_origin(centres[2 * p], centres[2 * p + 1], ph, pw, s.H, flavour, y0, x0);
  origins[2 * p] = y0;
  origins[2 * p + 1] = x0;
}

__global__ __launch_bounds__(256) void gather_eval_crops_kernel(PatchSrc s, int C, const int* __restrict__ centres, int ph,
                                                                int pw, int flavour, int vec, float* __restrict__ data_out,
                                                                short* __restrict__ labels_out) {
  if (!s.resolve(blockIdx.z) || !s.data || !s.labels) return;      // (uniform over the block: nobody waits at a barrier)
  const float* __restrict__ data = s.data;
  const short* __restrict__ labels = s.labels;
  const int Wd = s.Wd, H = s.H;
  __shared__ float tile[TS][TS + 1];          // [x (ping)][y (range)]
  __shared__ short ltile[TS][TS + 2];
  const int p = blockIdx.z;
  const int ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS;
  int y_base, x_base;
  eval_crop_origin(centres[2 * p], centres[2 * p + 1], ph, pw, H, flavour, y_base, x_base);
  y_base += ty0;
  x_base += tx0;
  const int tx = threadIdx.x & 31, tr = threadIdx.x >> 5;   // read phase: tx along range, tr + 8k along ping
  const int y = y_base + tx;
  // labels
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xi = tr + 8 * k, x = x_base + xi;
    short l = -100;
    if (x >= 0 && x < Wd && y >= 0 && y < H) l = labels[(long)x * H + y];
    ltile[xi][tx] = l;
  }
  __syncthreads();
  if (threadIdx.x < 128) {                                  // 32 rows x 4 groups of 8 pings
    const int yi = threadIdx.x >> 2, q = threadIdx.x & 3;
    const int py = ty0 + yi, px = tx0 + 8 * q;
    if (py < ph && px < pw) {
      short* dst = labels_out + ((long)p * ph + py) * pw + px;
      if (vec) {                                            // (pw % 8 == 0: the whole group lies inside the row)
        u16x8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (unsigned short)ltile[8 * q + j][yi];
        *reinterpret_cast<u16x8*>(dst) = r;
      } else {
        for (int j = 0; j < 8 && px + j < pw; ++j) dst[j] = ltile[8 * q + j][yi];
      }
    }
  }
  // data planes
  const int yi = threadIdx.x >> 3, q = threadIdx.x & 7;     // write phase: 32 rows x 8 groups of 4 pings
  const int py = ty0 + yi, px = tx0 + 4 * q;
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xi = tr + 8 * k, x = x_base + xi;
      float v = 0.f;
      if (x >= 0 && x < Wd && y >= 0 && y < H) v = data[((long)c * Wd + x) * H + y];
      if (flavour == 1) {
        if (!isfinite(v)) v = 0.f;
      } else {
        if (v != v) v = 0.f;                                // np.nan_to_num
        v = fminf(fmaxf(v, -3.402823466e+38f), 3.402823466e+38f);
      }
      tile[xi][tx] = v;
    }
    __syncthreads();
    if (py < ph && px < pw) {
      float* dst = data_out + (((long)p * C + c) * ph + py) * pw + px;
      if (vec) {
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = tile[4 * q + j][yi];
        *reinterpret_cast<f32x4*>(dst) = r;
      } else {
        for (int j = 0; j < 4 && px + j < pw; ++j) dst[j] = tile[4 * q + j][yi];
      }
    }
    __syncthreads();
  }
}

}  // namespace

static int eval_crops_run(const char* name, const PatchSrc& s, int C, const int* centres, int P, int ph, int pw,
                          int flavour, float* data_out, short* labels_out, void* stream) {
  CRIMAC_REQUIRE(s.ok() && (s.descs || s.labels) && centres && data_out && labels_out && C > 0 && P > 0 && ph > 0 && pw > 0,
                 "%s: bad arguments", name);
  CRIMAC_REQUIRE(P <= 65535, "%s: at most 65535 patches per call", name);
  const int vec = pw % 8 == 0 && ((uintptr_t)data_out & 15) == 0 && ((uintptr_t)labels_out & 15) == 0;
  dim3 grid((pw + TS - 1) / TS, (ph + TS - 1) / TS, P);
  hipLaunchKernelGGL(gather_eval_crops_kernel, grid, dim3(256), 0, (hipStream_t)stream, s, C, centres, ph, pw, flavour,
                     vec, data_out, labels_out);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_gather_eval_crops(const float* data, int C, int Wd, int H, const short* labels, const int* centres,
                                        int P, int ph, int pw, int flavour, float* data_out, short* labels_out,
                                        void* stream) {
  CRIMAC_REQUIRE(flavour == 0 || flavour == 1, "gather_eval_crops: flavour=%d (0 zarr, 1 memm)", flavour);
  return eval_crops_run("gather_eval_crops", PatchSrc{data, Wd, H, labels}, C, centres, P, ph, pw, flavour, data_out,
                        labels_out, stream);
}

extern "C" int crimac_gather_eval_crops_multi(const crimac_memm_desc* descs, int n_desc, const int* src, int C,
                                              const int* centres, int P, int ph, int pw, float* data_out,
                                              short* labels_out, void* stream) {
  CRIMAC_REQUIRE(descs, "gather_eval_crops_multi: needs the descriptor table");
  return eval_crops_run("gather_eval_crops_multi", PatchSrc{nullptr, 0, 0, nullptr, descs, n_desc, src}, C, centres, P,
                        ph, pw, 1, data_out, labels_out, stream);
}

extern "C" int crimac_eval_crop_origins(const int* centres, int P, int ph, int pw, int H, int flavour, int* origins,
                                        void* stream) {
  CRIMAC_REQUIRE(centres && origins && P > 0 && ph > 0 && pw > 0 && H > 0, "eval_crop_origins: bad arguments");
  CRIMAC_REQUIRE(flavour == 0 || flavour == 1, "eval_crop_origins: flavour=%d (0 zarr, 1 memm)", flavour);
  hipLaunchKernelGGL(eval_crop_origins_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     PatchSrc{nullptr, 0, H}, centres, P, ph, pw, flavour, origins);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_eval_crop_origins_multi(const crimac_memm_desc* descs, int n_desc, const int* src, const int* centres,
                                              int P, int ph, int pw, int* origins, void* stream) {
  const PatchSrc s{nullptr, 0, 0, nullptr, descs, n_desc, src};
  CRIMAC_REQUIRE(descs && s.ok() && centres && origins && P > 0 && ph > 0 && pw > 0, "eval_crop_origins_multi: bad arguments");
  hipLaunchKernelGGL(eval_crop_origins_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s,
                     centres, P, ph, pw, 1, origins);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_pr_histogram(const float* logits, int ncls, const void* labels, int label_bytes,
                                   int B, int H, int W, unsigned int* hist_pos, unsigned int* hist_neg,
                                   void* stream) {
  CRIMAC_REQUIRE(logits && labels && hist_pos && hist_neg && B > 0 && H > 0 && W > 0 && ncls >= 2 && ncls <= 8,
                 "pr_histogram: bad arguments");
  CRIMAC_REQUIRE(label_bytes == 2 || label_bytes == 4 || label_bytes == 8, "pr_histogram: label_bytes=%d", label_bytes);
  const long HW = (long)H * W, npix = B * HW;
  long blocks = (npix + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pr_histogram_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits, ncls,
                     labels, label_bytes, npix, HW, hist_pos, hist_neg);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_pr_histogram_classes(const float* logits, int ncls, const void* labels, int label_bytes, int B,
                                           int H, int W, unsigned int class_mask, unsigned int* hist, void* stream) {
  CRIMAC_REQUIRE(logits && labels && hist && B > 0 && H > 0 && W > 0 && ncls >= 2 && ncls <= 8,
                 "pr_histogram_classes: bad arguments");
  CRIMAC_REQUIRE(label_bytes == 2 || label_bytes == 4 || label_bytes == 8, "pr_histogram_classes: label_bytes=%d",
                 label_bytes);
  CRIMAC_REQUIRE(class_mask != 0u && !(class_mask & 1u) && !(class_mask >> ncls),
                 "pr_histogram_classes: class_mask=0x%x must select foreground classes 1 .. %d only", class_mask, ncls - 1);
  const long HW = (long)H * W, npix = B * HW;
  long blocks = (npix + 1023) / 1024;          // four pixels or more per thread: fewer workgroups flush their LDS counters
  if (blocks > 1024) blocks = 1024;
  const size_t lds = (size_t)__builtin_popcount(class_mask) * 2 * PR_LDS_BINS * sizeof(unsigned int);   // <= 56 KiB
  hipLaunchKernelGGL(pr_histogram_classes_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, logits,
                     ncls, labels, label_bytes, npix, HW, class_mask, hist);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

// The one launcher of the gather family; `name`: the entry point the caller used.  patch_labels picks PATCH_LABELS.
static int gather_run(const char* name, int prec, const GatherSrc& g, int C, const int* centres, int P, int ph, int pw,
                      void* out, long ld, void* stream, const short* patch_labels = nullptr) {
  const MetaPlaneSrc& m = g.meta;
  CRIMAC_REQUIRE(prec >= CRIMAC_PREC_BF16 && prec <= CRIMAC_PREC_MAX, "%s: bad precision %d", name, prec);
  CRIMAC_REQUIRE(g.from.ok() && centres && out && C > 0 && C <= 16 && P > 0 && ph > 0 && pw > 0,
                 "%s: bad arguments (C=%d must be <= 16)", name, C);
  CRIMAC_REQUIRE(ld >= C && ld % 8 == 0 && ld <= 16, "%s: ld=%ld must be 8 or 16 and >= C", name, ld);
  CRIMAC_REQUIRE(P <= 65535, "%s: at most 65535 patches per call", name);
  CRIMAC_REQUIRE(m.flags >= 0 && m.flags < 64, "%s: bad metadata flags %d", name, m.flags);
  CRIMAC_REQUIRE(!m.flags || g.meta_centres, "%s: metadata planes need the global centres", name);
  // (the table form: a descriptor that lacks a vector the flags need makes its patches skipped, MetaPlaneSrc::resolve)
  CRIMAC_REQUIRE(m.metas || !(m.flags & 2) || (m.portion_day && m.n_day > 0), "%s: portion_day needs its vector", name);
  CRIMAC_REQUIRE(m.metas || !(m.flags & 4) || (m.time_diff && m.n_td > 0), "%s: time_diff needs its vector", name);
  CRIMAC_REQUIRE(m.metas || !(m.flags & 56) || (m.seabed && m.n_sb > 0), "%s: the depth planes need the seabed vector", name);
  CRIMAC_REQUIRE(C + meta_plane_count(m.flags) <= ld, "%s: %d data + %d metadata channels do not fit ld=%ld", name, C,
                 meta_plane_count(m.flags), ld);
  dim3 grid((pw + TS - 1) / TS, (ph + TS - 1) / TS, P);
  const size_t lds = (size_t)C * TS * (TS + 1) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (patch_labels) {
    CRIMAC_FOR_STORAGE2(prec, TF_, T, hipLaunchKernelGGL((gather_patches_kernel<T, true>), grid, dim3(256), lds, st, g, C,
                                                   centres, ph, pw, (T*)out, (int)ld, patch_labels));
  } else {
    CRIMAC_FOR_STORAGE2(prec, TF_, T, hipLaunchKernelGGL((gather_patches_kernel<T, false>), grid, dim3(256), lds, st, g, C,
                                                   centres, ph, pw, (T*)out, (int)ld, patch_labels));
  }
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_gather_patches(int prec, const float* data, int C, int Wd, int H, const int* centres,
                                     int P, int ph, int pw, void* out, long ld, void* stream) {
  return gather_run("gather_patches", prec, GatherSrc{{data, Wd, H}}, C, centres, P, ph, pw, out, ld, stream);
}

extern "C" int crimac_gather_patches_memm(int prec, const float* data, int C, int Wd, int H, const int* centres,
                                          int P, int ph, int pw, void* out, long ld, const short* border_labels,
                                          void* stream) {
  CRIMAC_REQUIRE(border_labels, "gather_patches_memm: needs the label array (border rule)");
  return gather_run("gather_patches_memm", prec, GatherSrc{{data, Wd, H, border_labels}}, C, centres, P, ph, pw, out, ld,
                    stream);
}

extern "C" int crimac_gather_patches_memm_meta(int prec, const float* data, int C, int Wd, int H, const int* centres,
                                               int P, int ph, int pw, void* out, long ld, const short* border_labels,
                                               int db_scaled, int flags, double portion_year, const double* portion_day,
                                               int n_day, const double* time_diff, int n_td, const long long* seabed,
                                               int n_sb, const int* meta_centres, void* stream) {
  CRIMAC_REQUIRE(border_labels, "gather_patches_memm_meta: needs the label array (border rule)");
  CRIMAC_REQUIRE(flags > 0, "gather_patches_memm_meta: bad metadata arguments (flags=%d: no plane)", flags);
  const MetaPlaneSrc meta{flags, portion_year, portion_day, n_day, time_diff, n_td, seabed, n_sb};
  return gather_run("gather_patches_memm_meta", prec, GatherSrc{{data, Wd, H, border_labels}, db_scaled ? 1 : 0, meta,
                    meta_centres}, C, centres, P, ph, pw, out, ld, stream);
}

extern "C" int crimac_gather_patches_memm_labels(int prec, const float* data, int C, int Wd, int H, const int* centres,
                                                 int P, int ph, int pw, void* out, long ld, const short* patch_labels,
                                                 int db_scaled, int flags, double portion_year,
                                                 const double* portion_day, int n_day, const double* time_diff, int n_td,
                                                 const long long* seabed, int n_sb, const int* meta_centres,
                                                 void* stream) {
  CRIMAC_REQUIRE(patch_labels, "gather_patches_memm_labels: needs the transformed labels of the patches (border rule)");
  const MetaPlaneSrc meta{flags, portion_year, portion_day, n_day, time_diff, n_td, seabed, n_sb};
  return gather_run("gather_patches_memm_labels", prec, GatherSrc{{data, Wd, H}, db_scaled ? 1 : 0, meta, meta_centres}, C,
                    centres, P, ph, pw, out, ld, stream, patch_labels);
}

// The two forms for batches that span memmap echograms: border rule (by the descriptor's labels / by the TRANSFORMED
// labels of the patches, which belong to the batch, not to a source), no metadata planes, db_with_limits.
extern "C" int crimac_gather_patches_memm_multi(int prec, const crimac_memm_desc* descs, int n_desc, const int* src,
                                                int C, const int* centres, int P, int ph, int pw, void* out, long ld,
                                                void* stream) {
  CRIMAC_REQUIRE(descs, "gather_patches_memm_multi: needs the descriptor table");
  return gather_run("gather_patches_memm_multi", prec, GatherSrc{{nullptr, 0, 0, nullptr, descs, n_desc, src}}, C, centres,
                    P, ph, pw, out, ld, stream);
}

extern "C" int crimac_gather_patches_memm_labels_multi(int prec, const crimac_memm_desc* descs, int n_desc, const int* src,
                                                       int C, const int* centres, int P, int ph, int pw, void* out, long ld,
                                                       const short* patch_labels, void* stream) {
  CRIMAC_REQUIRE(descs, "gather_patches_memm_labels_multi: needs the descriptor table");
  CRIMAC_REQUIRE(patch_labels, "gather_patches_memm_labels_multi: needs the transformed labels of the patches (border rule)");
  return gather_run("gather_patches_memm_labels_multi", prec, GatherSrc{{nullptr, 0, 0, nullptr, descs, n_desc, src}}, C,
                    centres, P, ph, pw, out, ld, stream, patch_labels);
}

// crimac_gather_patches_memm_meta / _labels (patch_labels given) for batches that span memmap echograms: the metadata
// sources in a second table, parallel to the first; an echogram is its own chunk, so meta_centres are the centres.
extern "C" int crimac_gather_patches_memm_meta_multi(int prec, const crimac_memm_desc* descs,
                                                     const crimac_memm_meta_desc* metas, int n_desc, const int* src, int C,
                                                     const int* centres, int P, int ph, int pw, void* out, long ld,
                                                     const short* patch_labels, int db_scaled, int flags, void* stream) {
  CRIMAC_REQUIRE(descs && metas, "gather_patches_memm_meta_multi: needs the descriptor table and the metadata table");
  CRIMAC_REQUIRE(flags > 0, "gather_patches_memm_meta_multi: bad metadata arguments (flags=%d: no plane)", flags);
  const MetaPlaneSrc meta{flags, 0.0, nullptr, 0, nullptr, 0, nullptr, 0, metas, n_desc, src};
  return gather_run("gather_patches_memm_meta_multi", prec, GatherSrc{{nullptr, 0, 0, nullptr, descs, n_desc, src},
                    db_scaled ? 1 : 0, meta, centres}, C, centres, P, ph, pw, out, ld, stream, patch_labels);
}

extern "C" int crimac_scatter_patches_ex(const float* probs, int ncls, const int* centres, int P, int ph, int pw,
                                         int overlap, int start_ping, int n_chunk, int H, const short* labels,
                                         const unsigned char* seabed_mask, int mask_ping0, int mask_pings,
                                         const int* seabed, int seabed_ping0, int seabed_pings, const float* data0,
                                         int data_ping0, int data_pings, int seabed_pad, int seabed_rule, void* out,
                                         int out_f16, void* stream) {
  CRIMAC_REQUIRE(probs && centres && out && P > 0 && ph > 0 && pw > 0 && n_chunk > 0 && H > 0,
                 "scatter_patches: bad arguments");
  CRIMAC_REQUIRE(ncls >= 3, "scatter_patches: needs the SANDEEL (1) and OTHER (2) channels, ncls=%d", ncls);
  CRIMAC_REQUIRE(overlap >= 0 && 2 * overlap < ph && 2 * overlap < pw, "scatter_patches: bad overlap %d", overlap);
  CRIMAC_REQUIRE(seabed_rule == 0 || seabed_rule == 1, "scatter_patches: seabed_rule=%d", seabed_rule);
  CRIMAC_REQUIRE(!(seabed_mask && seabed), "scatter_patches: give the seabed mask OR the seabed vector");
  const long total = (long)P * (ph - 2 * overlap) * (pw - 2 * overlap);
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  ScatterParams q{probs, ncls, centres, P, ph, pw, overlap, start_ping, n_chunk, H, labels, seabed_mask, mask_ping0,
                  mask_pings, seabed, seabed_ping0, seabed_pings, data0, data_ping0, data_pings, seabed_pad,
                  seabed_rule, out, out_f16};
  hipLaunchKernelGGL(scatter_patches_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, q);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}

extern "C" int crimac_scatter_patches(const float* probs, int ncls, const int* centres, int P, int ph, int pw,
                                      int overlap, int start_ping, int n_chunk, int H, const short* labels,
                                      const unsigned char* seabed_mask, int mask_ping0, int mask_pings,
                                      const float* data0, int data_ping0, int data_pings, int seabed_pad,
                                      float* out, void* stream) {
  return crimac_scatter_patches_ex(probs, ncls, centres, P, ph, pw, overlap, start_ping, n_chunk, H, labels,
                                   seabed_mask, mask_ping0, mask_pings, nullptr, 0, 0, data0, data_ping0, data_pings,
                                   seabed_pad, 0, out, 0, stream);
}

extern "C" int crimac_scatter_patches_multi(const float* probs, int ncls, const crimac_memm_desc* descs, int n_desc,
                                            const int* src, const int* centres, int P, int ph, int pw, int overlap,
                                            int seabed_pad, int out_f16, void* stream) {
  CRIMAC_REQUIRE(probs && descs && src && centres && n_desc > 0 && P > 0 && ph > 0 && pw > 0,
                 "scatter_patches_multi: bad arguments");
  CRIMAC_REQUIRE(ncls >= 3, "scatter_patches_multi: needs the SANDEEL (1) and OTHER (2) channels, ncls=%d", ncls);
  CRIMAC_REQUIRE(overlap >= 0 && 2 * overlap < ph && 2 * overlap < pw, "scatter_patches_multi: bad overlap %d", overlap);
  CRIMAC_REQUIRE(P <= 65535, "scatter_patches_multi: at most 65535 patches per call");
  CRIMAC_REQUIRE((long)ph * pw < (1l << 30), "scatter_patches_multi: patch too large");
  const long per_patch = (long)(ph - 2 * overlap) * (pw - 2 * overlap);
  long bx = (per_patch + 255) / 256;
  if (bx > 64) bx = 64;
  ScatterMultiParams q{probs, ncls, descs, n_desc, src, centres, ph, pw, overlap, seabed_pad, out_f16};
  hipLaunchKernelGGL(scatter_patches_multi_kernel, dim3((unsigned)bx, (unsigned)P), dim3(256), 0, (hipStream_t)stream, q);
  CRIMAC_LAUNCH_CHECK();
  return CRIMAC_OK;
}
