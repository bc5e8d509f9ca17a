// Per-pixel metadata planes of a crop (reference batch/dataset.py:288-351, get_crop_memmap), shared by
// crimac_meta_planes (meta.hip: [P][Cm][H][W] planes for UNet_LateMetInject) and crimac_gather_patches_memm_meta
// (tiling.hip: the planes as extra INPUT channels of the gathered NHWC crop) so that the two cannot drift apart -- and by
// their _multi forms, which take the scalar and the vectors of patch p from a table (MetaPlaneSrc::resolve).
//
// Seven planes at most, every one a function of the crop centre and of three per-ping vectors of the echogram:
//   portion_year      : the echogram's scalar
//   portion_day (x2)  : sin / cos of 2 pi * portion_of_day_vector[centre ping]           (index clamped: < 0 -> 0, >= n -> last)
//   time_diff         : time_vector_diff[ping of the column]                             (same clamping, per column)
//   depth_rel         : row / seabed[ping]         depth_abs_surface : row / H         depth_abs_seabed : (seabed[ping] - row) / H
// with row = cy - H/2 + y, ping = cx - W/2 + x -- the reference's arange(c - w // 2, c + w // 2), one pixel up / left of the
// DATA crop's grid (getGrid: c - (w + 1) // 2 + 1 ...): reproduced, not "fixed".  The reference computes in float64 and the
// batch is cast to float32 by SegPipe.predict_batch (.float()): the same here (double arithmetic, one rounding).
#pragma once
#include "../../include/crimac_memm_meta.h"

constexpr int CRIMAC_MAX_META_PLANES = 7;

struct MetaPlaneSrc {
  int flags;                     // bit 0 portion_year, 1 portion_day, 2 time_diff, 3 depth_rel, 4 depth_abs_surface, 5 depth_abs_seabed
  double portion_year;
  const double* portion_day; int n_day;
  const double* time_diff; int n_td;
  const long long* seabed; int n_sb;
  // metas != NULL (batches that span memmap echograms): src[p] picks patch p's crimac_memm_meta_desc from a device-resident
  // table -- the one PatchSrc's src indexes (tiling.hip) -- and the scalar and the three vectors are that echogram's.
  const crimac_memm_meta_desc* metas; int n_desc; const int* src;
  // false: patch p has no source -- src[p] names no descriptor, or the descriptor lacks a vector the flags need -- and is
  // skipped, nothing of it is read.  The scalar form (metas == NULL) was checked by the host.
  __device__ __forceinline__ bool resolve(int p) {
    if (!metas) return true;
    const int i = src[p];
    if (i < 0 || i >= n_desc) return false;
    const crimac_memm_meta_desc d = metas[(long)i];
    portion_year = d.portion_year;
    portion_day = d.portion_day; n_day = meta_len(d.n_day);
    time_diff = d.time_diff; n_td = meta_len(d.n_td);
    seabed = d.seabed; n_sb = meta_len(d.n_sb);
    return (!(flags & 2) || (portion_day && n_day > 0)) && (!(flags & 4) || (time_diff && n_td > 0)) &&
           (!(flags & 56) || (seabed && n_sb > 0));
  }
  __device__ __forceinline__ static int meta_len(long long n) { return n > 2147483647ll ? 2147483647 : (int)n; }
};
static_assert(sizeof(crimac_memm_meta_desc) == 56, "crimac_memm_meta_desc: seven 64-bit fields (hip.MEMM_META_WORDS)");

__host__ __device__ inline int meta_plane_count(int flags) {
  return (flags & 1) + 2 * ((flags >> 1) & 1) + ((flags >> 2) & 1) + ((flags >> 3) & 1) + ((flags >> 4) & 1) +
         ((flags >> 5) & 1);
}

__device__ __forceinline__ int meta_clamp_last(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// Pixel (y, x) of the H x W crop centred on (cy, cx) (range idx, global ping idx): its planes, in flag order, into o[].
__device__ __forceinline__ void meta_plane_values(const MetaPlaneSrc& s, int cy, int cx, int H, int W, int y, int x,
                                                  float (&o)[CRIMAC_MAX_META_PLANES]) {
  const int row = cy - H / 2 + y, ping = cx - W / 2 + x;
  int c = 0;
  if (s.flags & 1) { o[c] = (float)s.portion_year; ++c; }
  if (s.flags & 2) {
    const double t = s.portion_day[meta_clamp_last(cx, s.n_day)];
    o[c] = (float)sin(2.0 * 3.141592653589793 * t); ++c;
    o[c] = (float)cos(2.0 * 3.141592653589793 * t); ++c;
  }
  if (s.flags & 4) { o[c] = (float)s.time_diff[meta_clamp_last(ping, s.n_td)]; ++c; }
  if (s.flags & 56) {
    const double sb = (double)s.seabed[meta_clamp_last(ping, s.n_sb)];
    if (s.flags & 8) { o[c] = (float)((double)row / sb); ++c; }
    if (s.flags & 16) { o[c] = (float)((double)row / (double)H); ++c; }
    if (s.flags & 32) { o[c] = (float)((sb - (double)row) / (double)H); ++c; }
  }
}
