/* The metadata table of the multi-source entry points of include/crimac_unet_hip.h
 * (crimac_gather_patches_memm_meta_multi, crimac_meta_planes_multi), which names the type and leaves its layout to this
 * header.  The ctypes binding (crimac_classifiers_unet_amd/hip.py) reads it with the parser it reads that header with. */
#ifndef CRIMAC_MEMM_META_H_
#define CRIMAC_MEMM_META_H_

#ifdef __cplusplus
extern "C" {
#endif

/* The metadata source of one memmap echogram: entry src[p] of a device-resident table parallel to the crimac_memm_desc
 * table.  Seven 64-bit fields, so a host writes the table as 64-bit words [n_desc][7] (the scalar through a float64 view);
 * the vectors are device addresses, of the lengths given, and are what crimac_meta_planes takes for that echogram alone. */
typedef struct crimac_memm_meta_desc {
  double portion_year;         /* portion_of_year_scalar */
  const double* portion_day;   /* portion_of_day_vector [n_day] */
  long long n_day;
  const double* time_diff;     /* time_vector_diff [n_td] */
  long long n_td;
  const long long* seabed;     /* the seabed line the depth planes go by [n_sb] */
  long long n_sb;
} crimac_memm_meta_desc;

#ifdef __cplusplus
}
#endif
#endif /* CRIMAC_MEMM_META_H_ */
