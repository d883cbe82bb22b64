// What the host side (uc_xcorr_api.cpp) and the kernel file (uc_xcorr_kernel.hip) of libuchirp_xcorr.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_xcorr_dev {

constexpr int THREADS = 128;             // 2 waves: one 2048-point transform per workgroup (uc_xform.hpp)
constexpr int POINTS = 2048;             // UC_XCORR_POINTS
constexpr int GROUP = 4;                 // UC_XCORR_GROUP: segments of one unit
constexpr int MAX_LAG = 512;             // UC_XCORR_MAX_LAG
constexpr int SUM_THREADS = 256;

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_XCORR_DTYPE_*

// one pair as the kernel reads it (16 bytes): workgroup-uniform, fetched by scalar loads
struct Pair {
  uint64_t ref;        // ref * in_stride: the reference row, in elements from in_dev
  uint64_t mic;        // mic * in_stride
};

// A unit is (pair, group of GROUP segments); unit = pair * n_groups + group.
// Unit sums: float part[unit * (2 max_lag + 1) + (l + max_lag)].
struct Params {
  const void* in;
  const float* tw;           // exp(-2 pi i k / 2048), k < 2048, (re, im)
  float* part;
  double* corr;
  int64_t n_in;
  int64_t first;
  int64_t n;
  uint64_t corr_stride;
  uint64_t n_units;          // n_pairs * n_groups
  uint32_t n_pairs;
  uint32_t n_segments;       // ceil(n / (POINTS - 2 max_lag))
  uint32_t n_groups;         // ceil(n_segments / GROUP)
  int32_t max_lag;
};

// workgroups of the correlation kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launches (uc_xcorr_kernel.hip); dtype: UC_XCORR_DTYPE_*; return the hipError_t of the launch as int
int launch_correlate(int dtype, unsigned grid, void* stream, const Params& p, const Pair* pairs);
int launch_sum(void* stream, const Params& p);

}  // namespace uc_xcorr_dev
