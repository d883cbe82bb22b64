// What the host side (uc_wcorr_api.cpp) and the kernel file (uc_wcorr_kernel.hip) of libuchirp_wcorr.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_wcorr_dev {

constexpr int THREADS = 128;             // 2 waves: one 2048-point transform per workgroup (uc_xform.hpp)
constexpr int POINTS = 2048;             // UC_WCORR_POINTS
constexpr int GROUP = 4;                 // UC_WCORR_GROUP: segments of one unit
constexpr int MAX_LAG = 512;             // UC_WCORR_MAX_LAG: the bound on max_lag + guard
constexpr int BINS = POINTS / 2 + 1;     // UC_WCORR_BINS: the weights of bins 0 .. 1024
constexpr int SUM_THREADS = 256;

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_WCORR_DTYPE_*

// one pair as the kernel reads it (16 bytes): workgroup-uniform, fetched by scalar loads
struct Pair {
  uint64_t ref;        // ref * in_stride: the reference row, in elements from in_dev
  uint64_t mic;        // mic * in_stride
};

// A unit is (pair, window, group of GROUP segments); unit = (pair * n_windows + window) * n_groups + group, so that units
// which read the same samples are neighbours.  Unit sums: float part[unit * (2 max_lag + 1) + (l + max_lag)].
struct Params {
  const void* in;
  const float* tw;           // exp(-2 pi i k / 2048), k < 2048, (re, im)
  const float* weights;      // w[k], k < BINS (staged behind the pairs)
  float* part;
  double* corr;
  int64_t n_in;
  int64_t first;
  int64_t window_len;
  int64_t hop;
  uint64_t corr_stride;
  uint64_t n_units;          // n_pairs * n_windows * n_groups
  uint32_t n_pairs;
  uint32_t n_windows;
  uint32_t n_segments;       // of one window: ceil(window_len / (POINTS - 2 (max_lag + guard)))
  uint32_t n_groups;         // of one window: ceil(n_segments / GROUP)
  int32_t max_lag;           // L: 2 L + 1 sums of a unit are stored
  int32_t guard;             // L' = L + guard: the segments are those of the wide-lag correlator at L'
};

// workgroups of the correlation kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launches (uc_wcorr_kernel.hip); dtype: UC_WCORR_DTYPE_*; return the hipError_t of the launch as int
int launch_correlate(int dtype, unsigned grid, void* stream, const Params& p, const Pair* pairs);
int launch_sum(void* stream, const Params& p);

}  // namespace uc_wcorr_dev
