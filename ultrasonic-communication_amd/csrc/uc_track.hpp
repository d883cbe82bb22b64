// What the host side (uc_track_api.cpp) and the kernel file (uc_track_kernel.hip) of libuchirp_track.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_track_dev {

constexpr int THREADS = 128;             // 2 waves: one 2048-point transform per workgroup (uc_xform.hpp)
constexpr int POINTS = 2048;             // UC_TRACK_POINTS
constexpr int GROUP = 4;                 // UC_TRACK_GROUP: segments of one unit
constexpr int MAX_LAG = 512;             // UC_TRACK_MAX_LAG
constexpr int SLOTS = 4;                 // UC_TRACK_SLOTS
constexpr int CREST_THREADS = 64;        // one wave per (pair, window)

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_TRACK_DTYPE_*
constexpr uint32_t NO_PEAK = 1, AT_EDGE = 2, NOT_FINITE = 4;   // UC_TRACK_* flags

// one pair as the kernel reads it (16 bytes): workgroup-uniform, fetched by scalar loads
struct Pair {
  uint64_t ref;        // ref * in_stride: the reference row, in elements from in_dev
  uint64_t mic;        // mic * in_stride
};

// struct uc_track_slot / uc_track_crest as the device writes them
struct Slot {
  int32_t k;
  int32_t reserved;
  double r[3];
};
struct Crest {
  uint32_t flags;
  uint32_t n_candidates;
  Slot slot[SLOTS];
};

// A unit is (pair, window, group of GROUP segments); unit = (pair * n_windows + window) * n_groups + group, so that units
// which read the same samples are neighbours.  Unit sums: float part[unit * (2 max_lag + 1) + (l + max_lag)].
struct Params {
  const void* in;
  const float* tw;           // exp(-2 pi i k / 2048), k < 2048, (re, im)
  float* part;
  double* corr;              // or nullptr
  Crest* crest;              // or nullptr
  int64_t n_in;
  int64_t first;
  int64_t window_len;
  int64_t hop;
  uint64_t corr_stride;
  uint64_t n_units;          // n_pairs * n_windows * n_groups
  uint32_t n_pairs;
  uint32_t n_windows;
  uint32_t n_segments;       // of one window: ceil(window_len / (POINTS - 2 max_lag))
  uint32_t n_groups;         // of one window: ceil(n_segments / GROUP)
  int32_t max_lag;
  uint32_t from_corr;        // (UC_TUNING only) the crest kernel reads corr instead of the unit sums
};

// workgroups of the correlation kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launches (uc_track_kernel.hip); dtype: UC_TRACK_DTYPE_*; return the hipError_t of the launch as int
int launch_correlate(int dtype, unsigned grid, void* stream, const Params& p, const Pair* pairs);
int launch_crest(void* stream, const Params& p);

}  // namespace uc_track_dev
