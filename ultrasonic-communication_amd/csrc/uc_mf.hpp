// What the host side (uc_mf_api.cpp) and the kernel file (uc_mf_kernel.hip) of libuchirp_mf.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_mf_dev {

constexpr int THREADS = 128;             // 2 waves: one 2048-point transform per workgroup (uc_xform.hpp)
constexpr int POINTS = 2048;             // UC_MF_POINTS
constexpr int MAX_TAPS = 1664;           // UC_MF_MAX_TAPS
constexpr int CANDIDATES = 4;            // UC_MF_CANDIDATES
constexpr int RECORD_WORDS = 20;         // sizeof(uc_mf_record) / 4

constexpr int DT_I32 = 0, DT_F32 = 1, DT_C32 = 2;                    // UC_MF_DTYPE_*
constexpr int OUT_COMPLEX = 0, OUT_REAL = 1, OUT_POWER = 2, OUT_MAG = 3;   // UC_MF_OUT_*

// one job as the kernel reads it (16 bytes): workgroup-uniform, fetched by scalar loads
struct Job {
  uint64_t row;        // row * in_stride: the row, in elements from in_dev
  uint32_t set;
  uint32_t pad;
};

// A unit is (job, segment of the call); unit = job * n_segments + segment.  Workgroup b does the units
// b * chunk .. min(n_units, (b + 1) * chunk) - 1: runs of consecutive segments of one job.
struct Params {
  const void* in;
  const float* tw;           // exp(-2 pi i k / 2048), k < 2048, (re, im)
  const float* spectra;      // [n_sets][2048] (re, im): H of the definition
  void* out;                 // or nullptr
  uint32_t* records;         // or nullptr: [n_jobs][n_segments][RECORD_WORDS]
  int64_t n_in;              // elements of a row
  int64_t base0;             // row element of output 0 of the call's first segment: first_segment * S - pos0 (may be negative)
  int64_t first;
  int64_t n;
  uint64_t out_stride;
  uint64_t n_units;          // n_jobs * n_segments
  uint64_t chunk;            // units of one workgroup
  uint32_t n_segments;
  int32_t taps;              // T
  int32_t format;            // OUT_*
};

// workgroups of the kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launch (uc_mf_kernel.hip); dtype: UC_MF_DTYPE_*; returns the hipError_t of the launch as int
int launch_run(int dtype, unsigned grid, void* stream, const Params& p, const Job* jobs);

}  // namespace uc_mf_dev
