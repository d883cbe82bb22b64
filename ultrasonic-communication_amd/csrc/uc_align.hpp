// What the host side (uc_align_api.cpp) and the kernel file (uc_align_kernel.hip) of libuchirp_align.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_align_dev {

constexpr int THREADS = 256;             // 4 waves; every wave works on units of its own
constexpr int WAVE_SAMPLES = 256;        // one pass of a wave: 64 lanes x 4 consecutive samples of the reference row
constexpr int SEGMENT = 4096;            // UC_ALIGN_SEGMENT: samples of one float sum (16 passes)
constexpr int LAGS = 32;                 // lags of one unit: one accumulator each per lane
constexpr int MAX_LAG = 64;              // UC_ALIGN_MAX_LAG
// floats of the microphone row one wave stages per pass: lane l reads [4 l, 4 l + LAGS + 4) with aligned 16-byte reads
constexpr int WINDOW = WAVE_SAMPLES + LAGS + 4;   // 292

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_ALIGN_DTYPE_*

// one pair as the kernel reads it (16 bytes): wave-uniform, fetched by scalar loads
struct Pair {
  uint64_t ref;        // ref * in_stride: the reference row, in elements from in_dev
  uint64_t mic;        // mic * in_stride
};

// A unit is (pair, segment, block of LAGS lags); unit = (pair * n_segments + segment) * n_blocks + block, so that the
// units that read the same samples run next to each other.  Block b holds the lags l = 32 b - lag_pad + (0 .. 31),
// lag_pad = max_lag rounded up to a multiple of 4 (the staged window then starts on a 16-byte slot for every lane).
// Unit sums: float part[(pair * n_segments + segment) * n_blocks * 32 + (l + lag_pad)].
struct Params {
  const void* in;
  float* part;
  double* corr;
  int64_t n_in;
  int64_t first;
  int64_t n;
  uint64_t corr_stride;
  uint64_t n_units;
  uint32_t n_pairs;
  uint32_t n_segments;       // ceil(n / SEGMENT)
  uint32_t n_blocks;         // ceil((lag_pad + max_lag + 1) / LAGS)
  int32_t max_lag;
  int32_t lag_pad;
};

// workgroups of the correlation kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launches (uc_align_kernel.hip); dtype: UC_ALIGN_DTYPE_*; return the hipError_t of the launch as int
int launch_correlate(int dtype, unsigned grid, void* stream, const Params& p, const Pair* pairs);
int launch_sum(void* stream, const Params& p);

}  // namespace uc_align_dev
