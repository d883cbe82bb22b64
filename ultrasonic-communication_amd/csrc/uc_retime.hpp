// What the host side (uc_retime_api.cpp) and the kernel file (uc_retime_kernel.hip) of libuchirp_retime.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_retime_dev {

constexpr int THREADS = 256;             // 4 waves
constexpr int WAVE_SAMPLES = 256;        // one wave: 64 lanes x 4 consecutive outputs of one row
constexpr int TILE_SAMPLES = 1024;       // one workgroup pass: 4 waves
constexpr int COEFS = 16;
constexpr int TABLE_ROWS = 257;          // fractions 0, 1/256 .. 255/256, 1
constexpr int WINDOW = WAVE_SAMPLES + COEFS;   // floats of input one wave stages: 256 + 15 + 1 (I - j may step by one in a wave)

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_RETIME_DTYPE_*

// one line as the kernel reads it (24 bytes): wave-uniform, fetched by scalar loads
struct Line {
  int64_t lead_fx;     // llrint(delay_samples * 2^32)
  int64_t drift_fx;    // llrint(slope * 2^32), |drift_fx| <= 2^23
  uint64_t row;        // mic * in_stride: the microphone's row, in elements from in_dev
};

struct Params {
  const void* in;
  float* out;
  const float* table;        // T[257][16] in device memory, 16-byte aligned
  int64_t in_first;          // absolute sample of element 0 of every input row
  int64_t n_in;
  int64_t out_first;
  int64_t n_out;
  uint64_t out_stride;
  uint32_t tiles_per_row;    // ceil(n_out / TILE_SAMPLES)
  uint32_t n_lines;
};

// workgroups of the kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launch (uc_retime_kernel.hip); dtype: UC_RETIME_DTYPE_*; returns the hipError_t of the launch as int
int launch_rows(int dtype, unsigned grid, void* stream, const Params& p, const Line* lines);

}  // namespace uc_retime_dev
