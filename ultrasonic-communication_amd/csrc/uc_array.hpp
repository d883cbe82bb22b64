// What the host side (uc_array_api.cpp) and the kernel file (uc_array_kernel.hip) of libuchirp_array.so share.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_array_dev {

constexpr int THREADS = 256;             // 4 waves
constexpr int WAVE_SAMPLES = 256;        // one wave: 64 lanes x 4 consecutive outputs of one beam
constexpr int TILE_SAMPLES = 1024;       // one workgroup pass: 4 waves
constexpr int COEFS = 16;
constexpr int WINDOW = WAVE_SAMPLES + COEFS;   // floats of input one wave stages per tap (271 are read)
constexpr uint32_t MAX_TAPS = 32;

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_ARRAY_DTYPE_*

// one tap as the kernel reads it (80 bytes): wave-uniform, fetched by scalar loads; the coefficients stay in scalar
// registers and feed the multiply-adds as scalar operands
struct Tap {
  int64_t shift;       // floor(delay) - 7
  uint64_t row;        // mic * in_stride: the microphone's row, in elements from in_dev
  float c[COEFS];
};

// one beam (8 bytes; the layout of uc_array_beam)
struct Beam {
  uint32_t first_tap;
  uint32_t n_taps;
};

struct Params {
  const void* in;
  float* out;
  int64_t in_first;          // absolute sample of element 0 of every input row
  int64_t n_in;
  int64_t out_first;
  int64_t n_out;
  uint64_t out_stride;
  uint32_t tiles_per_beam;   // ceil(n_out / TILE_SAMPLES)
  uint32_t n_beams;
};

// workgroups of the kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launch (uc_array_kernel.hip); dtype: UC_ARRAY_DTYPE_*; returns the hipError_t of the launch as int
int launch_combine(int dtype, unsigned grid, void* stream, const Params& p, const Beam* beams, const Tap* taps);

}  // namespace uc_array_dev
