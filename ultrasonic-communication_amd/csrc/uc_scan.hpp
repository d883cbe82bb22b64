// What the host side (uc_scan_api.cpp) and the kernel file (uc_scan_kernel.hip) of libuchirp_scan.so share: how a raw input
// word becomes a float, one tap's chain of one product and fifteen fused multiply-adds, and the square-and-add of a chain of
// include/uchirp_scan.h, written once and compiled for both, so that uc_scan_power_row (the definition in plain C for one
// beam and one window) and the kernel cannot drift apart.
//
// The fused multiply-adds are the explicit ones of the definition; nothing else may fuse.  The device flags contract by
// default, so everything below (and every file that includes this one) stands under a contraction-off pragma.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#pragma clang fp contract(off)

#ifdef __HIP__
#define UC_SCAN_HD __host__ __device__ __forceinline__
#else
#define UC_SCAN_HD inline
#endif

namespace uc_scan_dev {

constexpr int THREADS = 256;             // 4 waves
constexpr int WAVES = THREADS / 64;
constexpr int STEP = 256;                // samples of one wave step: 64 lanes x 4 consecutive samples = the 64 chains
constexpr int SEGMENT = 4096;            // samples of one float32 partial sum: 16 steps
constexpr int COEFS = 16;
constexpr int FRACTIONS = 256;
constexpr int MAX_TAPS = 32;
constexpr int BEAMS_PER_WAVE = 4;        // beams a wave carries through a window side by side
constexpr int GROUP = WAVES * BEAMS_PER_WAVE;   // beams of one work unit: they share every staged image
constexpr int SPREAD = 64;               // shifts of a tap that the staged image serves: lo_k .. lo_k + SPREAD
constexpr int IMAGE = STEP + SPREAD + 24;       // floats of one tap's image: 86 aligned quads (a lane reads 6 of them)
constexpr int SMALL_TAPS = 8;            // the kernel is built twice: LDS for 8 taps and for 32

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_SCAN_DTYPE_*

UC_SCAN_HD float bits_to_float(uint32_t raw) {
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(raw);
#else
  float f;
  memcpy(&f, &raw, sizeof(f));
  return f;
#endif
}

// UC_SCAN_DTYPE_F32: the float as it is.  UC_SCAN_DTYPE_I32: (float) of the word, as the array combiner casts it.
template <int DT>
UC_SCAN_HD float sample_of(uint32_t raw) {
  return DT == DT_F32 ? bits_to_float(raw) : (float)(int32_t)raw;
}

// one tap of one beam sample: c[0] * x[0], then fmaf(c[t], x[t], .) for t = 1 .. 15
UC_SCAN_HD float tap_sample(const float* c, const float* x) {
  float a = c[0] * x[0];
#pragma unroll
  for (int t = 1; t < COEFS; ++t) a = __builtin_fmaf(c[t], x[t], a);
  return a;
}

// one sample into its chain: the square rounded once, the sum rounded once
UC_SCAN_HD float chain_add(float chain, float y) {
  const float s = y * y;
  return chain + s;
}

struct Params {
  const void* in;
  double* power;             // the caller's, or the object's scratch
  const int32_t* q;          // n_beams x n_taps quantised delays
  const float* table;        // n_taps x 256 x 16 coefficients
  const uint8_t* direct;     // n_beams: 1 where a shift of the beam lies outside the staged image
  int64_t in_first;          // absolute sample of element 0 of every input row
  int64_t n_in;
  int64_t first;             // absolute sample of window 0
  int64_t window_len;
  int64_t hop;
  uint64_t in_stride;        // elements
  uint64_t power_stride;     // doubles
  uint64_t array_rows;
  uint32_t n_taps;
  uint32_t n_beams;
  uint32_t n_windows;
  uint32_t n_arrays;
  uint32_t beam_groups;      // ceil(n_beams / GROUP)
  uint32_t mic[MAX_TAPS];    // tap k's row within an array
  int32_t lo[MAX_TAPS];      // the lowest shift of tap k that the staged image serves
};

// one best record as the kernel writes it (the layout of uc_scan_best)
struct Best {
  uint32_t beam;
  uint32_t flags;
  double power;
};

// variant: dtype | (n_taps > SMALL_TAPS ? 2 : 0).  Workgroups of that build one CU holds at once (<= 0: unknown)
int resident_blocks_per_cu(int variant);

// launches (uc_scan_kernel.hip); each returns the hipError_t of the launch as int
int launch_power(int dtype, unsigned grid, void* stream, const Params& p);
int launch_best(unsigned grid, void* stream, const double* power, uint64_t power_stride, uint32_t n_beams, uint32_t rows, Best* best);

}  // namespace uc_scan_dev
