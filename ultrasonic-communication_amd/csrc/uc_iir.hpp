// What the host side (uc_iir_api.cpp) and the kernel file (uc_iir_kernel.hip) of libuchirp_iir.so share: how a raw input
// word becomes a float and the one sample of a biquad cascade of include/uchirp_iir.h, written once and compiled for both, so
// that uc_iir_filter_row (the definition in plain C for one row) and the kernel cannot drift apart.
//
// Every operation of the recurrence is one correctly rounded float32 multiply, add or subtract.  The device flags contract
// by default, so everything below stands under a contraction-off pragma of this file's own; nothing here may be compiled
// with flags that flush denormals or relax the arithmetic.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIP__
#define UC_IIR_HD __host__ __device__ __forceinline__
#else
#define UC_IIR_HD inline
#endif

namespace uc_iir_dev {

constexpr int LANES = 64;                // one wave per workgroup; a lane is one output row
constexpr int GROUP = 4;                 // samples of one 16-byte access
constexpr int MAX_SECTIONS = 8;
constexpr int MAX_SETS = 256;
constexpr int COEFS = 5;                 // b0 b1 b2 a1 a2 of a section (a0 = 1)
constexpr int STATE_WORDS = 2 * MAX_SECTIONS;   // z1, z2 of sections 0 .. 7: a row's state in the caller's memory

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_IIR_DTYPE_*

UC_IIR_HD float bits_to_float(uint32_t raw) {
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(raw);
#else
  float f;
  memcpy(&f, &raw, sizeof(f));
  return f;
#endif
}

UC_IIR_HD uint32_t float_to_bits(float f) {
#ifdef __HIP_DEVICE_COMPILE__
  return __float_as_uint(f);
#else
  uint32_t raw;
  memcpy(&raw, &f, sizeof(raw));
  return raw;
#endif
}

// UC_IIR_DTYPE_F32: the float as it is (denormals too); NaN and the infinities read as +0.
// UC_IIR_DTYPE_I32: the 24-bit value of a DFSDM word, (float)(word >> 8): exact.
template <int DT>
UC_IIR_HD float sample_of(uint32_t raw) {
  if (DT == DT_F32) return (raw & 0x7F800000u) == 0x7F800000u ? 0.0f : bits_to_float(raw);
  return (float)((int32_t)raw >> 8);
}

// One sample through NS sections; c: NS x {b0 b1 b2 a1 a2}, z: NS x {z1, z2}.  Returns the last section's output.
template <int NS>
UC_IIR_HD float filter_sample(const float* c, float* z, float u) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float b0 = c[COEFS * s], b1 = c[COEFS * s + 1], b2 = c[COEFS * s + 2], a1 = c[COEFS * s + 3], a2 = c[COEFS * s + 4];
    const float o = (b0 * u) + z[2 * s];
    z[2 * s] = ((b1 * u) - (a1 * o)) + z[2 * s + 1];
    z[2 * s + 1] = (b2 * u) - (a2 * o);
    u = o;
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(u));          // sections in the order written: the scheduler would interleave samples and run out of registers
#endif
  }
  return u;
}

struct Params {
  const void* in;
  float* out;
  float* state;              // n_rows x 16: {z1, z2} of sections 0 .. 7; the words of sections 0 .. n_sections - 1 are read and written
  const float* sections;     // n_sets x n_sections x 5, in the object's memory
  const uint32_t* row_map;   // n_rows input rows, or NULL: row r reads input row r
  const uint32_t* set_index; // n_rows sets, or NULL: set 0
  uint64_t in_stride;        // elements
  uint64_t out_stride;
  uint64_t n_samples;
  uint32_t n_rows;
  uint32_t row_blocks;       // ceil(n_rows / LANES)
  uint32_t in_vec;           // 1: every row of the input starts on 16 bytes (pointer and stride allow b128 loads)
  uint32_t out_vec;          // 1: the same of the output
};

// launch (uc_iir_kernel.hip); dtype: UC_IIR_DTYPE_*; n_sections 1 .. 8; returns the hipError_t of the launch as int
int launch_filter(int dtype, int n_sections, unsigned grid, void* stream, const Params& p);

}  // namespace uc_iir_dev
