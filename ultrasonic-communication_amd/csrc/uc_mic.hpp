// What the host side (uc_mic_api.cpp) and the kernel file (uc_mic_kernel.hip) of libuchirp_mic.so share: the quantiser and the
// one sample of 32 bit-steps of include/uchirp_mic.h, written once and compiled for both, so that uc_mic_modulate_row (the
// definition in plain C for one row) and the kernel cannot drift apart.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIP__
#define UC_MIC_HD __host__ __device__ __forceinline__
#else
#define UC_MIC_HD inline
#endif

namespace uc_mic_dev {

constexpr int LANES = 64;                // one wave per workgroup; a lane is one row (one microphone)
constexpr int GROUP = 4;                 // samples of one 16-byte access

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_MIC_DTYPE_*

constexpr int32_t Q_MAX = (1 << 23) - 1; // |q| of a quantised sample, at most
constexpr uint32_t Y = 1u << 25;         // the quantiser's feedback: full scale of the loop

// the carried state of a row, in registers
struct State {
  uint32_t prev, s1, s2;                 // int32 in two's complement; unsigned here so that every sum wraps
};

// UC_MIC_DTYPE_F32: one multiply, to nearest even, clamped; NaN reads as 0.  (The clamp comes first: its bounds are whole
// numbers, so rounding what is clamped equals clamping what is rounded, and the cast never sees a value it cannot hold.)
UC_MIC_HD int32_t quantise_f32(float x, float scale) {
  float v = x * scale;
  v = v != v ? 0.0f : v;
  v = v > (float)Q_MAX ? (float)Q_MAX : v;
  v = v < -(float)Q_MAX ? -(float)Q_MAX : v;
  return (int32_t)__builtin_rintf(v);
}

// UC_MIC_DTYPE_I32: the 24-bit value of a DFSDM word; only -2^23 is out of range
UC_MIC_HD int32_t quantise_i32(int32_t word) {
  const int32_t q = word >> 8;
  return q < -Q_MAX ? -Q_MAX : q;
}

// One input sample: 32 bit-steps, the output word.  `ramp` is d (b + 1) as a running sum; its >> is arithmetic.  The
// quantiser without a comparison: below = 1 where s2 < 0, -y = (below << 26) - Y is +Y there and -Y elsewhere, and the
// word collects `below` from the top down, so that after 32 steps bit b is step b's and the word is the complement of the
// bits wanted.  On the device that is nine full-rate integer instructions per bit and no condition code.
UC_MIC_HD uint32_t modulate_sample(State& s, int32_t q) {
  const uint32_t d = (uint32_t)q - s.prev;
  const uint32_t base = 2u * s.prev;
  uint32_t ramp = 0, s1 = s.s1, s2 = s.s2, word = 0;
#pragma unroll
  for (int b = 0; b < 32; ++b) {
    ramp += d;
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(ramp));       // a sum, not d * (b + 1): the 32-bit multiply runs at a quarter of the rate
#endif
    const uint32_t u = base + (uint32_t)((int32_t)ramp >> 4);
    uint32_t below = s2 >> 31;
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(below));      // one shift serves -y (a shift-add) and the word (an align-bit), not a mask for each
#endif
    const uint32_t minus_y = (below << 26) - Y;
    s1 += u + minus_y;
    s2 += s1 + minus_y;
    word = (word >> 1) | (below << 31);
  }
  s.prev = (uint32_t)q;
  s.s1 = s1;
  s.s2 = s2;
  return ~word;
}

struct Params {
  const void* in;
  uint32_t* out;
  int32_t* state;            // n_rows x 4: {prev, s1, s2, 0}
  uint64_t in_stride;        // elements
  uint64_t out_stride;
  uint64_t n_samples;
  uint32_t n_rows;
  uint32_t row_blocks;       // ceil(n_rows / LANES)
  float scale;
  uint32_t in_vec;           // 1: every row of the input starts on 16 bytes (pointer and stride allow b128 loads)
  uint32_t out_vec;          // 1: the same of the output
};

// launch (uc_mic_kernel.hip); dtype: UC_MIC_DTYPE_*; returns the hipError_t of the launch as int
int launch_modulate(int dtype, unsigned grid, void* stream, const Params& p);

}  // namespace uc_mic_dev
