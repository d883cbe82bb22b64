// What the host side (uc_duc_api.cpp) and the kernel file (uc_duc_kernel.hip) of libuchirp_duc.so share: how a raw input word
// becomes a float, the carrier of a phase, one step of the polyphase chain, the mixer, the sum over channels and the int16
// output stage of include/uchirp_duc.h, written once and compiled for both, so that uc_duc_filter_row and uc_duc_sum_row (the
// definition in plain C) and the kernel cannot drift apart; and the geometry of the kernel's units of work, which the host
// needs for the launch.
//
// The carrier is the down-converter's (csrc/uc_ddc.hpp), restated: the two libraries share no text, and
// tests/test_duc_cpu.py holds their tables equal to the bit.  Every operation of the carrier, the mixer and the sum is one
// correctly rounded float32 multiply, add or subtract; a chain is one fused multiply-add per tap.  The device flags contract
// by default, so everything below stands under a contraction-off pragma of this file's own; nothing here may be compiled
// with flags that flush denormals or relax the arithmetic.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIP__
#define UC_DUC_HD __host__ __device__ __forceinline__
#else
#define UC_DUC_HD inline
#endif

#pragma clang fp contract(off)

namespace uc_duc_dev {

constexpr int THREADS = 256;             // a workgroup: four waves; a lane is every 256th output of a span
constexpr int MAX_PHASE_TAPS = 128;      // K: taps per phase
constexpr int MAX_INTERP = 64;           // L
constexpr int MAX_TAPS = 2048;           // K L: the prototype
constexpr int MAX_SETS = 256;
constexpr int MAX_CHAN = 16;
constexpr int STATE_SAMPLES = 128;       // an input row's state in the caller's memory: the samples in front of `first`
constexpr int TABLE = 1024;              // (cos, sin) pairs of the coarse and of the fine table
constexpr int TILE_OUT = 2048;           // the outputs of a span, at most
constexpr int MAX_PER_LANE = TILE_OUT / THREADS;   // outputs of one lane in a span: 8

constexpr int IN_IQ = 0, IN_I = 1;       // UC_DUC_IN_*
constexpr int OUT_F32 = 0, OUT_I16 = 1;  // UC_DUC_OUT_*

// A span: the outputs of one unit of work, (2048 div L) L of them, so that a span starts on phase 0 of an input sample.
constexpr uint32_t span_inputs(uint32_t interp) { return TILE_OUT / interp; }
constexpr uint32_t span_outputs(uint32_t interp) { return span_inputs(interp) * interp; }
// One LDS pool holds a channel's staged samples and its tap set behind them: span_inputs + K samples (K - 1 of history and
// one more, which the lanes without an output reach) of 2 floats at most, then K L taps.  K <= 128 and K L <= 2048, so the
// largest is L = 1, K = 128: 2 (2048 + 128) + 128 floats.
constexpr uint32_t pool_floats(uint32_t interp, uint32_t k_taps) { return 2 * (span_inputs(interp) + k_taps) + k_taps * interp; }
constexpr int POOL_FLOATS = 2 * (TILE_OUT + MAX_PHASE_TAPS) + MAX_PHASE_TAPS;
// o / L for o < 2^12 as (o * recip) >> 20: recip = ceil(2^20 / L) errs by less than L / 2^20 per unit of o
constexpr uint32_t span_recip(uint32_t interp) { return ((1u << 20) + interp - 1) / interp; }

UC_DUC_HD float bits_to_float(uint32_t raw) {
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(raw);
#else
  float f;
  memcpy(&f, &raw, sizeof(f));
  return f;
#endif
}

// an input float as it is (denormals too); NaN and the infinities read as +0
UC_DUC_HD float sample_of(uint32_t raw) { return (raw & 0x7F800000u) == 0x7F800000u ? 0.0f : bits_to_float(raw); }

// the phase of the OUTPUT with absolute index n (its low 32 bits are all that counts)
UC_DUC_HD uint32_t phase_of(uint32_t phase0, uint32_t step, uint64_t n) { return phase0 + step * (uint32_t)n; }

// (cos, sin) of a phase from the two tables' entries: (cc, sc) = coarse[phase >> 22], (cf, sf) = fine[(phase >> 12) & 1023]
UC_DUC_HD void carrier(float cc, float sc, float cf, float sf, float* c, float* s) {
  const float a = cc * cf, b = sc * sf, d = sc * cf, e = cc * sf;
  *c = a - b;
  *s = d + e;
}

// one step of a chain
UC_DUC_HD float chain(float h, float z, float acc) { return __builtin_fmaf(h, z, acc); }

// the mixer: I cos + Q sin, two rounded products and one rounded sum; I alone: one product
UC_DUC_HD float mix_iq(float ai, float aq, float c, float s) {
  const float a = ai * c, b = aq * s;
  return a + b;
}
UC_DUC_HD float mix_i(float ai, float c) { return ai * c; }

// one step of the sum over channels
UC_DUC_HD float add_channel(float sum, float y) { return sum + y; }

// UC_DUC_OUT_I16: rintf (ties to even), clamped to -32768 .. 32767; NaN gives 0.  *clipped: the rounded value lay outside
// int16, or y was NaN.
UC_DUC_HD int16_t to_i16(float y, bool* clipped) {
  if (y != y) {
    *clipped = true;
    return 0;
  }
  const float r = __builtin_rintf(y);
  if (r > 32767.0f) {
    *clipped = true;
    return 32767;
  }
  if (r < -32768.0f) {
    *clipped = true;
    return -32768;
  }
  *clipped = false;
  return (int16_t)(int32_t)r;
}

// channel j of output row r, record r n_chan + j: what row_map, set_index, step and phase0 say of it
struct Channel {
  uint32_t row, set, step, phase0;
};

struct Params {
  const uint32_t* in;        // n_in_rows rows of floats: pairs for UC_DUC_IN_IQ
  void* out;                 // n_rows rows of floats or of int16
  float* state;              // n_in_rows x 128 samples
  uint32_t* clip;            // n_rows counts, or NULL
  const float* taps;         // n_sets x K L, in the object's memory
  const float* tables;       // coarse (2048 floats), fine (2048 floats), in the object's memory
  const Channel* chan;       // n_rows x n_chan records, or NULL: channel j of row r reads input row r n_chan + j, set 0, step 0, phase 0
  uint64_t in_stride;        // floats
  uint64_t out_stride;       // elements
  uint64_t n_samples;
  uint64_t first_out;        // the absolute index of the call's first output: first * L
  uint64_t count;            // outputs of a row: n_samples * L
  uint64_t spans;            // ceil(count / span)
  uint64_t units;            // n_rows * spans
  uint32_t n_in_rows;
  uint32_t n_chan;
  uint32_t k_taps;           // K
  uint32_t interp;           // L
  uint32_t span;             // span_outputs(L)
  uint32_t span_in;          // span_inputs(L)
  uint32_t recip;            // span_recip(L)
  uint32_t in_vec;           // 1: every input row starts on 8 bytes (8-byte loads of I, Q pairs)
};

// launches (uc_duc_kernel.hip); formats: UC_DUC_IN_*, UC_DUC_OUT_*; they return the hipError_t of the launch as int
int launch_convert(int in_format, int out_format, unsigned grid, void* stream, const Params& p);
int launch_state(int in_format, unsigned grid, void* stream, const Params& p);

}  // namespace uc_duc_dev
