// What the host side (uc_ddc_api.cpp) and the kernel file (uc_ddc_kernel.hip) of libuchirp_ddc.so share: how a raw input word
// becomes a float, the carrier of a phase, the mixer and one step of the FIR chain of include/uchirp_ddc.h, written once and
// compiled for both, so that uc_ddc_filter_row (the definition in plain C for one row) and the kernel cannot drift apart;
// and the geometry of the kernel's units of work, which the host needs for the launch.
//
// Every operation of the carrier and the mixer is one correctly rounded float32 multiply, add or subtract; the chain is one
// fused multiply-add per tap.  The device flags contract by default, so everything below stands under a contraction-off
// pragma of this file's own; nothing here may be compiled with flags that flush denormals or relax the arithmetic.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIP__
#define UC_DDC_HD __host__ __device__ __forceinline__
#else
#define UC_DDC_HD inline
#endif

namespace uc_ddc_dev {

constexpr int THREADS = 256;             // a workgroup: four waves; a lane is every 256th output of a span
constexpr int MAX_TAPS = 128;
constexpr int MAX_DECIM = 64;
constexpr int MAX_SETS = 256;
constexpr int STATE_WORDS = 128;         // an input row's state in the caller's memory: the samples in front of `first`
constexpr int TABLE = 1024;              // (cos, sin) pairs of the coarse and of the fine table
constexpr int TILE_IN = 2048;            // the input samples a span's outputs advance over, at most
constexpr int MAX_PER_LANE = TILE_IN / THREADS;   // outputs of one lane in a span: 8 at D = 1

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_DDC_DTYPE_*
constexpr int FMT_IQ = 0, FMT_I = 1;     // UC_DDC_OUT_*

// A span: the outputs of one unit of work.  Its staged samples lie in LDS by phase: sample t of the span (t = 0: the oldest
// one the first output needs) at row t mod D, column t / D of a D x plen matrix, so that the 256 lanes' reads of one tap are
// 256 consecutive elements whatever D is.
constexpr uint32_t span_outputs(uint32_t decim) { return TILE_IN / decim; }
// columns of a row of that matrix: the span's outputs and the taps' reach, odd (so that the staging writes of neighbouring
// samples, plen elements apart, spread over the banks)
constexpr uint32_t span_plen(uint32_t decim) { return (span_outputs(decim) + (MAX_TAPS - 1) / decim + 2) | 1u; }
// the largest D * plen is 2367 (D = 64); a lane without an output reads up to 255 elements behind the last one that counts
constexpr int STAGE_ELEMS = 2367 + THREADS + 1;
// t / D for t < 2^12 as (t * recip) >> 20: recip = ceil(2^20 / D) errs by less than D / 2^20 per unit of t
constexpr uint32_t span_recip(uint32_t decim) { return ((1u << 20) + decim - 1) / decim; }

UC_DDC_HD float bits_to_float(uint32_t raw) {
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(raw);
#else
  float f;
  memcpy(&f, &raw, sizeof(f));
  return f;
#endif
}

// UC_DDC_DTYPE_F32: the float as it is (denormals too); NaN and the infinities read as +0.
// UC_DDC_DTYPE_I32: the 24-bit value of a DFSDM word, (float)(word >> 8): exact.
template <int DT>
UC_DDC_HD float sample_of(uint32_t raw) {
  if (DT == DT_F32) return (raw & 0x7F800000u) == 0x7F800000u ? 0.0f : bits_to_float(raw);
  return (float)((int32_t)raw >> 8);
}

// the phase of the sample with absolute index n (its low 32 bits are all that counts)
UC_DDC_HD uint32_t phase_of(uint32_t phase0, uint32_t step, uint64_t n) { return phase0 + step * (uint32_t)n; }

// (cos, sin) of a phase from the two tables' entries: (cc, sc) = coarse[phase >> 22], (cf, sf) = fine[(phase >> 12) & 1023]
UC_DDC_HD void carrier(float cc, float sc, float cf, float sf, float* c, float* s) {
#pragma clang fp contract(off)
  const float a = cc * cf, b = sc * sf, d = sc * cf, e = cc * sf;
  *c = a - b;
  *s = d + e;
}

// the mixer's one product
UC_DDC_HD float mix(float x, float c) {
#pragma clang fp contract(off)
  return x * c;
}

// one step of a chain
UC_DDC_HD float chain(float h, float m, float acc) { return __builtin_fmaf(h, m, acc); }

struct Params {
  const void* in;
  float* out;
  float* state;              // n_in_rows x 128
  const float* taps;         // n_sets x n_taps, in the object's memory
  const float* tables;       // coarse (2048 floats), fine (2048 floats), in the object's memory
  const uint32_t* row_map;   // n_rows input rows, or NULL: row r reads input row r
  const uint32_t* set_index; // n_rows sets, or NULL: set 0
  const uint32_t* step;      // n_rows steps, or NULL: 0
  const uint32_t* phase0;    // n_rows phases, or NULL: 0
  uint64_t in_stride;        // elements
  uint64_t out_stride;
  uint64_t n_samples;
  uint64_t first;            // the absolute index of in[0]
  uint64_t count;            // outputs of a row
  uint64_t spans;            // ceil(count / span)
  uint64_t units;            // n_rows * spans
  uint32_t n_in_rows;
  uint32_t lead;             // the first output's sample, counted from in[0]: p_first * D - first, below D
  uint32_t n_taps;
  uint32_t decim;
  uint32_t span;             // span_outputs(decim)
  uint32_t plen;             // span_plen(decim)
  uint32_t recip;            // span_recip(decim)
  uint32_t out_vec;          // 1: every output row starts on 8 bytes (pointer and stride allow 8-byte stores of I, Q pairs)
};

// launches (uc_ddc_kernel.hip); dtype: UC_DDC_DTYPE_*; format: UC_DDC_OUT_*; they return the hipError_t of the launch as int
int launch_convert(int dtype, int format, unsigned grid, void* stream, const Params& p);
int launch_state(int dtype, unsigned grid, void* stream, const Params& p);

}  // namespace uc_ddc_dev
