// What the host side (uc_dfsdm_api.cpp) and the kernel file (uc_dfsdm_kernel.hip) of libuchirp_dfsdm.so share: the bit-step,
// the decimation step and the output word of include/uchirp_dfsdm.h, written once and compiled for both, so that
// uc_dfsdm_filter_row (the definition in plain C for one row) and the kernel cannot drift apart.  The word path's tables and
// its matrix are derived here from the same bit-step.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIP__
#define UC_DFSDM_HD __host__ __device__ __forceinline__
#else
#define UC_DFSDM_HD inline
#endif

namespace uc_dfsdm_dev {

constexpr int LANES = 64;                // one wave per workgroup; a lane is one row (one bit stream)
constexpr int STATE_WORDS = 16;          // integ[5], comb[5], fast[2], acc, 3 reserved
constexpr int ST_INTEG = 0, ST_COMB = 5, ST_FAST = 10, ST_ACC = 12, ST_RESERVED = 13;

constexpr int ORDER_FAST = 0, ORDER_MAX = 5;
constexpr uint32_t RATIO_MAX = 1024, INTEG_MAX = 256;
constexpr int SHIFT_MAX = 31;
constexpr int32_t OUT_MAX = (1 << 23) - 1, OUT_MIN = -(1 << 23);
constexpr uint64_t GAIN_MAX = 0x7FFFFFFFull;

// integrator stages of an order: FastSinc runs two
constexpr int stages_of(int order) { return order == ORDER_FAST ? 2 : order; }

// the full-scale gain of the header: R^N I, or 2 R^2 I for FastSinc (R <= 2^10, N <= 5, I <= 2^8: below 2^59)
inline uint64_t gain_of(int order, uint32_t ratio, uint32_t integ) {
  uint64_t g = integ;
  for (int k = 0; k < stages_of(order); ++k) g *= ratio;
  return order == ORDER_FAST ? 2 * g : g;
}

// the carried state of a row, in registers; int32 in two's complement, unsigned here so that every sum wraps
template <int ORDER>
struct State {
  static constexpr int N = stages_of(ORDER);
  uint32_t integ[N], comb[N], fast[2], acc;
};

template <int ORDER>
UC_DFSDM_HD void load_state(State<ORDER>& s, const int32_t* st) {
  for (int k = 0; k < State<ORDER>::N; ++k) {
    s.integ[k] = (uint32_t)st[ST_INTEG + k];
    s.comb[k] = (uint32_t)st[ST_COMB + k];
  }
  s.fast[0] = ORDER == ORDER_FAST ? (uint32_t)st[ST_FAST] : 0u;
  s.fast[1] = ORDER == ORDER_FAST ? (uint32_t)st[ST_FAST + 1] : 0u;
  s.acc = (uint32_t)st[ST_ACC];
}

// the words an order does not use stay as they are; the reserved ones are written 0
template <int ORDER>
UC_DFSDM_HD void store_state(const State<ORDER>& s, int32_t* st) {
  for (int k = 0; k < State<ORDER>::N; ++k) {
    st[ST_INTEG + k] = (int32_t)s.integ[k];
    st[ST_COMB + k] = (int32_t)s.comb[k];
  }
  if (ORDER == ORDER_FAST) {
    st[ST_FAST] = (int32_t)s.fast[0];
    st[ST_FAST + 1] = (int32_t)s.fast[1];
  }
  st[ST_ACC] = (int32_t)s.acc;
  st[ST_RESERVED] = st[ST_RESERVED + 1] = st[ST_RESERVED + 2] = 0;
}

// step 1 of the definition: one input of +1, -1 (a bit) or 0 (what the word path's tables run between a byte and the end
// of its word) through the integrators, each stage on the stage before it as already brought up to date
template <int N>
UC_DFSDM_HD void integrate(uint32_t (&integ)[N], uint32_t s) {
  integ[0] += s;
#pragma unroll
  for (int k = 1; k < N; ++k) integ[k] += integ[k - 1];
}

// step 2: at every R-th bit, the combs (and FastSinc's 1 + z^-2R), into the accumulator
template <int ORDER>
UC_DFSDM_HD void decimate(State<ORDER>& s) {
  constexpr int N = State<ORDER>::N;
  uint32_t v = s.integ[N - 1];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint32_t d = v - s.comb[k];
    s.comb[k] = v;
    v = d;
  }
  if (ORDER == ORDER_FAST) {
    const uint32_t w = v + s.fast[1];
    s.fast[1] = s.fast[0];
    s.fast[0] = v;
    v = w;
  }
  s.acc += v;
}

// step 3: at every I-th such value, the output word: clip((y >> shift) - offset, -2^23, 2^23 - 1) * 256.  (y >> shift is
// first held to +-2^25: |offset| <= 2^23, so the difference cannot wrap and the clip's result is the same.)
template <int ORDER>
UC_DFSDM_HD int32_t output_word(State<ORDER>& s, int shift, int32_t offset) {
  int32_t y = (int32_t)s.acc >> shift;
  s.acc = 0;
  y = y > (1 << 25) ? (1 << 25) : y;
  y = y < -(1 << 25) ? -(1 << 25) : y;
  y -= offset;
  y = y > OUT_MAX ? OUT_MAX : y;
  y = y < OUT_MIN ? OUT_MIN : y;
  return (int32_t)((uint32_t)y << 8);
}

// where a row stands between the R and the I boundaries: bits since the last R-th bit, values since the last output.  A
// function of words_before and the configuration alone, so one value for every row of a call
struct Phase {
  uint32_t r, i;
};

inline Phase phase_of(uint64_t words_before, uint32_t ratio, uint32_t integ) {
  const uint64_t bits = 32 * words_before;
  return Phase{(uint32_t)(bits % ratio), (uint32_t)((bits / ratio) % integ)};
}

// THE BIT PATH: the definition's loop over the 32 bits of one word.  emit(word) takes each output as it falls.
template <int ORDER, class Emit>
UC_DFSDM_HD void word_by_bits(State<ORDER>& s, uint32_t w, Phase& ph, uint32_t ratio, uint32_t integ, int shift, int32_t offset, Emit& emit) {
  for (int b = 0; b < 32; ++b) {
    integrate(s.integ, 2u * ((w >> b) & 1u) - 1u);
    if (++ph.r == ratio) {
      ph.r = 0;
      decimate(s);
      if (++ph.i == integ) {
        ph.i = 0;
        emit(output_word(s, shift, offset));
      }
    }
  }
}

// ---- the word path (R a multiple of 32): what 32 bit-steps do to the integrators, at once.
// The integrators are linear in their state and their inputs, so over one word
//   integ' = M integ + sum over the word's four bytes of T[byte position][byte value]
// M: 32 bit-steps with input 0; lower triangular and constant along its diagonals, so its first column says it all.
// T: the byte's eight bits from a zero state, then input 0 to the end of the word.
// Both are taken from `integrate` itself, M at compile time.
constexpr uint32_t word_matrix(int d) {
  uint32_t v[ORDER_MAX] = {1, 0, 0, 0, 0};
  for (int t = 0; t < 32; ++t)
    for (int k = 1; k < ORDER_MAX; ++k) v[k] += v[k - 1];     // `integrate` with s = 0, spelled out for a constant expression
  return v[d];
}
static_assert(word_matrix(0) == 1 && word_matrix(1) == 32 && word_matrix(2) == 528 && word_matrix(3) == 5984 && word_matrix(4) == 52360,
              "the diagonals of 32 zero-input steps: C(31 + d, d)");

template <int N>
UC_DFSDM_HD void advance_word(uint32_t (&integ)[N], const uint32_t (&add)[N]) {
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    uint32_t v = integ[k] + add[k];
#pragma unroll
    for (int j = 0; j < k; ++j) v += word_matrix(k - j) * integ[j];
    integ[k] = v;
  }
}

// entry e = 256 * byte position + byte value of the tables: ORDER_MAX ints, the stages an order does not run are 0
constexpr int TABLE_ENTRIES = 4 * 256;
template <int N>
inline void table_entry(int pos, uint32_t value, uint32_t (&out)[N]) {
  for (int k = 0; k < N; ++k) out[k] = 0;
  for (int t = 8 * pos; t < 32; ++t) integrate(out, t < 8 * pos + 8 ? 2u * ((value >> (t - 8 * pos)) & 1u) - 1u : 0u);
}

struct Params {
  const uint32_t* in;        // n_rows rows of n_words packed PDM words
  int32_t* out;              // n_rows rows of n_out words
  int32_t* state;            // n_rows x 16
  const int32_t* table;      // word path: TABLE_ENTRIES x 4 ints (stages 0 .. 3), then TABLE_ENTRIES ints (stage 4)
  uint64_t in_stride;        // words
  uint64_t out_stride;
  uint64_t n_words;
  uint64_t n_out;
  uint32_t n_rows;
  uint32_t row_blocks;       // ceil(n_rows / LANES)
  uint32_t ratio, integ;
  uint32_t phase_r, phase_i; // Phase at the call's first bit
  int32_t shift, offset;
  uint32_t in_vec;           // 1: every row of the input starts on 16 bytes (pointer and stride allow b128 loads)
  uint32_t out_vec;          // 1: the same of the output
};

// launch (uc_dfsdm_kernel.hip); word_path: R is a multiple of 32; returns the hipError_t of the launch as int
int launch_filter(int order, bool word_path, unsigned grid, void* stream, const Params& p);

}  // namespace uc_dfsdm_dev
