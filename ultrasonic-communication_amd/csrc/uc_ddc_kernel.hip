// uc_ddc_kernel.hip -- the down-converter's kernels (gfx950): every output row is one input row (float or DFSDM words) times
// the carrier of a 32-bit phase accumulator, through a FIR of 1 .. 128 taps, decimated by D.  include/uchirp_ddc.h states the
// definition; uchirp/ddc.py holds it in numpy float32 (`emulate32`); uc_ddc.hpp holds the arithmetic itself, shared with
// uc_ddc_filter_row.
//
// A FIR is parallel in time.  A unit of work is (output row, span): the span_outputs(D) = 2048 / D outputs from a multiple
// of that number on.  Units are dealt blockIdx.x, + gridDim.x, ...; a workgroup of four waves loads the carrier's two tables
// (16 KB) into LDS once and then walks its units:
//   stage   the span's (S - 1) D + n_taps samples -- those in front of in[0] from the row's state -- are converted and mixed
//           ONCE each: lane-consecutive dword loads, two table reads, the six operations of the carrier, the two products;
//           the pair (mi, mq) -- mi alone for UC_DDC_OUT_I -- goes to LDS BY PHASE: sample t to row t mod D, column t / D.
//           The set's taps go to LDS next to them.
//   dot     lane l owns the outputs l, l + 256, ... of the span (at most 8).  Output o, tap k reads sample o D + (n_taps - 1
//           - k): row (n_taps - 1 - k) mod D, column o + (n_taps - 1 - k) / D.  Row and column offset are the same for the
//           whole workgroup (scalar arithmetic), the lanes' columns are consecutive: one ds_read_b64 per output and tap
//           without a bank conflict at ANY D, its address the lane's own plus an immediate per output, and behind it the I
//           and the Q fused multiply-add.  The 2 x 8 chains of a lane are independent; within a chain k runs 0, 1, ... as
//           the definition says.  The tap itself is one broadcast LDS read per k for the 16 multiply-adds.
//   store   lane-consecutive: 8-byte stores of I, Q pairs where the rows lie on 8 bytes, dwords otherwise.
// A second kernel, launched behind the first on the same stream, brings the states up to date: one pass per input row, which
// reads all of the new state (from the row's last samples and, for calls shorter than 128 samples, the old state's tail)
// before it writes.
//
// Built for 4 workgroups per CU (4 waves per SIMD): at most 128 registers and 40 KB of LDS (tests/test_ddc_cpu.py reads both
// from the code object).  The bits depend on the row's samples, state, taps, step, phase and position only, never on the
// path or the grid.
#include <hip/hip_runtime.h>

#include "uc_ddc.hpp"

namespace uc_ddc_dev {
namespace {

constexpr uint32_t max_stage_elems() {
  uint32_t m = 0;
  for (uint32_t d = 1; d <= (uint32_t)MAX_DECIM; ++d) m = d * span_plen(d) > m ? d * span_plen(d) : m;
  return m;
}
static_assert(max_stage_elems() + THREADS <= (uint32_t)STAGE_ELEMS, "the staged span and the idle lanes' reach fit the LDS array");
static_assert((TILE_IN + MAX_TAPS) < 4096, "span_recip divides what a span stages");

template <int FMT>
struct Elem;
template <>
struct Elem<FMT_IQ> {
  typedef float2 type;
};
template <>
struct Elem<FMT_I> {
  typedef float type;
};

__device__ __forceinline__ float2 make_elem(float mi, float mq, float2*) { return make_float2(mi, mq); }
__device__ __forceinline__ float make_elem(float mi, float, float*) { return mi; }

// the chains of RB outputs of this lane over all taps, and their stores.  `mine`: the lane's column 0 of the staged matrix
// (stage + threadIdx.x); cnt: the span's outputs; dst: the row's element of the span's output 0.
template <int FMT, int RB>
__device__ __forceinline__ void dot(const typename Elem<FMT>::type* mine, const float* taps, const Params& p, uint32_t cnt, float* dst) {
  typedef typename Elem<FMT>::type E;
  float ai[RB], aq[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) ai[j] = aq[j] = 0.0f;
  const uint32_t n_taps = p.n_taps, decim = p.decim, plen = p.plen;
  uint32_t row = (n_taps - 1) % decim, col = (n_taps - 1) / decim;     // of the sample that tap 0 meets at output 0
  for (uint32_t k = 0; k < n_taps; ++k) {
    const float h = taps[k];
    const E* const at = mine + row * plen + col;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const E v = at[j * THREADS];
      if constexpr (FMT == FMT_IQ) {
        ai[j] = chain(h, v.x, ai[j]);
        aq[j] = chain(h, v.y, aq[j]);
      } else {
        ai[j] = chain(h, v, ai[j]);
      }
    }
    if (row == 0) {
      row = decim - 1;
      --col;                                                            // (wraps behind the last tap only)
    } else {
      --row;
    }
  }
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const uint32_t o = threadIdx.x + j * THREADS;
    if (o >= cnt) break;
    if constexpr (FMT == FMT_IQ) {
      if (p.out_vec) {
        *reinterpret_cast<float2*>(dst + 2 * (uint64_t)o) = make_float2(ai[j], aq[j]);
      } else {
        dst[2 * (uint64_t)o] = ai[j];
        dst[2 * (uint64_t)o + 1] = aq[j];
      }
    } else {
      dst[o] = ai[j];
    }
  }
}

template <int DT, int FMT>
__global__ __launch_bounds__(THREADS) void ddc_kernel(const Params p) {
  typedef typename Elem<FMT>::type E;
  __shared__ float2 coarse[TABLE], fine[TABLE];
  __shared__ E stage[STAGE_ELEMS];
  __shared__ float taps[MAX_TAPS];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < (uint32_t)TABLE; i += THREADS) {
    coarse[i] = reinterpret_cast<const float2*>(p.tables)[i];
    fine[i] = reinterpret_cast<const float2*>(p.tables)[TABLE + i];
  }
  constexpr uint32_t WORDS = FMT == FMT_IQ ? 2 : 1;
  for (uint64_t u = blockIdx.x; u < p.units; u += gridDim.x) {
    const uint64_t r = u / p.spans, sp = u - r * p.spans;
    const uint64_t o0 = sp * p.span;                                    // the span's first output, counted from the row's
    const uint64_t left = p.count - o0;
    const uint32_t cnt = left < p.span ? (uint32_t)left : p.span;
    const uint64_t src = p.row_map ? p.row_map[r] : r;
    const uint32_t set = p.set_index ? p.set_index[r] : 0u;
    const uint32_t step = p.step ? p.step[r] : 0u, phase0 = p.phase0 ? p.phase0[r] : 0u;
    const uint32_t* const in = (const uint32_t*)p.in + src * p.in_stride;
    const float* const st = p.state + src * STATE_WORDS;
    // sample t of the span is in[i0 + t]; in front of in[0]: the state's st[128 + i0 + t]
    const int64_t i0 = (int64_t)(p.lead + o0 * p.decim) - (int64_t)(p.n_taps - 1);
    const uint32_t n_stage = (cnt - 1) * p.decim + p.n_taps;
    __syncthreads();                                                    // the tables are there; the last unit's reads are over
    if (tid < p.n_taps) taps[tid] = p.taps[(uint64_t)set * p.n_taps + tid];
    for (uint32_t t = tid; t < n_stage; t += THREADS) {
      const int64_t i = i0 + (int64_t)t;
      const float x = i >= 0 ? sample_of<DT>(in[i]) : st[STATE_WORDS + i];
      const uint32_t ph = phase_of(phase0, step, p.first + (uint64_t)i);
      const float2 cs = coarse[ph >> 22], fs = fine[(ph >> 12) & (TABLE - 1)];
      float c, s;
      carrier(cs.x, cs.y, fs.x, fs.y, &c, &s);
      const uint32_t col = (t * p.recip) >> 20, row = t - col * p.decim;
      stage[row * p.plen + col] = make_elem(mix(x, c), FMT == FMT_IQ ? mix(x, s) : 0.0f, (E*)nullptr);
    }
    __syncthreads();
    float* const dst = p.out + r * p.out_stride + o0 * WORDS;
    const E* const mine = stage + tid;
    switch ((cnt + THREADS - 1) / THREADS) {                            // the outputs of a lane: uniform
      case 1: dot<FMT, 1>(mine, taps, p, cnt, dst); break;
      case 2: dot<FMT, 2>(mine, taps, p, cnt, dst); break;
      case 3: dot<FMT, 3>(mine, taps, p, cnt, dst); break;
      case 4: dot<FMT, 4>(mine, taps, p, cnt, dst); break;
      case 5: dot<FMT, 5>(mine, taps, p, cnt, dst); break;
      case 6: dot<FMT, 6>(mine, taps, p, cnt, dst); break;
      case 7: dot<FMT, 7>(mine, taps, p, cnt, dst); break;
      default: dot<FMT, 8>(mine, taps, p, cnt, dst); break;
    }
  }
}

// the states behind the call: word j of a row's new state is the sample n_samples - 128 + j of the call, which for a call
// shorter than 128 samples is word j + n_samples of the old state.  128 lanes per row; all reads before the writes.
template <int DT>
__global__ __launch_bounds__(STATE_WORDS) void ddc_state_kernel(const Params p) {
  const uint32_t j = threadIdx.x;
  for (uint64_t r = blockIdx.x; r < p.n_in_rows; r += gridDim.x) {
    float* const st = p.state + r * STATE_WORDS;
    const int64_t i = (int64_t)p.n_samples - STATE_WORDS + (int64_t)j;
    const float v = i >= 0 ? sample_of<DT>(((const uint32_t*)p.in + r * p.in_stride)[i]) : st[j + p.n_samples];
    __syncthreads();
    st[j] = v;
  }
}

template <int DT>
int launch_format(int format, unsigned grid, hipStream_t hs, const Params& p) {
  switch (format) {
    case FMT_IQ: hipLaunchKernelGGL((ddc_kernel<DT, FMT_IQ>), dim3(grid), dim3(THREADS), 0, hs, p); break;
    case FMT_I: hipLaunchKernelGGL((ddc_kernel<DT, FMT_I>), dim3(grid), dim3(THREADS), 0, hs, p); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace

int launch_convert(int dtype, int format, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: return launch_format<DT_F32>(format, grid, hs, p);
    case DT_I32: return launch_format<DT_I32>(format, grid, hs, p);
    default: return (int)hipErrorInvalidValue;
  }
}

int launch_state(int dtype, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((ddc_state_kernel<DT_F32>), dim3(grid), dim3(STATE_WORDS), 0, hs, p); break;
    case DT_I32: hipLaunchKernelGGL((ddc_state_kernel<DT_I32>), dim3(grid), dim3(STATE_WORDS), 0, hs, p); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_ddc_dev
