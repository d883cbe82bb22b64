// uc_duc_kernel.hip -- the up-converter's kernels (gfx950): every output row is the sum of n_chan channels, each one base-band
// input row (I, Q pairs or I alone) interpolated by L through a polyphase FIR of K taps per phase and multiplied by the
// carrier of a 32-bit phase accumulator; floats or int16 PCM leave.  include/uchirp_duc.h states the definition;
// uchirp/duc.py holds it in numpy float32 (`emulate32`); uc_duc.hpp holds the arithmetic itself, shared with
// uc_duc_filter_row and uc_duc_sum_row.
//
// A unit of work is (output row, span): the span_outputs(L) = (2048 div L) L outputs from a multiple of that number on, so
// a span starts on phase 0 of an input sample.  Units are dealt blockIdx.x, + gridDim.x, ...; a workgroup of four waves
// loads the carrier's two tables (16 KB) into LDS once and then walks its units.  Lane l owns the outputs l, l + 256, ... of
// the span (at most 8) and keeps their sums over the channels in registers.  Per channel:
//   stage   the span's (2048 div L) + K - 1 input samples -- those in front of in[0] from the input row's state -- go to LDS
//           as they are (not finite: +0), lane-consecutive 8-byte loads where the rows lie on 8 bytes, dwords otherwise;
//           the set's prototype, which already is [k][rho] (h[rho + k L]), goes behind them.
//   dot     output o = m L + rho, tap k reads sample m - k and tap rho + k L.  Consecutive lanes read consecutive rho of one
//           k (mod L) and groups of L lanes one sample: both reads broadcast or walk the banks.  Where L divides 256 the
//           lane's outputs share rho: one tap read per k serves its 8 x 2 chains, and the samples' addresses are the lane's
//           own plus an immediate per output; elsewhere every output reads its own tap.  Within a chain k runs 0, 1, ... as
//           the definition says.
//   mix     the carrier at the OUTPUT index: two table reads, six operations, then (ai c) + (aq s), and the sum over the
//           channels in channel order (the first channel starts the sum: no +0 is added).
// Behind the last channel: floats leave lane-consecutive; int16 values go through LDS, so that a row leaves as single
// values up to the first 8-byte boundary (a pair where 4 bytes are left to it), 8-byte stores of quads, and a pair and a
// single at the end.  The clipped values of a unit are counted in LDS and added to the row's count with one atomic.
// A second kernel, launched behind the first on the same stream, brings the states up to date: one pass per input row, which
// reads all of the new state before it writes.
//
// Built for 4 workgroups per CU (4 waves per SIMD): at most 128 registers and 40 KB of LDS (tests/test_duc_cpu.py reads both
// from the code object).  The bits depend on the channels' samples, states, taps, steps, phases and position only, never on
// the path or the grid.
#include <hip/hip_runtime.h>

#include "uc_duc.hpp"

namespace uc_duc_dev {
namespace {

constexpr uint32_t max_pool_floats() {
  uint32_t m = 0;
  for (uint32_t l = 1; l <= (uint32_t)MAX_INTERP; ++l)
    for (uint32_t k = 1; k <= (uint32_t)MAX_PHASE_TAPS && k * l <= (uint32_t)MAX_TAPS; ++k) m = pool_floats(l, k) > m ? pool_floats(l, k) : m;
  return m;
}
static_assert(max_pool_floats() <= (uint32_t)POOL_FLOATS, "the staged samples and the tap set fit the LDS pool");
static_assert(TILE_OUT < 4096, "span_recip divides what a span holds");
static_assert(TILE_OUT * sizeof(int16_t) <= POOL_FLOATS * sizeof(float), "the int16 values of a span fit the pool");

struct Shared {
  float2 coarse[TABLE], fine[TABLE];
  float pool[POOL_FLOATS];
  uint32_t clipped;
};

// the unit's int16 values, o0 .. o0 + cnt - 1 of the row, from LDS to dst (the row's element o0): wide stores where dst
// allows them
__device__ __forceinline__ void store_i16(const int16_t* vals, int16_t* dst, uint32_t cnt) {
  const uint32_t tid = threadIdx.x;
  const uint32_t at = (uint32_t)((uintptr_t)dst >> 1) & 3u;              // dst's place in its 8 bytes, in elements
  // the head: a single where dst is off 4 bytes, then a pair where 4 bytes are left to the 8-byte boundary (cnt >= 1)
  const uint32_t single = at & 1u;
  const uint32_t pair = ((at + single) & 3u) == 2u && cnt - single >= 2u ? 2u : 0u;
  const uint32_t head = single + pair;
  if (tid == 0 && single) dst[0] = vals[0];
  if (tid == 1 && pair) *reinterpret_cast<uint32_t*>(dst + single) = (uint32_t)(uint16_t)vals[single] | ((uint32_t)(uint16_t)vals[single + 1] << 16);
  const uint32_t quads = (cnt - head) >> 2;
  for (uint32_t q = tid; q < quads; q += THREADS) {
    const uint32_t e = head + 4u * q;
    uint2 v;
    v.x = (uint32_t)(uint16_t)vals[e] | ((uint32_t)(uint16_t)vals[e + 1] << 16);
    v.y = (uint32_t)(uint16_t)vals[e + 2] | ((uint32_t)(uint16_t)vals[e + 3] << 16);
    *reinterpret_cast<uint2*>(dst + e) = v;
  }
  // the tail: a pair, then a single
  const uint32_t tail0 = head + 4u * quads, tail = cnt - tail0;
  if (tid == 2 && tail >= 2u) *reinterpret_cast<uint32_t*>(dst + tail0) = (uint32_t)(uint16_t)vals[tail0] | ((uint32_t)(uint16_t)vals[tail0 + 1] << 16);
  if (tid == 3 && (tail & 1u)) dst[cnt - 1] = vals[cnt - 1];
}

// one unit: row r, the cnt outputs from o0 on; RB: the outputs of a lane; UNI: L divides 256
template <int IN, int OUT, int RB, bool UNI>
__device__ __forceinline__ void unit(Shared& sh, const Params& p, uint64_t r, uint64_t sp, uint64_t o0, uint32_t cnt) {
  constexpr uint32_t WORDS = IN == IN_IQ ? 2 : 1;
  const uint32_t tid = threadIdx.x;
  const uint32_t K = p.k_taps, L = p.interp, n_taps = K * L;
  float* const stage = sh.pool;
  float* const taps = sh.pool + (p.span_in + K) * WORDS;
  // the lane's outputs: their sample (counted from the span's first) and their phase of the filter
  constexpr int OWN = UNI ? 1 : RB;                                      // (L divides 256: m[j] = m[0] + j (256 / L), rho[j] = rho[0])
  uint32_t m[OWN], rho[OWN];
#pragma unroll
  for (int j = 0; j < OWN; ++j) {
    const uint32_t o = tid + j * THREADS;
    m[j] = (o * p.recip) >> 20;
    rho[j] = o - m[j] * L;
  }
  // sample t of the span (t = 0: the oldest one that output 0 needs) is sample i0 + t of the call; in front of the call's
  // first: the state's sample 128 + i0 + t
  const int64_t i0 = (int64_t)(sp * p.span_in) - (int64_t)(K - 1);
  const uint32_t n_stage = cnt / L + K - 1;                              // (cnt is a multiple of L)
  float sum[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) sum[j] = 0.0f;                            // (channel 0 replaces it: no +0 is added)
  for (uint32_t ch = 0; ch < p.n_chan; ++ch) {
    const uint64_t slot = r * p.n_chan + ch;
    uint64_t src = slot;
    uint32_t set = 0u, step = 0u, phase0 = 0u;
    if (p.chan) {
      const Channel c = p.chan[slot];
      src = c.row;
      set = c.set;
      step = c.step;
      phase0 = c.phase0;
    }
    const uint32_t* const in = p.in + src * p.in_stride;
    const uint32_t* const st = reinterpret_cast<const uint32_t*>(p.state) + src * (STATE_SAMPLES * WORDS);
    __syncthreads();                                                     // the tables are there; the last reads of the pool are over
    for (uint32_t k = tid; k < n_taps; k += THREADS) taps[k] = p.taps[(uint64_t)set * n_taps + k];
    for (uint32_t t = tid; t < n_stage; t += THREADS) {
      const int64_t i = i0 + (int64_t)t;
      if constexpr (IN == IN_IQ) {
        uint32_t a, b;
        if (i < 0) {
          a = st[2 * (STATE_SAMPLES + i)];                               // (the state holds what sample_of gave)
          b = st[2 * (STATE_SAMPLES + i) + 1];
        } else if (p.in_vec) {
          const uint2 v = reinterpret_cast<const uint2*>(in)[i];
          a = v.x;
          b = v.y;
        } else {
          a = in[2 * i];
          b = in[2 * i + 1];
        }
        reinterpret_cast<float2*>(stage)[t] = make_float2(sample_of(a), sample_of(b));
      } else {
        stage[t] = sample_of(i < 0 ? st[STATE_SAMPLES + i] : in[i]);
      }
    }
    __syncthreads();
    float ai[RB], aq[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) ai[j] = aq[j] = 0.0f;
    if constexpr (UNI) {
      const uint32_t per = THREADS / L;
      const float* tp = taps + rho[0];
      if constexpr (IN == IN_IQ) {
        const float2* at = reinterpret_cast<const float2*>(stage) + m[0] + (K - 1);
        for (uint32_t k = 0; k < K; ++k) {
          const float h = *tp;
#pragma unroll
          for (int j = 0; j < RB; ++j) {
            const float2 v = at[j * per];
            ai[j] = chain(h, v.x, ai[j]);
            aq[j] = chain(h, v.y, aq[j]);
          }
          tp += L;
          --at;
        }
      } else {
        const float* at = stage + m[0] + (K - 1);
        for (uint32_t k = 0; k < K; ++k) {
          const float h = *tp;
#pragma unroll
          for (int j = 0; j < RB; ++j) ai[j] = chain(h, at[j * per], ai[j]);
          tp += L;
          --at;
        }
      }
    } else {
      for (uint32_t k = 0; k < K; ++k) {
        const uint32_t back = K - 1 - k;
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          const float h = taps[k * L + rho[j]];
          if constexpr (IN == IN_IQ) {
            const float2 v = reinterpret_cast<const float2*>(stage)[m[j] + back];
            ai[j] = chain(h, v.x, ai[j]);
            aq[j] = chain(h, v.y, aq[j]);
          } else {
            ai[j] = chain(h, stage[m[j] + back], ai[j]);
          }
        }
      }
    }
    // the carrier at the output's own index, the mixer, the sum over the channels
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const uint32_t ph = phase_of(phase0, step, p.first_out + o0 + (uint64_t)(tid + j * THREADS));
      const float2 cs = sh.coarse[ph >> 22], fs = sh.fine[(ph >> 12) & (TABLE - 1)];
      float c, s;
      carrier(cs.x, cs.y, fs.x, fs.y, &c, &s);
      const float y = IN == IN_IQ ? mix_iq(ai[j], aq[j], c, s) : mix_i(ai[j], c);
      sum[j] = ch == 0 ? y : add_channel(sum[j], y);
    }
  }
  // the output stage
  if constexpr (OUT == OUT_F32) {
    float* const dst = reinterpret_cast<float*>(p.out) + r * p.out_stride + o0;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const uint32_t o = tid + j * THREADS;
      if (o < cnt) dst[o] = sum[j];
    }
  } else {
    int16_t* const vals = reinterpret_cast<int16_t*>(sh.pool);
    __syncthreads();                                                     // the last channel's reads of the pool are over
    if (tid == 0) sh.clipped = 0u;
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const uint32_t o = tid + j * THREADS;
      if (o < cnt) {
        bool clipped;
        vals[o] = to_i16(sum[j], &clipped);
        mine += clipped ? 1u : 0u;
      }
    }
    __syncthreads();
    if (p.clip && mine) atomicAdd(&sh.clipped, mine);
    store_i16(vals, reinterpret_cast<int16_t*>(p.out) + r * p.out_stride + o0, cnt);
    __syncthreads();
    if (p.clip && tid == 0 && sh.clipped) atomicAdd(p.clip + r, sh.clipped);
  }
}

template <int IN, int OUT, int RB, bool UNI>
__global__ __launch_bounds__(THREADS) void duc_kernel(const Params p) {
  __shared__ Shared sh;
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < (uint32_t)TABLE; i += THREADS) {
    sh.coarse[i] = reinterpret_cast<const float2*>(p.tables)[i];
    sh.fine[i] = reinterpret_cast<const float2*>(p.tables)[TABLE + i];
  }
  for (uint64_t u = blockIdx.x; u < p.units; u += gridDim.x) {
    const uint64_t r = u / p.spans, sp = u - r * p.spans;
    const uint64_t o0 = sp * p.span;                                     // the span's first output, counted from the row's
    const uint64_t left = p.count - o0;
    unit<IN, OUT, RB, UNI>(sh, p, r, sp, o0, left < p.span ? (uint32_t)left : p.span);
  }
}

// the states behind the call: word w of a row's new state is word (n_samples - 128) WORDS + w of the call's row, which for
// a call shorter than 128 samples is word w + n_samples WORDS of the old state.  One lane per word; all reads before the
// writes.
template <int IN>
__global__ __launch_bounds__(2 * STATE_SAMPLES) void duc_state_kernel(const Params p) {
  constexpr uint32_t WORDS = IN == IN_IQ ? 2 : 1;
  const uint32_t w = threadIdx.x;
  for (uint64_t r = blockIdx.x; r < p.n_in_rows; r += gridDim.x) {
    uint32_t* const st = reinterpret_cast<uint32_t*>(p.state) + r * (STATE_SAMPLES * WORDS);
    const int64_t i = ((int64_t)p.n_samples - STATE_SAMPLES) * (int64_t)WORDS + (int64_t)w;
    const uint32_t v = i >= 0 ? (p.in + r * p.in_stride)[i] : st[w + p.n_samples * WORDS];
    __syncthreads();
    st[w] = i >= 0 ? __float_as_uint(sample_of(v)) : v;
    __syncthreads();
  }
}

// RB: the outputs of a lane in the call's longest span (1, 2, 4 or 8: a shorter last span leaves lanes idle); UNI: L divides 256
template <int IN, int OUT, int RB>
int launch_uni(bool uniform, unsigned grid, hipStream_t hs, const Params& p) {
  if (uniform)
    hipLaunchKernelGGL((duc_kernel<IN, OUT, RB, true>), dim3(grid), dim3(THREADS), 0, hs, p);
  else
    hipLaunchKernelGGL((duc_kernel<IN, OUT, RB, false>), dim3(grid), dim3(THREADS), 0, hs, p);
  return (int)hipGetLastError();
}

template <int IN, int OUT>
int launch_rb(unsigned grid, hipStream_t hs, const Params& p) {
  const uint64_t longest = p.count < p.span ? p.count : p.span;
  const bool uniform = THREADS % p.interp == 0;
  if (longest <= 1 * THREADS) return launch_uni<IN, OUT, 1>(uniform, grid, hs, p);
  if (longest <= 2 * THREADS) return launch_uni<IN, OUT, 2>(uniform, grid, hs, p);
  if (longest <= 4 * THREADS) return launch_uni<IN, OUT, 4>(uniform, grid, hs, p);
  return launch_uni<IN, OUT, 8>(uniform, grid, hs, p);
}

template <int IN>
int launch_out(int out_format, unsigned grid, hipStream_t hs, const Params& p) {
  switch (out_format) {
    case OUT_F32: return launch_rb<IN, OUT_F32>(grid, hs, p);
    case OUT_I16: return launch_rb<IN, OUT_I16>(grid, hs, p);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace

int launch_convert(int in_format, int out_format, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (in_format) {
    case IN_IQ: return launch_out<IN_IQ>(out_format, grid, hs, p);
    case IN_I: return launch_out<IN_I>(out_format, grid, hs, p);
    default: return (int)hipErrorInvalidValue;
  }
}

int launch_state(int in_format, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (in_format) {
    case IN_IQ: hipLaunchKernelGGL((duc_state_kernel<IN_IQ>), dim3(grid), dim3(2 * STATE_SAMPLES), 0, hs, p); break;
    case IN_I: hipLaunchKernelGGL((duc_state_kernel<IN_I>), dim3(grid), dim3(STATE_SAMPLES), 0, hs, p); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_duc_dev
