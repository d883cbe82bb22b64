// uc_link_kernel.hip -- the link simulator's kernels (gfx950): what n_streams microphones receive from n_streams
// independent chirp transmissions, rendered in one pass into the receiver's input buffer (include/uchirp_link.h
// states the definition; uchirp/link.py holds its float64 model).
//
// Shape: one lane owns one Philox counter = four consecutive samples 4c .. 4c + 3 (absolute indices) = one 16-byte
// store (8 bytes for int16); a wave owns 256 consecutive samples of one stream; a workgroup takes tiles of 1024
// samples, dealt statically over (stream, tile) to a persistent grid.  Nothing is shared between lanes: no LDS, no
// barrier, no atomics.  A value depends only on (seed, stream, sample index, the stream's parameters), never on the
// grid or on where a call's first_sample cuts the recording.
//
// Signal: the phase f t - 1/4 (+ 1/8: cos a + sin a = sqrt 2 sin(a + pi/4)) is kept in TURNS in double precision (up
// to ~500 turns inside a symbol: float would leave 3e-5 turns), reduced to [-1/2, 1/2] and only then rounded to float;
// sinpif takes it from there.  sinpif is the library function, not the hardware sine: the bound of 8 float ulp at the
// peak leaves the sine 4, which the library function meets by construction (<= 2 ulp of its own result) while the
// hardware instruction's absolute error near the peak is not specified that tightly.
// Noise: Philox4x32-10 -> 24-bit uniforms centred in their cell -> Box-Muller.  u = (k + 1/2) 2^-24 has 25 significant
// bits for k >= 2^23, so the half bit float drops is carried next to it: ln u = ln u_hi + u_lo / u_hi, and the angle
// 2 pi u is folded to (0, 1/2) pi in integers, where it is exact in float again.
#include <hip/hip_runtime.h>

#include "uc_link.hpp"

namespace uc_link_dev {
namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr int DT_I32 = 0, DT_F32 = 1, DT_I16 = 3;   // UC_LINK_DTYPE_*

struct Words {
  uint32_t w[4];
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return Words{{c0, c1, c2, c3}};
}

// two words -> two independent standard normals (Box-Muller on u = ((w >> 8) + 1/2) 2^-24)
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float kf = (float)(wa >> 8);                       // exact: 24 bits
  const float sh = kf + 0.5f;                              // rounds to even from 2^23 on ...
  const float lo = ((kf - sh) + 0.5f) * 0x1p-24f;          // ... and this is exactly what it dropped (0 or +-2^-25)
  const float hi = sh * 0x1p-24f;                          // in (0, 1]
  const float ln_u = logf(hi) + lo * __builtin_amdgcn_rcpf(hi);
  const float r = sqrtf(-2.0f * ln_u);
  // angle 2 pi u = pi * m 2^-24, m = 2 (w >> 8) + 1 odd in [1, 2^25): fold to pi * m' 2^-24 with m' < 2^23
  uint32_t m = 2u * (wb >> 8) + 1u;
  const bool neg_both = m >= (1u << 24);                   // + pi: both signs flip
  m &= (1u << 24) - 1u;
  const bool neg_cos = m > (1u << 23);                     // pi - x: the cosine's sign flips
  m = neg_cos ? (1u << 24) - m : m;
  float s, c;
  sincospif((float)m * 0x1p-24f, &s, &c);
  z0 = r * ((neg_both != neg_cos) ? -c : c);
  z1 = r * (neg_both ? -s : s);
}

// the transmitter's law at absolute sample jd of one stream (0 in silence and outside the frame)
__device__ __forceinline__ float signal_at(const Params& p, const Stream& st, const uint8_t* __restrict__ text, uint32_t n_on,
                                           double jd) {
  const double tt = jd * st.rate - st.lead_s;
  const double q = floor((tt + 1e-10) * p.inv_sym_dur);
  // symbols 1 .. n_on - 1 sound (0 is the leading G; from n_on on: the guard, then nothing)
  if (!(q >= 1.0 && q < (double)n_on)) return 0.0f;
  const uint32_t idx = (uint32_t)q;
  const double tau = fmax(tt - q * p.sym_dur, 0.0);
  const double t = tau * p.t_scale;
  bool up = idx <= p.n_preamble;                           // preamble H; idx == n_preamble + 1 is the delimiter L
  if (idx > p.n_preamble + 1u) {
    const uint32_t b = idx - p.n_preamble - 2u;            // data bit, MSB first
    up = (text[b >> 3] >> (7u - (b & 7u))) & 1u;
  }
  const double f = up ? p.f0 + p.half_k * t : p.f1 - p.half_k * t;
  double ph = f * t - 0.125;                               // turns: (2 pi f t - pi/2 + pi/4) / 2 pi
  ph -= rint(ph);
  return st.amp * sinpif(2.0f * (float)ph);
}

template <int DT>
struct Out;
template <>
struct Out<DT_F32> {
  using T = float;
  using V = float4;
  static __device__ __forceinline__ T cvt(float x) { return x; }
};
template <>
struct Out<DT_I32> {
  using T = int32_t;
  using V = int4;
  static __device__ __forceinline__ T cvt(float x) {
    return (int32_t)fminf(fmaxf(rintf(x), -8388608.0f), 8388607.0f) * 256;
  }
};
template <>
struct Out<DT_I16> {
  using T = int16_t;
  using V = short4;
  static __device__ __forceinline__ T cvt(float x) { return (int16_t)(int32_t)fminf(fmaxf(x, -32768.0f), 32767.0f); }
};

template <int DT>
__global__ __launch_bounds__(THREADS) void link_kernel(const Params p, const Stream* __restrict__ streams,
                                                       const uint8_t* __restrict__ text, void* __restrict__ out_v) {
  using T = typename Out<DT>::T;
  using V = typename Out<DT>::V;
  T* __restrict__ out = (T*)out_v;
  const uint64_t n_tiles = (uint64_t)p.n_streams * p.tiles_per_stream;
  const uint64_t end = p.first_sample + p.n_samples;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t s = (uint32_t)(tile / p.tiles_per_stream);
    const uint32_t tl = (uint32_t)(tile - (uint64_t)s * p.tiles_per_stream);
    const uint64_t quad = p.first_quad + (uint64_t)tl * TILE_QUADS + threadIdx.x;
    const uint64_t j0 = quad * 4u;
    if (j0 >= end) continue;
    const Stream st = streams[s];
    const uint8_t* __restrict__ tx = text + (size_t)s * p.text_stride;
    const uint32_t n_on = 2u + p.n_preamble + 8u * st.text_len;
    float v[4];
    const double jd = (double)j0;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = signal_at(p, st, tx, n_on, jd + (double)i);
    if (st.sigma != 0.0f) {
      const Words w = philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), s, 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
      float z[4];
      box_muller(w.w[0], w.w[1], z[0], z[1]);
      box_muller(w.w[2], w.w[3], z[2], z[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += st.sigma * z[i];
    }
    // a lane at a chunk's edge owns samples outside the call: only a lane that lies wholly inside forms the vector's address
    T* const row = out + (size_t)s * p.stride;
    const bool whole = j0 >= p.first_sample && j0 + 4u <= end;
    T* const dst = row + (whole ? (size_t)(j0 - p.first_sample) : 0);
    if (whole && ((uintptr_t)dst & (sizeof(V) - 1)) == 0) {
      V o;
      o.x = Out<DT>::cvt(v[0]);
      o.y = Out<DT>::cvt(v[1]);
      o.z = Out<DT>::cvt(v[2]);
      o.w = Out<DT>::cvt(v[3]);
      *(V*)dst = o;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint64_t j = j0 + (uint64_t)i;
        if (j >= p.first_sample && j < end) row[(size_t)(j - p.first_sample)] = Out<DT>::cvt(v[i]);
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void words_kernel(uint64_t seed, uint64_t sid, uint64_t first_counter, uint64_t n_counters,
                                                        uint32_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n_counters; i += (uint64_t)gridDim.x * THREADS) {
    const uint64_t c = first_counter + i;
    const Words w = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), (uint32_t)sid, (uint32_t)(sid >> 32), (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * i + k] = w.w[k];
  }
}

}  // namespace

int launch_transmit(int dtype, unsigned grid, void* stream, const Params& p, const Stream* streams, const uint8_t* text, void* out) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(link_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, streams, text, out); break;
    case DT_I32: hipLaunchKernelGGL(link_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, streams, text, out); break;
    case DT_I16: hipLaunchKernelGGL(link_kernel<DT_I16>, dim3(grid), dim3(THREADS), 0, hs, p, streams, text, out); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_words(unsigned grid, void* stream, uint64_t seed, uint64_t sid, uint64_t first_counter, uint64_t n_counters, uint32_t* out) {
  hipLaunchKernelGGL(words_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, seed, sid, first_counter, n_counters, out);
  return (int)hipGetLastError();
}

}  // namespace uc_link_dev
