// uc_link_dev.hpp -- device code that the link simulator's kernels (uc_link_kernel.hip) and the scene renderer's
// (uc_scene_kernel.hip) share: the generator, the transmitter's law and the output conversions.  Everything is
// force-inlined; a kernel file includes this after uc_link.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "uc_link.hpp"

namespace uc_link_dev {

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

// seconds since the frame began at absolute sample j = j0 + i (j0 the first sample of j's quad, a multiple of 4; i = 0 .. 3),
// and the (unclamped) index of the frame's symbol at that time.  ST: a record with rate, t0, origin and amp (Stream; the
// scene's Path).
// The time is taken from the INTEGER distance to the stream's origin, the sample nearest to the frame's beginning
// (frame_origin() of uc_link_host.hpp): j0 - origin is exact in int64, its double and the sum with i are exact while the
// distance is below 2^53 - 3, and t0 is under a sample, so the one rounding of the fma is 2^-53 of a time inside the frame
// wherever in a recording the frame lies.  (The form j * rate - lead_s that stood here cancelled two times of size j / fs_out:
// 10 ulp of the signal at j = 2^33, 800 at 2^40.)  The conversion is taken once per quad (quad_distance) because an int64 ->
// double conversion costs several double-precision instructions and a lane owns the quad's four samples; the quad belongs to
// the absolute sample grid, not to the call, so the time stays a function of j alone.
// Both functions are monotone in j, rounding included, which is what lets the scene kernel decide from a tile's first
// and last sample that a path is silent over all of it.  The steps: a = j0 - origin is exact (j < 2^53, |origin| <= 2^53, so
// |a| < 2^54); D(j) = RN(RN(a) + i) is monotone inside a quad (RN is) and from a quad's last sample to the next quad's first:
// |a| < 2^54 leaves RN(a) <= a + 1, so RN(a) + 3 <= a + 4 and RN(RN(a) + 3) <= RN(a + 4); d -> d * rate + t0 is monotone
// in exact arithmetic (either way, by the sign of rate) and the fma rounds it once; symbol_at adds a constant, multiplies by
// a positive constant and takes the floor.
// Every caller must take its times from these functions and from nothing else (the tile's last sample as its quad's
// i = 3): the fma is written out, so every site gets the same roundings whatever the contraction setting.
template <class ST>
__device__ __forceinline__ double quad_distance(const ST& st, uint64_t j0) {
  return (double)((int64_t)j0 - st.origin);
}
template <class ST>
__device__ __forceinline__ double frame_time(const ST& st, double d0, int i) {
  return fma(d0 + (double)i, st.rate, st.t0);
}
__device__ __forceinline__ double symbol_at(const Params& p, double tt) { return floor((tt + 1e-10) * p.inv_sym_dur); }

// the transmitter's law at sample i of the quad whose first sample lies d0 = quad_distance() from the stream's origin
// (0 in silence and outside the frame)
template <class ST>
__device__ __forceinline__ float signal_at(const Params& p, const ST& st, const uint8_t* __restrict__ text, uint32_t n_on,
                                           double d0, int i) {
  const double tt = frame_time(st, d0, i);
  const double q = symbol_at(p, tt);
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

}  // namespace uc_link_dev
