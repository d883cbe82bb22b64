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
// Time: the seconds since a stream's frame began come from the integer distance of the sample to the stream's origin
// (frame_time() of uc_link_dev.hpp), so their error does not grow with the position in the recording.
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
#include "uc_link_dev.hpp"

namespace uc_link_dev {
namespace {

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
    const double d0 = quad_distance(st, j0);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = signal_at(p, st, tx, n_on, d0, i);
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
