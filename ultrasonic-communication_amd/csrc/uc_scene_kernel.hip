// uc_scene_kernel.hip -- the scene renderer's kernels (gfx950): what n_mics microphones receive over up to 16 paths
// each -- arrivals of any of the scene's transmissions, each with its own gain, lead and clock offset -- summed and
// given noise once per microphone, in one pass into the receiver's input buffer (include/uchirp_scene.h states the
// definition; uchirp/scene.py holds its float64 model).
//
// Shape: the link kernel's (uc_link_kernel.hip).  One lane owns one Philox counter = four consecutive samples = one
// 16-byte store; a wave owns 256 consecutive samples of ONE microphone; tiles of 1024 samples are dealt statically over
// (microphone, tile) to a persistent grid.  No LDS, no barrier, no atomics.
//
// Path loop: the microphone index comes from blockIdx and the tile counter alone, so the microphone's record, its path
// records (rate, t0, origin, amp, n_on, tx: derived on the host) and the loop's trip count are the same in every lane: they
// are read through const __restrict__ pointers with wave-uniform indices, which the compiler turns into scalar loads
// into scalar registers.  The vector side carries four accumulators next to the live set of the link kernel's signal_at.
//
// Silent paths: a short message sounds over a few dozen tiles of a long recording.  symbol_at(frame_time(j)) is
// monotone in j, every rounding included (an exact integer difference with a constant, its conversion to double, the sum
// with the place in the quad, one fma with two constants, a sum with a constant, a product with a positive constant and floor are each monotone: the comment
// at frame_time() gives the steps), so if the symbol index at the tile's first
// and at its last sample lie on the same silent side of the frame, signal_at returns +0.0f at every sample between them.
// The proof needs the skip check and signal_at to evaluate ONE function: both call frame_time() and symbol_at() of
// uc_link_dev.hpp and nothing else, and frame_time() writes its one fma out, so both sites get the same rounding; an
// edit that computes a time any other way at one site breaks the proof, and the chunking and model tests of
// tests/test_gpu_scene.py and tests/test_gpu_far.py (a path long over, one not yet begun, far from sample 0) are what
// would show it.  The fmax / fmin form also covers a negative rate.
// Such a path is not evaluated; +0.0f is added in its place, so the bits are those of the definition.
//
// Sum: the accumulators start at -0.0f, the one float that x + acc leaves every x unchanged for (the signs of zeros
// included): the first path's value is taken as it is.  The additions are kept apart from the product inside signal_at
// (no fused multiply-add): every path's value is rounded to float before it is added, as the definition has it.
//
// Noise: fma(sigma, z, sum), written out.  The link kernel writes `v += sigma * z` and leaves the form to the compiler's
// contraction, which makes exactly this of it (its v is a select between 0 and amp * sin, so the product of the signal
// cannot be the fused one); the one-path identity with uc_link_transmit rests on that and tests/test_gpu_scene.py holds
// it.  (The link kernels' machine code was compared with an earlier build's once, when this file was written; no test holds
// such a comparison, and the one-path identity is the check of the two forms.)
#include <hip/hip_runtime.h>

#include "uc_link_dev.hpp"
#include "uc_scene.hpp"

namespace uc_scene_dev {
namespace {

using namespace uc_link_dev;

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <int DT>
__global__ __launch_bounds__(THREADS) void scene_kernel(const Params p, const Mic* __restrict__ mics, const Path* __restrict__ paths,
                                                        const uint8_t* __restrict__ text, void* __restrict__ out_v) {
  using T = typename Out<DT>::T;
  using V = typename Out<DT>::V;
  T* __restrict__ out = (T*)out_v;
  const uint64_t n_tiles = (uint64_t)p.n_streams * p.tiles_per_stream;
  const uint64_t end = p.first_sample + p.n_samples;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t m = (uint32_t)(tile / p.tiles_per_stream);
    const uint32_t tl = (uint32_t)(tile - (uint64_t)m * p.tiles_per_stream);
    const uint64_t tile_quad = p.first_quad + (uint64_t)tl * TILE_QUADS;
    const uint64_t quad = tile_quad + threadIdx.x;
    const uint64_t j0 = quad * 4u;
    if (j0 >= end) continue;
    const Mic mc = mics[m];
    // the tile's first and last sample (of the whole workgroup: uniform)
    const uint64_t jt0 = tile_quad * 4u, jt1 = jt0 + (uint64_t)(4 * TILE_QUADS - 4);   // its first and its last quad
    const float start = mc.n_paths ? -0.0f : 0.0f;
    float v[4] = {start, start, start, start};
    for (uint32_t k = 0; k < mc.n_paths; ++k) {
      const Path pt = paths[mc.first_path + k];
      const double qa = symbol_at(p, frame_time(pt, quad_distance(pt, jt0), 0)), qb = symbol_at(p, frame_time(pt, quad_distance(pt, jt1), 3));
      if (fmax(qa, qb) < 1.0 || fmin(qa, qb) >= (double)pt.n_on) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = add_rn(v[i], 0.0f);
        continue;
      }
      const uint8_t* __restrict__ tx = text + (size_t)pt.tx * p.text_stride;
      const double d0 = quad_distance(pt, j0);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = add_rn(v[i], signal_at(p, pt, tx, pt.n_on, d0, i));
    }
    if (mc.sigma != 0.0f) {
      const Words w = philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), m, 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
      float z[4];
      box_muller(w.w[0], w.w[1], z[0], z[1]);
      box_muller(w.w[2], w.w[3], z[2], z[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = __fmaf_rn(mc.sigma, z[i], v[i]);
    }
    // a lane at a chunk's edge owns samples outside the call: only a lane that lies wholly inside forms the vector's address
    T* const row = out + (size_t)m * p.stride;
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

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scene_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scene_kernel<DT_I32>, THREADS, 0); break;
    case DT_I16: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scene_kernel<DT_I16>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_render(int dtype, unsigned grid, void* stream, const Params& p, const Mic* mics, const Path* paths, const uint8_t* text,
                  void* out) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(scene_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, mics, paths, text, out); break;
    case DT_I32: hipLaunchKernelGGL(scene_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, mics, paths, text, out); break;
    case DT_I16: hipLaunchKernelGGL(scene_kernel<DT_I16>, dim3(grid), dim3(THREADS), 0, hs, p, mics, paths, text, out); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_scene_dev
