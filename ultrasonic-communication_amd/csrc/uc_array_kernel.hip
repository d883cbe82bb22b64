// uc_array_kernel.hip -- the array combiner's kernels (gfx950): delay-and-sum beams.  Every beam is a sum of up to 32
// taps; a tap is one microphone's row passed through a 16-coefficient fractional-delay interpolator (a Kaiser-windowed
// sinc whose coefficients the host computed) at an integer shift.  include/uchirp_array.h states the definition;
// uchirp/array.py holds its float64 model.
//
// Shape: that of the link and scene kernels.  A lane owns 4 consecutive outputs = one 16-byte store; a wave owns 256
// consecutive outputs of ONE beam; tiles of 1024 samples are dealt statically over (beam, tile) to a persistent grid.
//
// Tap records: the beam index comes from blockIdx and the tile counter alone, so the beam's record, its tap records
// (shift, row offset, 16 coefficients) and the loop's trip count are the same in every lane: they are read through
// const __restrict__ pointers with wave-uniform indices, which the compiler turns into scalar loads.  The 16
// coefficients stay in scalar registers and enter the 64 multiply-adds of a lane and tap as scalar operands.
//
// Input window: for one tap a wave needs the 256 + 15 input samples from j0 + shift on, at an offset that is in general
// not a multiple of four samples, so a lane's 19 values are no aligned vectors in global memory.  The wave stages the
// window through its own 272 floats of LDS: lane l loads the four samples 4 l .. 4 l + 3 of the window with ONE 16-byte
// load (global loads need no alignment beyond the sample's; lanes 0 .. 3 load the last 16 samples with a second one) and
// puts them where they belong with one ds_write_b128; then every lane reads its values 4 l .. 4 l + 19 with five aligned
// ds_read_b128 -- consecutive lanes on consecutive 16-byte slots on both sides, no bank conflict.  (A first form took the
// window as five dword loads and five ds_write_b32 per lane; it ran at 0.29 of the read probe's rate: DESIGN.md section 11.)
// The region is private to the wave and LDS operations of one wave complete in order, so a wave-level fence (no
// instruction, it only pins the compiler's order) is all that separates the writes from the reads and the reads from the
// next tap's writes: no workgroup barrier.  Global memory is asked for 272 / 256 = 1.06 values per tap-sample (the 16
// shared with the neighbouring wave come from the cache) where per-lane loads would ask for 4.75.  The next tap's loads are
// issued before the current tap's multiply-adds.  The kernel is held to 8 waves per SIMD (64 vector registers): the edge
// form's predicated loads would otherwise take the allocation to 72 and the occupancy to 7.
//
// Edges: the window's position against [in_first, in_first + n_in) is wave-uniform.  A window inside the row is loaded
// without predicates from a scalar base; one that crosses an end is loaded sample by sample, and a lane whose sample
// lies outside forms no address and keeps +0.0f.  Nothing outside the rows is ever read.  I32 words are cast with (float)
// on their way into LDS.
//
// Sum: the accumulators start at -0.0f, the one float that leaves every a_0 unchanged under y + a_0 (signs of zeros
// included); every a_k is a chain of one product and 15 fused multiply-adds, written out, and is added with one rounding.
#include <hip/hip_runtime.h>

#include "uc_array.hpp"

#pragma clang fp contract(off)

namespace uc_array_dev {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4_any __attribute__((ext_vector_type(4), aligned(4)));   // a quad in a row: no alignment beyond a sample's

constexpr int READS = 5;                          // ds_read_b128 of a lane: its values 4 l .. 4 l + 19
constexpr int TAIL_LANES = (WINDOW - 256) / 4;    // lanes whose second quad lies inside the window: 4

// orders this wave's LDS operations for the compiler; the hardware completes one wave's LDS operations in order
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the raw words of the wave's window for one tap: samples rel + 4 lane .. + 3 of the row in g[0], and in lanes 0 .. 3
// samples rel + 256 + 4 lane .. + 3 in g[1]
__device__ __forceinline__ void load_window(const Params& p, const uint32_t* __restrict__ row, int64_t rel, int lane, u4 g[2]) {
  const u4 zero = {0u, 0u, 0u, 0u};
  g[1] = zero;
  if (rel >= 0 && rel + WINDOW <= p.n_in) {
    const uint32_t* __restrict__ src = row + rel;
    g[0] = *(const u4_any*)(src + 4 * lane);
    if (lane < TAIL_LANES) g[1] = *(const u4_any*)(src + 256 + 4 * lane);
  } else {
    // the window crosses an end of the row: every sample on its own, a lane whose sample lies outside forms no address
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      u4 v = zero;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t idx = rel + (int64_t)(256 * q + 4 * lane + e);
        const bool in = idx >= 0 && idx < p.n_in && (q == 0 || lane < TAIL_LANES);
        v[e] = in ? row[in ? idx : 0] : 0u;
      }
      g[q] = v;
    }
  }
}

template <int DT>
__device__ __forceinline__ float as_sample(uint32_t w) {
  return DT == DT_I32 ? (float)(int32_t)w : __uint_as_float(w);
}

template <int DT>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void array_kernel(const Params p, const Beam* __restrict__ beams, const Tap* __restrict__ taps) {
  __shared__ f4 lds[(THREADS / 64) * (WINDOW / 4)];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63u);
  f4* const win4 = lds + wave * (WINDOW / 4);
  const uint32_t* __restrict__ in = (const uint32_t*)p.in;
  const uint64_t n_tiles = (uint64_t)p.n_beams * p.tiles_per_beam;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t b = (uint32_t)(tile / p.tiles_per_beam);
    const uint32_t tl = (uint32_t)(tile - (uint64_t)b * p.tiles_per_beam);
    const int64_t i_wave = (int64_t)tl * TILE_SAMPLES + wave * WAVE_SAMPLES;   // from out_first
    if (i_wave >= p.n_out) continue;                                          // the whole wave lies behind the call's end
    const Beam bm = beams[b];
    const int64_t base = p.out_first + i_wave - p.in_first;                   // the wave's first output, in row elements
    u4 g[2];
    {
      const Tap& t0 = taps[bm.first_tap];
      load_window(p, in + t0.row, base + t0.shift, lane, g);
    }
    float y[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
    for (uint32_t k = 0; k < bm.n_taps; ++k) {
      const Tap t = taps[bm.first_tap + k];
      {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = as_sample<DT>(g[0][e]);
        win4[lane] = v;
        if (lane < TAIL_LANES) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = as_sample<DT>(g[1][e]);
          win4[64 + lane] = v;
        }
      }
      wave_fence();
      float x[4 * READS];
#pragma unroll
      for (int r = 0; r < READS; ++r) {
        const f4 v = win4[lane + r];
        x[4 * r] = v.x;
        x[4 * r + 1] = v.y;
        x[4 * r + 2] = v.z;
        x[4 * r + 3] = v.w;
      }
      wave_fence();
      if (k + 1 < bm.n_taps) {
        const Tap& tn = taps[bm.first_tap + k + 1];
        load_window(p, in + tn.row, base + tn.shift, lane, g);
      }
      float a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = t.c[0] * x[i];
#pragma unroll
      for (int c = 1; c < COEFS; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = __builtin_fmaf(t.c[c], x[i + c], a[i]);
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = y[i] + a[i];
    }
    // a lane at the call's end owns samples outside it: only a lane that lies wholly inside forms the vector's address
    const int64_t i0 = i_wave + 4 * lane;
    float* const rowo = p.out + (size_t)b * p.out_stride;
    const bool whole = i0 + 4 <= p.n_out;
    float* const dst = rowo + (whole ? i0 : 0);
    if (whole && ((uintptr_t)dst & 15u) == 0) {
      f4 o;
      o.x = y[0];
      o.y = y[1];
      o.z = y[2];
      o.w = y[3];
      *(f4*)dst = o;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i0 + i < p.n_out) rowo[i0 + i] = y[i];
    }
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, array_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, array_kernel<DT_I32>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_combine(int dtype, unsigned grid, void* stream, const Params& p, const Beam* beams, const Tap* taps) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(array_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, beams, taps); break;
    case DT_I32: hipLaunchKernelGGL(array_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, beams, taps); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_array_dev
