// uc_retime_kernel.hip -- the retimer's kernels (gfx950): every output row is one microphone's row read along a line
// p(j) = j + delay + slope j through a 16-coefficient fractional-delay interpolator whose coefficients change from sample
// to sample.  include/uchirp_retime.h states the definition; uchirp/retime.py holds its float64 model.
//
// Shape: that of the array combiner (uc_array_kernel.hip).  A lane owns 4 consecutive outputs = one 16-byte store; a wave
// owns 256 consecutive outputs of ONE row; tiles of 1024 samples are dealt statically over (row, tile) to a persistent
// grid.  The row index comes from blockIdx and the tile counter alone, so the line's record (two 64-bit integers and the
// row offset) is wave-uniform and fetched by scalar loads.
//
// Positions: off = lead_fx + j drift_fx in exact 64-bit integers, per output; k = off >> 32 is the whole part of the
// position against j, the low 32 bits the fraction (8 bits of table row q, 24 bits of blend weight mu).  |drift_fx| <= 2^23,
// so over the 256 outputs of a wave off moves by less than 2^31: k takes at most two values, kmin and kmin + 1, and is
// monotonic.  kmin = min(k(first), k(last)) is wave-uniform (scalar arithmetic).
//
// Input window: the wave needs the samples j0 + kmin - 7 .. j0 + kmin + 255 + 1 + 8, 256 + 15 + 1 = 272 of them, at an
// offset that is in general no multiple of four samples.  It stages them through its own 272 floats of LDS exactly as the
// array combiner does: lane l loads samples 4 l .. 4 l + 3 of the window with ONE 16-byte load (lanes 0 .. 3 the last 16 with
// a second one), one ds_write_b128 puts them in place, five aligned ds_read_b128 fetch the lane's 20 values 4 l .. 4 l + 19:
// its four outputs need 4 l + e + (k - kmin) + t, e = 0 .. 3, t = 0 .. 15, all within them.  The region is private to the
// wave and one wave's LDS operations complete in order: a wave-level fence, no workgroup barrier.
//
// Coefficients: the table T[257][16] (16448 bytes) is copied into LDS once per workgroup, before the tile loop, behind
// the kernel's only workgroup barrier.  An output reads rows q and q + 1 (eight ds_read_b128, lanes with the same q read
// the same addresses: a broadcast), forms D = T[q + 1] - T[q] (the float subtraction of the definition) and blends
// c[t] = fmaf(mu, D[t], T[q][t]) on its way into the chain.  A lane keeps T[q] and D across its four outputs and fetches
// them again only where q changes: at a slope of 50 ppm q steps every 78 outputs, so about three lanes of a wave run the
// second fetch (the others are masked off, and a wave where no lane needs it branches over it); at 2^-9 every lane fetches
// for every output.  Both forms read the same table entries and do the same arithmetic: the same bits.
//
// Integer step: in a wave where k(first) == k(last) every output e of a lane reads x[e + t]; in the rare wave that holds a
// step (one in 1 / (256 |slope|)) an output with k = kmin + 1 reads x[e + 1 + t], picked per value under a wave-uniform
// branch.
//
// Edges: as in the array combiner.  A window inside the row is loaded without predicates from a scalar base; one that
// crosses an end is loaded sample by sample, and a lane whose sample lies outside forms no address and keeps +0.0f.
// Nothing outside the rows is ever read.  I32 words are cast with (float) on their way into LDS.
#include <hip/hip_runtime.h>

#include "uc_retime.hpp"

#pragma clang fp contract(off)

namespace uc_retime_dev {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4_any __attribute__((ext_vector_type(4), aligned(4)));   // a quad in a row: no alignment beyond a sample's

constexpr int READS = 5;                          // ds_read_b128 of a lane: its values 4 l .. 4 l + 19
constexpr int TAIL_LANES = (WINDOW - 256) / 4;    // lanes whose second quad lies inside the window: 4
constexpr int TABLE_QUADS = TABLE_ROWS * COEFS / 4;

// orders this wave's LDS operations for the compiler; the hardware completes one wave's LDS operations in order
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the raw words of the wave's window: samples rel + 4 lane .. + 3 of the row in g[0], and in lanes 0 .. 3
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

// rows q and q + 1 of the table in LDS: T[q] and D[q] = T[q + 1] - T[q]
__device__ __forceinline__ void fetch_rows(const f4* tab, uint32_t q, float cT[COEFS], float cD[COEFS]) {
#pragma unroll
  for (int r = 0; r < COEFS / 4; ++r) {
    const f4 a = tab[4 * q + r], b = tab[4 * q + 4 + r];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cT[4 * r + i] = a[i];
      cD[4 * r + i] = b[i] - a[i];
    }
  }
}

template <int DT>
__global__ __launch_bounds__(THREADS) void retime_kernel(const Params p, const Line* __restrict__ lines) {
  __shared__ f4 tab[TABLE_QUADS];
  __shared__ f4 lds[(THREADS / 64) * (WINDOW / 4)];
  for (int i = (int)threadIdx.x; i < TABLE_QUADS; i += THREADS) tab[i] = ((const f4*)p.table)[i];
  __syncthreads();                                                           // the only workgroup barrier: the table is in place
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63u);
  f4* const win4 = lds + wave * (WINDOW / 4);
  const uint32_t* __restrict__ in = (const uint32_t*)p.in;
  const uint64_t n_tiles = (uint64_t)p.n_lines * p.tiles_per_row;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t r = (uint32_t)(tile / p.tiles_per_row);
    const uint32_t tl = (uint32_t)(tile - (uint64_t)r * p.tiles_per_row);
    const int64_t i_wave = (int64_t)tl * TILE_SAMPLES + wave * WAVE_SAMPLES;   // from out_first
    if (i_wave >= p.n_out) continue;                                          // the whole wave lies behind the call's end
    const Line ln = lines[r];
    const int64_t j0 = p.out_first + i_wave;                                  // the wave's first output, absolute
    const int64_t k_first = (ln.lead_fx + j0 * ln.drift_fx) >> 32;
    const int64_t k_last = (ln.lead_fx + (j0 + (WAVE_SAMPLES - 1)) * ln.drift_fx) >> 32;
    const int64_t kmin = k_first < k_last ? k_first : k_last;
    const bool step = k_first != k_last;
    u4 g[2];
    load_window(p, in + ln.row, j0 - p.in_first + kmin - 7, lane, g);
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
    for (int rd = 0; rd < READS; ++rd) {
      const f4 v = win4[lane + rd];
      x[4 * rd] = v.x;
      x[4 * rd + 1] = v.y;
      x[4 * rd + 2] = v.z;
      x[4 * rd + 3] = v.w;
    }
    wave_fence();
    int64_t off = ln.lead_fx + (j0 + 4 * lane) * ln.drift_fx;                 // of the lane's first output
    float cT[COEFS], cD[COEFS];
    float y[4];
    uint32_t q_held = 0xFFFFFFFFu;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      uint32_t frac = (uint32_t)off;
      // the four outputs one after the other: this output's table row hangs on the previous output's value, through an empty
      // statement that the compiler cannot see through.  Left to itself it fetches the rows of all four outputs up front
      // (LDS reads may be hoisted over the branch) and keeps 240 registers; in turn they need 20 + 16 + 16 + 16 and a few.
      if (e > 0) asm volatile("" : "+v"(frac) : "v"(y[e - 1]));
      const uint32_t q = frac >> 24;
      const float mu = (float)(frac & 0xFFFFFFu) * 0x1p-24f;
      if (q != q_held) {                                                      // e = 0: every lane; later: lanes where q stepped
        fetch_rows(tab, q, cT, cD);
        q_held = q;
      }
      float xe[COEFS];
      if (step) {
        // a bit-field insert per value, not a select: the compiler turns a select of two array elements into one element at
        // a computed index, which costs a compare chain over the whole array
        const uint32_t up = (off >> 32) != kmin ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int t = 0; t < COEFS; ++t)
          xe[t] = __uint_as_float((__float_as_uint(x[e + 1 + t]) & up) | (__float_as_uint(x[e + t]) & ~up));
      } else {
#pragma unroll
        for (int t = 0; t < COEFS; ++t) xe[t] = x[e + t];
      }
      float a = __builtin_fmaf(mu, cD[0], cT[0]) * xe[0];
#pragma unroll
      for (int t = 1; t < COEFS; ++t) a = __builtin_fmaf(__builtin_fmaf(mu, cD[t], cT[t]), xe[t], a);
      y[e] = a;
      off += ln.drift_fx;
    }
    // a lane at the call's end owns samples outside it: only a lane that lies wholly inside forms the vector's address
    const int64_t i0 = i_wave + 4 * lane;
    float* const rowo = p.out + (size_t)r * p.out_stride;
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
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, retime_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, retime_kernel<DT_I32>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_rows(int dtype, unsigned grid, void* stream, const Params& p, const Line* lines) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(retime_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, lines); break;
    case DT_I32: hipLaunchKernelGGL(retime_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, lines); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_retime_dev
