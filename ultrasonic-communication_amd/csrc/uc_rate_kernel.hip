// uc_rate_kernel.hip -- the rate converter's kernel (gfx950): every output row is the input row at up / down times its
// rate, through a polyphase Kaiser-windowed sinc of `taps` input samples per output.  include/uchirp_rate.h states the
// definition; uchirp/rate.py holds its float64 model.
//
// What is shared: all rows of a call have the same sample numbers, so output m has the same newest input k, the same phase
// p and the same `taps` coefficients in every row.  A unit is (a block of 16 rows) x (a tile of up to 256 outputs); a lane
// owns ONE output sample m of the tile and carries it through all 16 rows: it fetches a coefficient once and uses it 16
// times, as 8 packed multiply-adds over row pairs.  Units are dealt statically to a persistent grid; no atomics.
//
// Positions: one 64-bit division per unit, m0 = a up + f0 for the tile's first output m0, gives its phase number f0 and,
// with 32-bit steps, its k0 and p0; a lane adds its own 32-bit step: t = p0 + lane * down (below 2^21), k = k0 + t div up.
//
// Coefficients: the table in device memory is the definition's C[p][j] by OUTPUT phase and transposed,
// D[j][f] = C[p(f)][j] with f = m mod up and p(f) = (f down + c) mod up.  Neighbouring lanes are neighbouring outputs, so a
// wave's load of tap j is 64 consecutive floats (two runs where f wraps), whereas C's rows of neighbouring outputs lie
// `down` rows apart.  The table of 44.1 kHz (3125 x 49 floats, 0.6 MB) stays in L2; every float of it is read once per unit.
//
// Input: the samples k0 - taps + 1 .. k(last output) of the unit's 16 rows, at most 504 per row (the host sizes the tile so
// that they fit: uc_rate.hpp), go to LDS as pairs of rows, {row 2 q, row 2 q + 1} in one 8-byte word, so that one
// ds_read_b64 feeds one packed multiply-add.  They come through buffer resources that cover exactly the samples of the
// window that exist: the range check returns 0 for a sample in front of a row, behind it, or in a row past n_rows, and the
// cast of 0 is +0.0f.  Nothing outside the rows is ever read.
//
// The chain: y = C[T - 1] * x[k - T + 1], then fmaf for j = T - 2 .. 0, per row, in this order: the definition's.
#include <hip/hip_runtime.h>

#include "uc_rate.hpp"

#pragma clang fp contract(off)

namespace uc_rate_dev {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int PAIRS = ROWS / 2;
constexpr int kRsrcFlags = 0x00020000;   // gfx9 raw buffer, 32-bit data format
constexpr int kNowhere = 0x7ffffff0;     // a byte offset beyond every window (a window has at most 2048 bytes)

template <int DT>
__device__ __forceinline__ float load_sample(__amdgpu_buffer_rsrc_t r, int voff) {
  if (DT == DT_I16) return (float)(int16_t)__builtin_amdgcn_raw_buffer_load_b16(r, voff, 0, 0);
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}

// Every LDS read is to stay ONE ds_read_b64 (256 B per clock and CU): fused into ds_read2_b64 or ds_read2st64_b64 the same
// bytes move at half that rate.  Two reads are fused when they share a base register and lie less than 256 elements, or a
// multiple of 64 elements, apart.  The pairs of one tap lie PAIR_STRIDE = 505 elements apart (more than 255, no multiple of
// 64); the taps of one pair are neighbours, so each tap's index passes through an empty statement that the compiler cannot
// see through and gets a base register of its own.
constexpr int PAIR_STRIDE = WINDOW + 1;
static_assert(PAIR_STRIDE > 255 && PAIR_STRIDE % 64 != 0, "reads of two pairs must not fuse");
__device__ __forceinline__ uint32_t tap_index(uint32_t i) {
  asm volatile("" : "+v"(i));
  return i;
}

template <int DT>
__global__ __launch_bounds__(THREADS) void rate_kernel(const Params p) {
  constexpr int ELEM = DT == DT_I16 ? 2 : 4;
  __shared__ f2 win[PAIRS * PAIR_STRIDE];
  const uint32_t tid = threadIdx.x;
  const char* const in = (const char*)p.in;
  // unit = row block * tiles_per_row + tile, dealt blockIdx.x, + gridDim.x, ...: kept as the pair, stepped without a division
  uint32_t rb = blockIdx.x / p.tiles_per_row, ot = blockIdx.x % p.tiles_per_row;
  const uint32_t step_rb = gridDim.x / p.tiles_per_row, step_ot = gridDim.x % p.tiles_per_row;   // tiles_per_row < 2^31
  for (; rb < p.row_blocks; rb += step_rb, ot += step_ot) {
    if (ot >= p.tiles_per_row) {
      ot -= p.tiles_per_row;
      if (++rb >= p.row_blocks) break;
    }
    const uint64_t row0 = (uint64_t)rb * ROWS;
    const int64_t i0 = (int64_t)ot * p.tile;                                   // the tile's first output, from out_first
    const int64_t rest = p.n_out - i0;
    const uint32_t n_here = rest < (int64_t)p.tile ? (uint32_t)rest : p.tile;   // >= 1
    // the unit's one 64-bit division: m0 = a up + f0, so pos0 = m0 down + c = a up down + (f0 down + c), and the bracket is
    // below 2^25
    const uint64_t m0 = (uint64_t)(p.out_first + i0);
    const uint64_t a = m0 / p.up;
    const uint32_t f0 = (uint32_t)(m0 - a * p.up);
    const uint32_t s0 = f0 * p.down + p.centre;
    const uint64_t k0 = a * p.down + s0 / p.up;
    const uint32_t p0 = s0 % p.up;
    // the window: input samples k_lo .. k_lo + w - 1, w <= WINDOW by the tile's size
    const uint32_t dk_last = (p0 + (n_here - 1) * p.down) / p.up;
    const int64_t k_lo = (int64_t)k0 - (int64_t)(p.taps - 1);
    uint32_t w = dk_last + p.taps;
    w = w < (uint32_t)WINDOW ? w : (uint32_t)WINDOW;
    // the part of it that the rows hold: [lo, lo + cnt)
    const int64_t in_end = p.in_first + p.n_in;
    const int64_t lo = k_lo > p.in_first ? k_lo : p.in_first;
    const int64_t hi = k_lo + w < in_end ? k_lo + w : in_end;
    const int cnt = hi > lo ? (int)(hi - lo) : 0;
    const int shift = cnt ? (int)(lo - k_lo) : 0;                              // window index of sample lo
    const uint64_t off = cnt ? (uint64_t)(lo - p.in_first) : 0;                // row element of sample lo
    // pair by pair (not unrolled: two resources in scalar registers at a time, not sixteen); at most two passes of idx
#pragma unroll 1
    for (int q = 0; q < PAIRS; ++q) {
      __amdgpu_buffer_rsrc_t rs[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint64_t row = row0 + 2 * q + h;
        const bool there = row < p.n_rows;
        const char* base = in + ((there ? row : 0) * p.in_stride + off) * ELEM;
        rs[h] = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, there ? cnt * ELEM : 0, kRsrcFlags);
      }
      for (uint32_t idx = tid; idx < w; idx += THREADS) {
        const int e = (int)idx - shift;
        const int voff = e < 0 ? kNowhere : e * ELEM;                          // whole in the vector operand: the range check looks at it
        f2 v;
        v.x = load_sample<DT>(rs[0], voff);
        v.y = load_sample<DT>(rs[1], voff);
        win[q * PAIR_STRIDE + idx] = v;
      }
    }
    __syncthreads();
    const bool live = tid < n_here;
    const uint32_t i = live ? tid : 0;                                         // an idle lane goes along with output 0
    const uint32_t dk = (p0 + i * p.down) / p.up;
    const uint32_t f = (f0 + i) % p.up;
    const uint32_t newest = dk + p.taps - 1;                                   // window index of the sample under tap 0
    const float* const tab = p.table + f;
    f2 y[PAIRS];
    {
      const int j = (int)p.taps - 1;
      const float c = tab[(size_t)j * p.up];
#pragma unroll
      for (int q = 0; q < PAIRS; ++q) {
        const f2 v = win[q * PAIR_STRIDE + tap_index(newest - (uint32_t)j)];
        y[q].x = c * v.x;
        y[q].y = c * v.y;
      }
    }
    // four taps at a time, the coefficients of the next four on their way while these are used (an index below 0 is
    // moved to 0: loaded, not used)
    int j = (int)p.taps - 2;
    float c[4], nx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u] = tab[(size_t)(j - u > 0 ? j - u : 0) * p.up];
    for (; j >= 3; j -= 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) nx[u] = tab[(size_t)(j - 4 - u > 0 ? j - 4 - u : 0) * p.up];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f2 cc = {c[u], c[u]};
        const uint32_t at = tap_index(newest - (uint32_t)(j - u));
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) y[q] = __builtin_elementwise_fma(cc, win[q * PAIR_STRIDE + at], y[q]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = nx[u];
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      if (j - u >= 0) {                                                        // (uniform)
        const f2 cc = {c[u], c[u]};
        const uint32_t at = tap_index(newest - (uint32_t)(j - u));
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) y[q] = __builtin_elementwise_fma(cc, win[q * PAIR_STRIDE + at], y[q]);
      }
    }
    if (live) {
      float* const o = p.out + (i0 + i);
#pragma unroll
      for (int q = 0; q < PAIRS; ++q) {
        if (row0 + 2 * q < p.n_rows) o[(row0 + 2 * q) * p.out_stride] = y[q].x;
        if (row0 + 2 * q + 1 < p.n_rows) o[(row0 + 2 * q + 1) * p.out_stride] = y[q].y;
      }
    }
    __syncthreads();                                                           // the window is read: the next unit may overwrite it
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, rate_kernel<DT_F32>, THREADS, 0); break;
    case DT_I16: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, rate_kernel<DT_I16>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_convert(int dtype, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(rate_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p); break;
    case DT_I16: hipLaunchKernelGGL(rate_kernel<DT_I16>, dim3(grid), dim3(THREADS), 0, hs, p); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_rate_dev
