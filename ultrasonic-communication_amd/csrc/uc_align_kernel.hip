// uc_align_kernel.hip -- the delay estimator's kernels (gfx950): cross-correlations of pairs of rows over a window of
// lags.  include/uchirp_align.h states the definition, the order of every sum included; uchirp/align.py holds its
// float64 model.
//
// Shape: that of the array kernel.  The work unit is (pair, segment of 4096 samples, block of 32 lags); units are dealt
// statically to the WAVES of a persistent grid, and a wave does a unit from its first product to its 32 stored sums on
// its own: no barrier, no atomics, and a sum cannot depend on the grid.
//
// One pass of a wave covers 256 consecutive samples of the segment.  A lane owns four consecutive samples j of the
// REFERENCE row: one 16-byte load (global loads need no alignment beyond the sample's), kept in registers.  Of the
// MICROPHONE row the wave needs the 256 + 35 samples from j0 + lag0 on, at an offset that is in general no multiple of
// four samples; it stages them through its own 292 floats of LDS as the array kernel does: lane l loads samples
// 4 l .. 4 l + 3 of the window with one 16-byte load (lanes 0 .. 8 the last 36 with a second one), writes them with one
// ds_write_b128, and reads its own values 4 l .. 4 l + 35 back with nine aligned ds_read_b128 -- consecutive lanes on
// consecutive 16-byte slots on both sides.  The region is private to the wave and one wave's LDS operations complete in
// order, so a wave-level fence (no instruction) separates writes from reads.  Then 4 x 32 fused multiply-adds feed the 32
// accumulators of the lane (one per lag): 128 multiply-adds for 10 LDS instructions and 2.1 global ones.  The next pass's
// loads are issued before the current pass's arithmetic.  The compiler packs the multiply-adds by itself (64 v_pk_fma_f32
// per pass: the lane's reference sample against two neighbouring window values) and keeps the window's values in both
// pairings for it, which takes the kernel to 152 vector registers: it is held to 3 waves per SIMD (168 registers; at 4
// the 128 would spill 19), and 16 independent packed chains per wave leave the vector unit no gaps to hide.
//
// Edges: whether a pass is whole (all 256 samples inside the segment) and whether the window lies inside the microphone
// row are wave-uniform.  A whole pass inside the row takes unpredicated loads from scalar bases and plain multiply-adds.
// Otherwise every sample is loaded on its own, and a lane whose sample lies outside forms no address and keeps +0.0f: a
// reference sample behind the segment's end multiplies as zero and leaves the (finite) sums as they are.  Nothing
// outside the rows is ever read.  I32 words are cast with (float): the reference's in registers, the microphone's on
// their way into LDS.
//
// End of a unit: the 64 chains of every lag are added as the tree of the header (partners 32, 16, 8, 4, 2, 1 lanes
// apart).  The tree is transposed as it goes: at distance 32 the lower lane keeps lags 0 .. 15 and the upper one lags
// 16 .. 31, each sends the half the other keeps, and so on, so that the 32 sums cost 16 + 8 + 4 + 2 + 1 + 1 = 32
// cross-lane moves instead of 192 and end up one per even lane, stored as 32 consecutive floats.  IEEE addition commutes,
// so both partners form the same value.
//
// sum_kernel adds a pair's unit sums in double, in ascending segment order, one thread per (pair, lag).
#include <hip/hip_runtime.h>

#include "uc_align.hpp"

#pragma clang fp contract(off)

namespace uc_align_dev {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4_any __attribute__((ext_vector_type(4), aligned(4)));   // a quad in a row: no alignment beyond a sample's

constexpr int READS = (LAGS + 4) / 4;              // ds_read_b128 of a lane: its values 4 l .. 4 l + 35
constexpr int TAIL_LANES = (WINDOW - 256) / 4;     // lanes whose second quad lies inside the window: 9

static_assert(WINDOW % 4 == 0 && READS * 4 == LAGS + 4 && 4 * 63 + 4 * READS <= WINDOW, "the window holds what the last lane reads");
static_assert(SEGMENT % WAVE_SAMPLES == 0 && LAGS == 32, "the reduction below is written for 32 lags");

// orders this wave's LDS operations for the compiler; the hardware completes one wave's LDS operations in order
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the raw words row[at + e], e = 0 .. 3; `inside` (wave-uniform): all of the wave's quads of this kind lie in [lo, hi);
// otherwise a word outside [lo, hi) forms no address and reads as 0 (+0.0f, and 0 as an integer word)
__device__ __forceinline__ u4 load_quad(const uint32_t* __restrict__ row, int64_t at, int64_t lo, int64_t hi, bool inside) {
  if (inside) return *(const u4_any*)(row + at);
  u4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t idx = at + e;
    const bool in = idx >= lo && idx < hi;
    v[e] = in ? row[in ? idx : lo] : 0u;
  }
  return v;
}

template <int DT>
__device__ __forceinline__ float as_sample(uint32_t w) {
  return DT == DT_I32 ? (float)(int32_t)w : __uint_as_float(w);
}

// what one pass needs from memory, as raw words
struct Raw {
  u4 ref;      // reference samples j0 + 4 lane + (0 .. 3)
  u4 mic[2];   // window samples 4 lane + (0 .. 3), and in lanes 0 .. 8 samples 256 + 4 lane + (0 .. 3)
};

// j0: the pass's first reference sample (row element); end: one past the segment's last; mb: the window's first sample
__device__ __forceinline__ void load_pass(const Params& p, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ mic, int64_t j0,
                                          int64_t end, int64_t mb, int lane, Raw& g) {
  const u4 zero = {0u, 0u, 0u, 0u};
  g.ref = load_quad(ref, j0 + 4 * lane, j0, end, j0 + WAVE_SAMPLES <= end);
  const bool inside = mb >= 0 && mb + WINDOW <= p.n_in;
  g.mic[0] = load_quad(mic, mb + 4 * lane, 0, p.n_in, inside);
  g.mic[1] = zero;
  if (lane < TAIL_LANES) g.mic[1] = load_quad(mic, mb + 256 + 4 * lane, 0, p.n_in, inside);
}

// a lane's 4 x 32 multiply-adds of one pass; a sample the lane does not own has r[e] = +0.0f and adds a zero
__device__ __forceinline__ void accumulate(float (&acc)[LAGS], const float (&r)[4], const float (&x)[4 * READS]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < LAGS; ++k) acc[k] = __builtin_fmaf(r[e], x[e + k], acc[k]);
}

template <int DT>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void align_kernel(const Params p, const Pair* __restrict__ pairs) {
  __shared__ f4 lds[(THREADS / 64) * (WINDOW / 4)];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63u);
  f4* const win4 = lds + wave * (WINDOW / 4);
  const uint32_t* __restrict__ in = (const uint32_t*)p.in;
  const uint64_t n_waves = (uint64_t)gridDim.x * (THREADS / 64);
  for (uint64_t unit = (uint64_t)blockIdx.x * (THREADS / 64) + (uint64_t)wave; unit < p.n_units; unit += n_waves) {
    const uint64_t ps = unit / p.n_blocks;                    // pair * n_segments + segment
    const uint32_t block = (uint32_t)(unit - ps * p.n_blocks);
    const uint32_t pair = (uint32_t)(ps / p.n_segments);
    const uint32_t seg = (uint32_t)(ps - (uint64_t)pair * p.n_segments);
    const Pair pr = pairs[pair];
    const uint32_t* __restrict__ ref = in + pr.ref;
    const uint32_t* __restrict__ mic = in + pr.mic;
    const int64_t i0 = (int64_t)seg * SEGMENT;                                  // from first
    const int64_t len = p.n - i0 < SEGMENT ? p.n - i0 : (int64_t)SEGMENT;       // >= 1
    const int64_t j0 = p.first + i0, end = j0 + len;                            // row elements
    const int64_t lag0 = (int64_t)block * LAGS - p.max_lag;
    const int passes = (int)((len + WAVE_SAMPLES - 1) / WAVE_SAMPLES);
    float acc[LAGS];
#pragma unroll
    for (int k = 0; k < LAGS; ++k) acc[k] = 0.0f;
    Raw g;
    load_pass(p, ref, mic, j0, end, j0 + lag0, lane, g);
    for (int w = 0; w < passes; ++w) {
      const int64_t jw = j0 + (int64_t)w * WAVE_SAMPLES;
      {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = as_sample<DT>(g.mic[0][e]);
        win4[lane] = v;
        if (lane < TAIL_LANES) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = as_sample<DT>(g.mic[1][e]);
          win4[64 + lane] = v;
        }
      }
      float r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = as_sample<DT>(g.ref[e]);
      wave_fence();
      float x[4 * READS];
#pragma unroll
      for (int q = 0; q < READS; ++q) {
        const f4 v = win4[lane + q];
        x[4 * q] = v.x;
        x[4 * q + 1] = v.y;
        x[4 * q + 2] = v.z;
        x[4 * q + 3] = v.w;
      }
      wave_fence();
      if (w + 1 < passes) load_pass(p, ref, mic, jw + WAVE_SAMPLES, end, jw + WAVE_SAMPLES + lag0, lane, g);
      accumulate(acc, r, x);
    }
    // the tree of the header, transposed as it goes: after the step at distance d a lane keeps the half of its sums that
    // its bit d selects; after the step at distance 2 lane l holds the sum of lag (l >> 1), after distance 1 both of a pair
#pragma unroll
    for (int h = LAGS / 2, d = 32; h >= 1; h >>= 1, d >>= 1) {
      // (selects written as bit masks: a select between two elements of acc would become an indexed access to the array)
      const uint32_t upper = 0u - (((uint32_t)lane / (uint32_t)d) & 1u);
#pragma unroll
      for (int k = 0; k < h; ++k) {
        const uint32_t lo = __float_as_uint(acc[k]), hi = __float_as_uint(acc[k + h]);
        const float send = __uint_as_float((lo & upper) | (hi & ~upper));
        const float keep = __uint_as_float((hi & upper) | (lo & ~upper));
        acc[k] = keep + __shfl_xor(send, d, 64);
      }
    }
    const float total = acc[0] + __shfl_xor(acc[0], 1, 64);
    if ((lane & 1) == 0) p.part[unit * LAGS + (uint64_t)(lane >> 1)] = total;
  }
}

// corr[pair][k] = the pair's unit sums of lag k - max_lag, added in double in ascending segment order
__global__ __launch_bounds__(THREADS) void align_sum_kernel(const Params p) {
  const uint64_t lags = 2 * (uint64_t)p.max_lag + 1;
  const uint64_t total = (uint64_t)p.n_pairs * lags;
  const uint64_t row = (uint64_t)p.n_blocks * LAGS;             // floats of one (pair, segment)
  for (uint64_t t = (uint64_t)blockIdx.x * THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * THREADS) {
    const uint64_t pair = t / lags, k = t - pair * lags;
    const float* __restrict__ src = p.part + pair * p.n_segments * row + k;
    double sum = 0.0;
    for (uint32_t s = 0; s < p.n_segments; ++s) sum += (double)src[(uint64_t)s * row];
    p.corr[pair * p.corr_stride + k] = sum;
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, align_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, align_kernel<DT_I32>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_correlate(int dtype, unsigned grid, void* stream, const Params& p, const Pair* pairs) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(align_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    case DT_I32: hipLaunchKernelGGL(align_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_sum(void* stream, const Params& p) {
  const uint64_t total = (uint64_t)p.n_pairs * (2 * (uint64_t)p.max_lag + 1);
  uint64_t grid = (total + THREADS - 1) / THREADS;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(align_sum_kernel, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace uc_align_dev
