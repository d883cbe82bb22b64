// uc_scan_kernel.hip -- the beam scanner's kernels (gfx950): the power of every steered beam per window.  A beam sample is
// the array combiner's (up to 32 taps, each one microphone's row through 16 coefficients at an integer shift), a power is the
// sum of its squares over a window in the order include/uchirp_scan.h states; uchirp/scan.py holds the float64 model and
// uc_scan.hpp the arithmetic itself, shared with uc_scan_power_row.
//
// The work is n_arrays x n_windows x n_beams x window_len x n_taps x 16 multiply-adds over an input of only n_taps rows per
// array: thousands of beams read the same few rows.  So the rows are staged ONCE per workgroup and step, and many beams run
// against that image.
//
// Mapping.  A work unit is (array, window, group of 16 beams); units are dealt blockIdx.x, + gridDim.x, ...  A workgroup is
// 4 waves and a wave carries 4 beams of the group through the window side by side.  A step is 256 consecutive samples: a lane
// holds 4 of them, which is exactly one chain of the definition, so a beam's chain sum is ONE register per lane, kept across
// the 16 steps of a segment; at the segment's end the 64 chains are added by the cross-lane tree and the sum is added, as a
// double, to the beam's total.  One wave walks a (beam, window)'s segments in order: no scratch, no finishing pass.
//
// Staging.  Per step the workgroup writes, for every tap k, the IMAGE = 256 + 64 + 24 floats of its row from
// base + lo[k] on into LDS, already cast; samples outside the row are written as +0.0f (such a thread reads element 0 of the row and drops it: nothing outside the rows is read).  lo[k] is
// chosen by the host so that [lo[k], lo[k] + 64] holds the shifts of as many beams as possible.  32 taps are 43 KiB: three
// workgroups (12 waves) a CU; the build for up to 8 taps takes 10.75 KiB and is held by its registers, not by LDS.  The image
// is shared by the 16 beams of the group: 344 loads per tap and step against 16 x 256 x 16 multiply-adds.
//
// A beam's read.  The shift within the image, s = shift - lo[k], is wave-uniform but in general no multiple of four, so a
// lane reads the six ALIGNED quads that hold its 19 values (consecutive lanes on consecutive 16-byte slots: no bank
// conflict) and the case of s & 3 hands the right 19 registers to the multiply-adds (the compiler keeps one copy of them
// and moves the operands: DESIGN.md section 22 has what that costs).  The sixteen
// coefficients are wave-uniform: the beam index comes from blockIdx and the wave number alone, q is read through a uniform
// index, and the table row q & 255 arrives by scalar loads and feeds the multiply-adds as scalar operands.
//
// Direct path.  A beam with a shift outside some tap's [lo, lo + 64] (a set may hold a delay of 5000 samples next to delays
// of 3) is marked by the host.  For such a beam the wave fills a window of its own (280 floats of LDS per wave) from the row
// at the beam's shift, tap by tap, with the image's rule for samples outside the row, and reads its quads from there at
// offset 0.  The window is private to the wave and one wave's LDS operations complete in order, so a wave-level fence (no
// instruction) separates its writes from its reads.  The multiply-adds are the same instructions on both paths: same bits.
//
// Edges.  A lane's sample beyond the window's end is computed and not added.  Powers leave by one 8-byte vector store of
// lane 0, records by one 16-byte vector store.
#include <hip/hip_runtime.h>

#include "uc_scan.hpp"

namespace uc_scan_dev {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int QUADS = IMAGE / 4;         // 86
constexpr int READS = 6;                 // aligned quads that hold a lane's 19 values at any offset 0 .. 3

constexpr int OWN_QUADS = 64 + READS;    // a wave's own window on the direct path: 280 floats (271 are used)

// orders this wave's LDS operations for the compiler; the hardware completes one wave's LDS operations in order
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static_assert(IMAGE % 4 == 0 && (SPREAD / 4 + 63 + READS) * 4 <= IMAGE, "the last lane's last quad lies inside the image");

// the four samples of a lane for one tap: x[O + i .. O + i + 15], i = 0 .. 3
template <int O>
__device__ __forceinline__ void tap_quad(const float* c, const float* x, float a[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = tap_sample(c, x + O + i);
}

template <int DT, int CAP>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(CAP == SMALL_TAPS ? 4 : 3, CAP == SMALL_TAPS ? 4 : 3))) void scan_kernel(const Params p) {
  __shared__ f4 image[CAP * QUADS];
  __shared__ f4 own[WAVES * OWN_QUADS];                          // a wave's own window of one tap: the direct path
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t* __restrict__ in = (const uint32_t*)p.in;
  const uint32_t n_taps = p.n_taps;
  const uint32_t units = p.n_arrays * p.n_windows * p.beam_groups;   // (the host holds the triples, hence this, below 2^32)
  for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const uint32_t u = (uint32_t)unit;
    const uint32_t aw = u / p.beam_groups;                       // a * n_windows + w
    const uint32_t g = u - aw * p.beam_groups;
    const uint32_t w = aw % p.n_windows;
    const uint64_t row0 = (uint64_t)(aw / p.n_windows) * p.array_rows;   // the array's first row
    const int64_t j0 = p.first + (int64_t)w * p.hop - p.in_first;   // the window's sample 0 at shift 0, in row elements
    const uint32_t b0 = g * GROUP + (uint32_t)wave * BEAMS_PER_WAVE;
    double total[BEAMS_PER_WAVE];
    int direct = 0;                                              // bit r: beam b0 + r takes the direct path
#pragma unroll
    for (int r = 0; r < BEAMS_PER_WAVE; ++r) {
      total[r] = 0.0;
      if (b0 + r < p.n_beams) direct |= __builtin_amdgcn_readfirstlane((int)p.direct[b0 + r]) << r;
    }
    for (int64_t seg = 0; seg < p.window_len; seg += SEGMENT) {
      float chain[BEAMS_PER_WAVE];
#pragma unroll
      for (int r = 0; r < BEAMS_PER_WAVE; ++r) chain[r] = 0.0f;
      const int64_t left = p.window_len - seg;
      const int steps = (int)((left < SEGMENT ? left + STEP - 1 : SEGMENT) / STEP);
      for (int st = 0; st < steps; ++st) {
        const int64_t i0 = seg + (int64_t)st * STEP;             // the step's first sample, from the window's first
        const int64_t base = j0 + i0;
        // ---- the image of every tap's row: elements base + lo[k] .. + IMAGE - 1, zeros outside the row
        __syncthreads();
        for (uint32_t k = 0; k < n_taps; ++k) {
          const uint32_t* __restrict__ row = in + (row0 + p.mic[k]) * p.in_stride;
          const int64_t e0 = base + p.lo[k];
          float* const dst = (float*)image + k * IMAGE;
          for (int t = (int)threadIdx.x; t < IMAGE; t += THREADS) {
            const int64_t idx = e0 + t;
            const bool inside = idx >= 0 && idx < p.n_in;
            const uint32_t raw = row[inside ? idx : 0];            // (element 0 exists: a lane outside reads it and drops it)
            dst[t] = inside ? sample_of<DT>(raw) : 0.0f;
          }
        }
        __syncthreads();
        // ---- this wave's beams
        // (not unrolled: one copy of the multiply-adds.  The beam in hand is always chain[0]; the four chains rotate by one
        // behind every beam, so that no register is indexed by r and after four beams every chain is where it was)
#pragma unroll 1
        for (int r = 0; r < BEAMS_PER_WAVE; ++r) {
          const uint32_t b = b0 + r;
          float ch = chain[0];
          if (b < p.n_beams) {                                   // (uniform)
          const int32_t* __restrict__ qb = p.q + (uint64_t)b * n_taps;
          float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          for (uint32_t k = 0; k < n_taps; ++k) {
            const int32_t q = __builtin_amdgcn_readfirstlane(qb[k]);
            const int32_t shift = (q >> 8) - 7;
            const float* __restrict__ ct = p.table + ((size_t)k * FRACTIONS + (size_t)(q & 255)) * COEFS;
            float c[COEFS];
#pragma unroll
            for (int t = 0; t < COEFS; ++t) c[t] = ct[t];
            // where the lane's 19 values lie: in the workgroup's image at the beam's shift, or -- direct path -- in the
            // wave's own window, which the wave fills from the row first (zeros outside it, as the image's)
            int s = shift - p.lo[k];                             // 0 .. SPREAD on the staged path
            const f4* src = image + k * QUADS;
            if ((direct >> r) & 1) {
              const uint32_t* __restrict__ row = in + (row0 + p.mic[k]) * p.in_stride;
              const int64_t rel = base + shift;                  // the row element under c[0] of the step's first sample
              float* const dst = (float*)(own + wave * OWN_QUADS);
              for (int t = lane; t < 4 * OWN_QUADS; t += 64) {
                const int64_t idx = rel + t;
                const bool inside = idx >= 0 && idx < p.n_in;
                const uint32_t raw = row[inside ? idx : 0];
                dst[t] = inside ? sample_of<DT>(raw) : 0.0f;
              }
              wave_fence();
              s = 0;
              src = own + wave * OWN_QUADS;
            }
            float x[4 * READS];
            float a[4];
            src += (s >> 2) + lane;
#pragma unroll
            for (int v = 0; v < READS; ++v) {
              const f4 quad = src[v];
              x[4 * v] = quad.x;
              x[4 * v + 1] = quad.y;
              x[4 * v + 2] = quad.z;
              x[4 * v + 3] = quad.w;
            }
            wave_fence();                                        // (the next tap's window is written behind these reads)
            switch (s & 3) {
              case 0: tap_quad<0>(c, x, a); break;
              case 1: tap_quad<1>(c, x, a); break;
              case 2: tap_quad<2>(c, x, a); break;
              default: tap_quad<3>(c, x, a); break;
            }
            if (k == 0) {
#pragma unroll
              for (int i = 0; i < 4; ++i) y[i] = a[i];
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) y[i] = y[i] + a[i];
            }
          }
          // the lane's four samples into its chain, ascending; a sample behind the window's end is left out
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (i0 + 4 * lane + i < p.window_len) ch = chain_add(ch, y[i]);
          }
#pragma unroll
          for (int m = 0; m + 1 < BEAMS_PER_WAVE; ++m) chain[m] = chain[m + 1];
          chain[BEAMS_PER_WAVE - 1] = ch;
        }
      }
      // ---- the segment's sum: chain l takes chain l + h, h = 32 .. 1; then into the beam's double
#pragma unroll
      for (int r = 0; r < BEAMS_PER_WAVE; ++r) {
        float v = chain[r];
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_down(v, (unsigned)h, 64);
        total[r] = total[r] + (double)v;                         // (lane 0 holds the sum; the others are not stored)
      }
    }
    if (lane == 0) {
      double* const dst = p.power + (uint64_t)aw * p.power_stride;
#pragma unroll
      for (int r = 0; r < BEAMS_PER_WAVE; ++r)
        if (b0 + r < p.n_beams) dst[b0 + r] = total[r];
    }
  }
}

__device__ __forceinline__ bool finite(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

// the strongest beam of every row of powers (the lowest index on a tie); one workgroup walks rows blockIdx.x, + gridDim.x
__global__ __launch_bounds__(THREADS) void best_kernel(const double* __restrict__ power, uint64_t power_stride, uint32_t n_beams, uint32_t rows, Best* __restrict__ best) {
  __shared__ double s_power[THREADS];
  __shared__ uint32_t s_beam[THREADS];
  __shared__ uint32_t s_bad[THREADS];
  const uint32_t t = threadIdx.x;
  for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const double* __restrict__ src = power + (uint64_t)row * power_stride;
    double mine = -1.0;                  // (a finite power is >= 0)
    uint32_t at = 0xFFFFFFFFu, bad = 0;
    for (uint32_t b = t; b < n_beams; b += THREADS) {
      const double v = src[b];
      if (!finite(v)) bad = 1;
      if (v > mine) {                    // ascending b: the lowest index of equal powers stays
        mine = v;
        at = b;
      }
    }
    __syncthreads();                     // (the last row's reads of the shared arrays)
    s_power[t] = mine;
    s_beam[t] = at;
    s_bad[t] = bad;
    __syncthreads();
    for (uint32_t h = THREADS / 2; h >= 1; h >>= 1) {
      if (t < h) {
        const double other = s_power[t + h];
        const uint32_t other_at = s_beam[t + h];
        if (other > s_power[t] || (other == s_power[t] && other_at < s_beam[t])) {
          s_power[t] = other;
          s_beam[t] = other_at;
        }
        s_bad[t] |= s_bad[t + h];
      }
      __syncthreads();
    }
    if (t == 0) {
      Best rec;
      rec.beam = s_bad[0] ? 0u : s_beam[0];
      rec.flags = s_bad[0] ? 1u : 0u;
      rec.power = s_bad[0] ? 0.0 : s_power[0];
      best[row] = rec;
    }
  }
}

}  // namespace

int resident_blocks_per_cu(int variant) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (variant) {
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scan_kernel<DT_I32, SMALL_TAPS>, THREADS, 0); break;
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scan_kernel<DT_F32, SMALL_TAPS>, THREADS, 0); break;
    case 2 | DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scan_kernel<DT_I32, MAX_TAPS>, THREADS, 0); break;
    case 2 | DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scan_kernel<DT_F32, MAX_TAPS>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_power(int dtype, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  const bool small = p.n_taps <= (uint32_t)SMALL_TAPS;
  switch (dtype) {
    case DT_F32:
      if (small)
        hipLaunchKernelGGL((scan_kernel<DT_F32, SMALL_TAPS>), dim3(grid), dim3(THREADS), 0, hs, p);
      else
        hipLaunchKernelGGL((scan_kernel<DT_F32, MAX_TAPS>), dim3(grid), dim3(THREADS), 0, hs, p);
      break;
    case DT_I32:
      if (small)
        hipLaunchKernelGGL((scan_kernel<DT_I32, SMALL_TAPS>), dim3(grid), dim3(THREADS), 0, hs, p);
      else
        hipLaunchKernelGGL((scan_kernel<DT_I32, MAX_TAPS>), dim3(grid), dim3(THREADS), 0, hs, p);
      break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_best(unsigned grid, void* stream, const double* power, uint64_t power_stride, uint32_t n_beams, uint32_t rows, Best* best) {
  hipLaunchKernelGGL(best_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, power, power_stride, n_beams, rows, best);
  return (int)hipGetLastError();
}

}  // namespace uc_scan_dev
