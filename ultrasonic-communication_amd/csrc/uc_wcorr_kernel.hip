// uc_wcorr_kernel.hip -- the band-weighted correlator's kernels (gfx950): the windowed cross-correlations of
// uc_track_kernel.hip with a real, even weight on every bin of a group's cross-spectrum, and with guard lags that are
// computed and not stored.  include/uchirp_wcorr.h states the definition; uchirp/wcorr.py holds its float64 model and an
// independent float32 evaluation.
//
// wcorr_kernel.  track_kernel's deal over the unit of uc_corr_unit.hpp: the work unit is (pair, window, group of GROUP
// segments), numbered window-major inside a pair; units are dealt statically, a contiguous range each, to the 2-wave
// workgroups of a persistent grid; a workgroup does a unit from its first load to its 2 L + 1 stored sums on its own (no
// atomics, a sum cannot depend on the grid); the next unit's first loads are in flight over the inverse transform.
// What is this kernel's own:
//   - the segments are those of L' = max_lag + guard: S = 2048 - 2 L', and b_s starts L' samples in front of a_s;
//   - between a unit's last segment and its inverse transform every bin of the cross-spectrum is multiplied by its weight
//     (corr_weight: sixteen packed multiplies a thread).  A thread's sixteen weights do not depend on the unit: they are
//     fetched once, in front of the unit loop, and stay in registers (the kernel spills nothing with them and keeps
//     track_kernel's workgroups per CU: tests/test_wcorr_cpu.py reads both off the code object);
//   - of the unit's 2 L' + 1 sums those with index guard .. guard + 2 L are stored (corr_finish_at).
// With weights of 1.0f and guard 0 every operation is track_kernel's (x * 1.0f is x), so the unit sums have its bits.
//
// wcorr_sum_kernel adds a (pair, window) row's unit sums in double, in ascending group order, one thread per (row, lag).
#include <hip/hip_runtime.h>

#include "uc_corr_unit.hpp"
#include "uc_wcorr.hpp"

namespace uc_wcorr_dev {
namespace {

using namespace uc;

static_assert(POINTS == kN && THREADS == kXfThreads && 2 * MAX_LAG + 1 <= kCorrMaxLags, "the unit of uc_corr_unit.hpp");
static_assert(BINS == kCorrWeightBins, "the staged weight table");

// one unit: its window and its segments (workgroup-uniform)
struct Unit {
  CorrWindow w;
  uint32_t seg0, seg1;
};

// (n_units < 2^32: the host refuses more)
__device__ __forceinline__ Unit unit_of(const Params& p, const Pair* __restrict__ pairs, uint32_t unit) {
  const uint32_t pw = unit / p.n_groups;                              // pair * n_windows + window
  const uint32_t grp = unit - pw * p.n_groups;
  const uint32_t pair = pw / p.n_windows;
  const uint32_t w = pw - pair * p.n_windows;
  const Pair pr = pairs[pair];
  Unit u;
  u.w.ref = (const uint32_t*)p.in + pr.ref;
  u.w.mic = (const uint32_t*)p.in + pr.mic;
  u.w.first = p.first + (int64_t)w * p.hop;
  u.w.n = p.window_len;
  u.w.n_in = p.n_in;
  u.seg0 = grp * GROUP;
  u.seg1 = u.seg0 + GROUP < p.n_segments ? u.seg0 + GROUP : p.n_segments;   // > seg0
  return u;
}

template <int DT>
__global__ __launch_bounds__(THREADS, 2) void wcorr_kernel(const Params p, const Pair* __restrict__ pairs) {
  __shared__ __attribute__((aligned(16))) float lds[kCorrLdsFloats];
  const int j = threadIdx.x;
  CorrCtx c;
  corr_setup(c, lds, p.tw, j);

  const int lags = 2 * p.max_lag + 1, k0 = p.guard;
  const int L = p.max_lag + p.guard, S = POINTS - 2 * L;             // L': what the segments are cut for
  // this workgroup's units: one contiguous range of the numbering (track_kernel's deal)
  uint32_t unit = (uint32_t)((uint64_t)blockIdx.x * p.n_units / gridDim.x);
  const uint32_t end = (uint32_t)(((uint64_t)blockIdx.x + 1) * p.n_units / gridDim.x);
  if (unit >= end) return;                                           // (the host launches no more workgroups than units)
  v2f wv[8];
  corr_load_weights(p.weights, j, wv);
  Unit u = unit_of(p, pairs, unit);
  CorrRaw g;
  corr_load_segment(u.w, u.seg0, S, L, j, g);
  for (;;) {
    const uint32_t next = unit + 1;
    const bool more = next < end;                                    // workgroup-uniform
    v2f acc[2][8];
    corr_clear(acc);
    for (uint32_t seg = u.seg0; seg < u.seg1; ++seg)
      corr_segment<DT == DT_I32>(c, g, acc, [&]() __attribute__((always_inline)) {
        // a whole transform ahead: the unit's next segment, or across the unit boundary the next unit's first one
        const bool inside = seg + 1 < u.seg1;
        if (inside || more) {                                // (workgroup-uniform)
          const Unit ul = inside ? u : unit_of(p, pairs, next);
          corr_load_segment(ul.w, inside ? seg + 1 : ul.seg0, S, L, j, g);
        }
      });
    corr_weight(acc, wv);
    corr_finish_at(c, acc, p.part + unit * (uint64_t)lags, k0, lags);
    if (!more) break;
    unit = next;
    u = unit_of(p, pairs, next);
  }
}

// corr[row][k] = the row's unit sums of lag k - max_lag, added in double in ascending group order; row = pair * n_windows + window
__global__ __launch_bounds__(SUM_THREADS) void wcorr_sum_kernel(const Params p) {
  const uint64_t lags = 2 * (uint64_t)p.max_lag + 1;
  const uint64_t total = (uint64_t)p.n_pairs * p.n_windows * lags;
  for (uint64_t t = (uint64_t)blockIdx.x * SUM_THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * SUM_THREADS) {
    const uint64_t row = t / lags, k = t - row * lags;
    p.corr[row * p.corr_stride + k] = corr_unit_sum(p.part + row * p.n_groups * lags + k, p.n_groups, lags);
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wcorr_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wcorr_kernel<DT_I32>, THREADS, 0); break;
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
    case DT_F32: hipLaunchKernelGGL(wcorr_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    case DT_I32: hipLaunchKernelGGL(wcorr_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_sum(void* stream, const Params& p) {
  const uint64_t total = (uint64_t)p.n_pairs * p.n_windows * (2 * (uint64_t)p.max_lag + 1);
  uint64_t grid = (total + SUM_THREADS - 1) / SUM_THREADS;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(wcorr_sum_kernel, dim3((unsigned)grid), dim3(SUM_THREADS), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace uc_wcorr_dev
