// uc_xcorr_kernel.hip -- the wide-lag correlator's kernels (gfx950): cross-correlations of pairs of rows out to +-512
// lags.  include/uchirp_xcorr.h states the definition; uchirp/xcorr.py holds its float64 model and an independent float32
// evaluation.  What a unit is and how it is computed -- the segments, the two transforms, the barriers, the edges -- is
// uc_corr_unit.hpp; this file holds the deal.
//
// Shape: that of compress_kernel.  The work unit is (pair, group of GROUP segments); units are dealt statically to the
// 2-wave workgroups of a persistent grid, and a workgroup does a unit from its first load to its 2 L + 1 stored sums on
// its own: no atomics, and a sum cannot depend on the grid.  Inside a unit the next segment's loads are issued a whole
// transform ahead; a unit's first segment is loaded where the unit starts.
//
// sum_kernel adds a pair's unit sums in double, in ascending group order, one thread per (pair, lag).
#include <hip/hip_runtime.h>

#include "uc_corr_unit.hpp"
#include "uc_xcorr.hpp"

namespace uc_xcorr_dev {
namespace {

using namespace uc;

static_assert(POINTS == kN && THREADS == kXfThreads && 2 * MAX_LAG + 1 <= kCorrMaxLags, "the unit of uc_corr_unit.hpp");

template <int DT>
__global__ __launch_bounds__(THREADS, 2) void xcorr_kernel(const Params p, const Pair* __restrict__ pairs) {
  __shared__ __attribute__((aligned(16))) float lds[kCorrLdsFloats];
  const int j = threadIdx.x;
  CorrCtx c;
  corr_setup(c, lds, p.tw, j);

  const int L = p.max_lag, S = POINTS - 2 * L, lags = 2 * L + 1;
  const uint32_t* __restrict__ in = (const uint32_t*)p.in;
  for (uint64_t unit = blockIdx.x; unit < p.n_units; unit += gridDim.x) {
    const uint32_t pair = (uint32_t)(unit / p.n_groups);
    const uint32_t grp = (uint32_t)(unit - (uint64_t)pair * p.n_groups);
    const Pair pr = pairs[pair];
    const CorrWindow w = {in + pr.ref, in + pr.mic, p.first, p.n, p.n_in};
    const uint32_t seg0 = grp * GROUP;
    const uint32_t seg1 = seg0 + GROUP < p.n_segments ? seg0 + GROUP : p.n_segments;   // > seg0
    v2f acc[2][8];
    corr_clear(acc);
    CorrRaw g;
    corr_load_segment(w, seg0, S, L, j, g);
    for (uint32_t seg = seg0; seg < seg1; ++seg)
      corr_segment<DT == DT_I32>(c, g, acc, [&]() __attribute__((always_inline)) {
        if (seg + 1 < seg1) corr_load_segment(w, seg + 1, S, L, j, g);
      });
    corr_finish(c, acc, p.part + unit * (uint64_t)lags, lags);
  }
}

// corr[pair][k] = the pair's unit sums of lag k - max_lag, added in double in ascending group order
__global__ __launch_bounds__(SUM_THREADS) void xcorr_sum_kernel(const Params p) {
  const uint64_t lags = 2 * (uint64_t)p.max_lag + 1;
  const uint64_t total = (uint64_t)p.n_pairs * lags;
  for (uint64_t t = (uint64_t)blockIdx.x * SUM_THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * SUM_THREADS) {
    const uint64_t pair = t / lags, k = t - pair * lags;
    p.corr[pair * p.corr_stride + k] = corr_unit_sum(p.part + pair * p.n_groups * lags + k, p.n_groups, lags);
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, xcorr_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, xcorr_kernel<DT_I32>, THREADS, 0); break;
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
    case DT_F32: hipLaunchKernelGGL(xcorr_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    case DT_I32: hipLaunchKernelGGL(xcorr_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_sum(void* stream, const Params& p) {
  const uint64_t total = (uint64_t)p.n_pairs * (2 * (uint64_t)p.max_lag + 1);
  uint64_t grid = (total + SUM_THREADS - 1) / SUM_THREADS;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(xcorr_sum_kernel, dim3((unsigned)grid), dim3(SUM_THREADS), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace uc_xcorr_dev
