// uc_track_kernel.hip -- the delay tracker's kernels (gfx950): the cross-correlations of uc_xcorr_kernel.hip over a series
// of windows of one recording, and the crest search that leaves one small record per (pair, window).
// include/uchirp_track.h states the definitions; uchirp/track.py holds their float64 models.
//
// track_kernel.  The work unit is (pair, window, group of GROUP segments), numbered window-major inside a pair so that
// units which read the same samples are neighbours; units are dealt statically, a contiguous range each, to the 2-wave
// workgroups of a persistent grid, and a workgroup does a unit from its first load to its 2 L + 1 stored sums on its own:
// no atomics, and a sum cannot depend on the grid.  A unit is the unit of uc_corr_unit.hpp, the code xcorr_kernel runs,
// over the window first' = first + w hop, n' = window_len: that is why a unit sum has the bits that kernel gives.
// What is this kernel's own:
//   - a unit carries its window's first sample;
//   - a window's last group is usually short (window_len = 8192 at L = 128 is 4 + 1 segments), so the units are of unequal
//     length and a workgroup's next unit starts often;
//   - the loads of the next unit's first segment are therefore issued where a segment's successor is loaded inside a
//     unit: before the arithmetic of the unit's last B transform.  They stay in flight over the inverse transform (whose
//     registers are the accumulators' and the za's, both dead by then).
//
// track_crest_kernel.  One wave per (pair, window).  The lanes stride over k: each adds the row's unit sums in double in
// ascending group order (corr_unit_sum, what xcorr_sum_kernel does), stores the double if corr is given and keeps it in
// LDS; the largest sample (the first one on a tie) and the test for values that are not finite ride along.  Then every
// lane walks its candidates and keeps its own best four by (h2 descending, k ascending) in registers; four rounds of a
// wave-wide butterfly pick the best remaining head, and the four winners are written in ascending k.  The order is total
// (a k belongs to one lane), so the result depends neither on the grid nor on which lane saw which k.
#include <hip/hip_runtime.h>

#include "uc_corr_unit.hpp"
#include "uc_track.hpp"

namespace uc_track_dev {
namespace {

using namespace uc;

static_assert(POINTS == kN && THREADS == kXfThreads && 2 * MAX_LAG + 1 <= kCorrMaxLags, "the unit of uc_corr_unit.hpp");
static_assert(sizeof(Slot) == 32 && sizeof(Crest) == 8 + 32 * SLOTS, "struct uc_track_crest");

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
__global__ __launch_bounds__(THREADS, 2) void track_kernel(const Params p, const Pair* __restrict__ pairs) {
  __shared__ __attribute__((aligned(16))) float lds[kCorrLdsFloats];
  const int j = threadIdx.x;
  CorrCtx c;
  corr_setup(c, lds, p.tw, j);

  const int L = p.max_lag, S = POINTS - 2 * L, lags = 2 * L + 1;
  // this workgroup's units: one contiguous range of the numbering, all ranges within one unit of the same length.  (Dealing
  // unit b, b + grid, ... instead puts every long group on the even workgroups and every short one on the odd ones wherever a
  // window has two groups and the grid is even: 1.6 times the time at the bench shape, profiles/r13_track.txt.)
  uint32_t unit = (uint32_t)((uint64_t)blockIdx.x * p.n_units / gridDim.x);
  const uint32_t end = (uint32_t)(((uint64_t)blockIdx.x + 1) * p.n_units / gridDim.x);
  if (unit >= end) return;                                           // (the host launches no more workgroups than units)
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
          // (the next unit is derived again behind this one: that is cheaper than keeping it)
          const Unit ul = inside ? u : unit_of(p, pairs, next);
          corr_load_segment(ul.w, inside ? seg + 1 : ul.seg0, S, L, j, g);
        }
      });
    corr_finish(c, acc, p.part + unit * (uint64_t)lags, lags);
    if (!more) break;
    unit = next;
    u = unit_of(p, pairs, next);
  }
}

// the selection height of include/uchirp_track.h: every operation rounded once, none contracted
__device__ __forceinline__ double selection_height(double lo, double mid, double hi) {
#pragma clang fp contract(off)
  const double c = __ddiv_rn(__dadd_rn(lo, hi), __dmul_rn(2.0, mid));
  double h2 = __dmul_rn(mid, mid);
  if (c > -1.0 && c < 1.0) {
    const double s = __dsqrt_rn(__dmul_rn(__dsub_rn(1.0, c), __dadd_rn(1.0, c)));
    const double q = __ddiv_rn(__dsub_rn(hi, lo), __dmul_rn(2.0, s));
    h2 = __dadd_rn(h2, __dmul_rn(q, q));
  }
  return h2;
}

// (h, k) beats (bh, bk): the greater height, the smaller k on equal heights; an empty entry (k < 0) beats nothing
__device__ __forceinline__ bool beats(double h, int k, double bh, int bk) {
  return k >= 0 && (bk < 0 || h > bh || (h == bh && k < bk));
}

__global__ __launch_bounds__(CREST_THREADS) void track_crest_kernel(const Params p) {
  __shared__ double r[2 * MAX_LAG + 1];
  const int lane = threadIdx.x;
  const int L = p.max_lag, lags = 2 * L + 1, last = 2 * L;
  const uint64_t rows = (uint64_t)p.n_pairs * p.n_windows;
  for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    // ---- the row's doubles: unit sums added in ascending group order; the largest sample and the finite test ride along
    const float* __restrict__ src = p.part + row * p.n_groups * (uint64_t)lags;
    double* __restrict__ crow = p.corr ? p.corr + row * p.corr_stride : nullptr;
    int bad = 0, big_k = -1;
    double big = 0.0;
    for (int k = lane; k < lags; k += CREST_THREADS) {
      double sum;
      if (p.from_corr) {
        sum = crow[k];
      } else {
        sum = corr_unit_sum(src + k, p.n_groups, (uint64_t)lags);
        if (crow) crow[k] = sum;
      }
      r[k] = sum;
      bad |= !(__builtin_fabs(sum) < __builtin_inf());
      if (big_k < 0 || sum > big) {
        big = sum;
        big_k = k;
      }
    }
    bad = __any(bad);
    __syncthreads();
    if (!p.crest) {
      __syncthreads();
      continue;
    }
    Crest* __restrict__ out = p.crest + row;
    if (bad) {                                             // (wave-uniform)
      if (lane == 0) {
        Crest z = {};
        z.flags = NOT_FINITE;
        *out = z;
      }
      __syncthreads();
      continue;
    }
#pragma unroll
    for (int off = CREST_THREADS / 2; off > 0; off >>= 1) {
      const double ob = __shfl_xor(big, off);
      const int ok = __shfl_xor(big_k, off);
      if (ok >= 0 && (big_k < 0 || ob > big || (ob == big && ok < big_k))) {
        big = ob;
        big_k = ok;
      }
    }
    // ---- every lane's best four candidates, sorted by (h2 descending, k ascending)
    double h[SLOTS];
    int kk[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; i++) {
      h[i] = -1.0;
      kk[i] = -1;
    }
    int count = 0;
    for (int k = 1 + lane; k < last; k += CREST_THREADS) {
      const double lo = r[k - 1], mid = r[k], hi = r[k + 1];
      if (!(mid > 0.0 && mid >= lo && mid > hi)) continue;
      count++;
      double nh = selection_height(lo, mid, hi);
      int nk = k;
#pragma unroll
      for (int i = 0; i < SLOTS; i++)
        if (beats(nh, nk, h[i], kk[i])) {
          const double th = h[i];
          const int tk = kk[i];
          h[i] = nh;
          kk[i] = nk;
          nh = th;
          nk = tk;
        }
    }
#pragma unroll
    for (int off = CREST_THREADS / 2; off > 0; off >>= 1) count += __shfl_xor(count, off);
    // ---- the wave's best four: four times the best head, which its lane then drops
    int win[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; i++) {
      double bh = h[0];
      int bk = kk[0];
#pragma unroll
      for (int off = CREST_THREADS / 2; off > 0; off >>= 1) {
        const double oh = __shfl_xor(bh, off);
        const int ok = __shfl_xor(bk, off);
        if (beats(oh, ok, bh, bk)) {
          bh = oh;
          bk = ok;
        }
      }
      win[i] = bk;                                         // the same in every lane; -1: none left
      if (bk >= 0 && kk[0] == bk) {
#pragma unroll
        for (int s = 0; s + 1 < SLOTS; s++) {
          h[s] = h[s + 1];
          kk[s] = kk[s + 1];
        }
        h[SLOTS - 1] = -1.0;
        kk[SLOTS - 1] = -1;
      }
    }
    // ---- in ascending k, the unused ones last (a sorting network over four)
    auto order = [](int& a, int& b) {
      const unsigned ua = (unsigned)a, ub = (unsigned)b;   // -1 sorts behind every k
      if (ub < ua) {
        const int t = a;
        a = b;
        b = t;
      }
    };
    order(win[0], win[1]);
    order(win[2], win[3]);
    order(win[0], win[2]);
    order(win[1], win[3]);
    order(win[1], win[2]);
    if (lane == 0) {
      Crest c = {};
      c.flags = (count == 0 ? NO_PEAK : 0u) | (big_k == 0 || big_k == last ? AT_EDGE : 0u);
      c.n_candidates = (uint32_t)count;
#pragma unroll
      for (int i = 0; i < SLOTS; i++) {
        const int k = win[i];
        c.slot[i].k = k;
        if (k >= 0) {
          c.slot[i].r[0] = r[k - 1];
          c.slot[i].r[1] = r[k];
          c.slot[i].r[2] = r[k + 1];
        }
      }
      *out = c;
    }
    __syncthreads();                                       // the next row overwrites r
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, track_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, track_kernel<DT_I32>, THREADS, 0); break;
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
    case DT_F32: hipLaunchKernelGGL(track_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    case DT_I32: hipLaunchKernelGGL(track_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, pairs); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int launch_crest(void* stream, const Params& p) {
  uint64_t grid = (uint64_t)p.n_pairs * p.n_windows;
  if (grid > (1u << 20)) grid = 1u << 20;
  hipLaunchKernelGGL(track_crest_kernel, dim3((unsigned)grid), dim3(CREST_THREADS), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace uc_track_dev
