// uc_xcorr_kernel.hip -- the wide-lag correlator's kernels (gfx950): cross-correlations of pairs of rows out to +-512
// lags by overlap-save on the 2048-point transform of uc_xform.hpp.  include/uchirp_xcorr.h states the definition;
// uchirp/xcorr.py holds its float64 model and an independent float32 evaluation.
//
// Shape: that of compress_kernel.  The work unit is (pair, group of GROUP segments); units are dealt statically to the
// 2-wave workgroups of a persistent grid, and a workgroup does a unit from its first load to its 2 L + 1 stored sums on
// its own: no atomics, and a sum cannot depend on the grid.
//
// One segment: thread j loads a_s[j + 128 t] and b_s[j + 128 t], t = 0 .. 15 (32 dword buffer loads; consecutive lanes
// read consecutive samples).  a_s and b_s go through a forward 16 x 16 x 8 transform EACH (pass 1 in registers,
// xf_store1 | xf_fwd2 | xf_fwd3, a barrier between them), as the real parts of complex inputs.  Thread j then holds the
// sixteen bins A_s[k], and after the second transform B_s[k], k = j + 128 h + 256 t, and adds conj(A_s[k]) B_s[k] to its
// sixteen accumulators: two packed instructions per bin.  The accumulators stay in registers over the group's segments.
// Why not ONE transform of z = a_s + j b_s and the separation A = (Z[k] + conj Z[P - k]) / 2, B = (Z[k] - conj Z[P - k]) / 2j
// (a mirrored exchange through LDS: 16 writes, 16 reads, a barrier, and four packed instructions per bin)?  That form
// needs about a quarter fewer instructions per segment, but its error scales with ||a_s||^2 + ||b_s||^2, not with
// ||a_s|| ||b_s||: a reference row of zeros gave sums that were not zero, and a single reference sample (n = 1) against a
// window of 1025 microphone samples came out at 3.95 x 2^-24 E_p where the float32 emulation has 0.27.  The header's error
// form is part of the definition, so the transforms are kept apart: a row of zeros transforms to zeros exactly, and the
// error of a product is the error of its factors.
// Pass 1 of a transform writes the tile pass 2 of the one before has read, pass 2 the tile pass 3 of the one before has
// read, each behind a barrier the read lies in front of: four barriers per segment, none extra.
//
// End of a unit: the accumulated cross-spectrum sits exactly where xf_fwd3_h_invA has its product, so the inverse
// 8 x 16 x 16 starts in the same registers: xf_invA | xf_invB | xf_invC.  The transform is not normalised: y = P c, so the
// correlation is Re(y) * 2^-11 (exact).  Output sample j + 128 t is c[j + 128 t]; the 2 L + 1 <= 1025 first ones are
// stored as floats, consecutive lanes on consecutive words.
//
// Edges: a segment's two windows are described by buffer resources that cover exactly the samples that exist -- the
// reference's cnt samples; of the microphone's cnt + 2 L the part inside the row -- and every load goes through the
// resource's range check, which returns 0 (+0.0f, and 0 as an integer word) instead of reading: nothing outside the rows
// is ever read, whatever first, n and L are.  Where the microphone's window starts in front of the row (a row's first
// segment), the resource starts at the row and a sample in front of it is given an offset beyond every window.
// The next segment's loads are issued before the arithmetic of the current segment's second transform.
//
// sum_kernel adds a pair's unit sums in double, in ascending group order, one thread per (pair, lag).
#include <hip/hip_runtime.h>

#include "uc_dev.hpp"
#include "uc_xcorr.hpp"
#include "uc_xform.hpp"
#include "uc_xform_split.hpp"

namespace uc_xcorr_dev {
namespace {

using namespace uc;

constexpr int T = THREADS;
constexpr int kTw2Off = 4 * POINTS;              // floats: behind the two tiles of 2048 complex values
constexpr int kTwBOff = kTw2Off + kXfTw2Floats;
constexpr int kLdsFloats = kTwBOff + kXfTwBFloats;

static_assert(POINTS == kN && THREADS == kXfThreads, "the transform of uc_xform.hpp");
static_assert(2 * MAX_LAG + 1 <= 9 * THREADS, "outputs j + 128 t, t = 0 .. 8, hold every lag");

template <int DT>
__device__ __forceinline__ float as_sample(float raw) {
  return DT == DT_I32 ? (float)__float_as_int(raw) : raw;
}

constexpr int kNowhere = 0x7ffffff0;   // a byte offset beyond every window (a window has at most 8192 bytes)

// the raw words of one segment: a_s[j + 128 t] and b_s[j + 128 t]
struct Raw {
  float a[16];
  float b[16];
};

// segment `seg` of the pair whose rows start at ref / mic (elements from p.in); S = POINTS - 2 L
__device__ __forceinline__ void load_segment(const Params& p, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ mic,
                                             uint32_t seg, int S, int L, int j, Raw& g) {
  const int64_t i0 = (int64_t)seg * S;                                  // from first
  const int64_t rest = p.n - i0;
  const int cnt = rest < S ? (int)rest : S;                             // >= 1
  const int64_t w0 = p.first + i0 - L;                                  // row element of b_s[0]; >= -L
  const int lo = w0 < 0 ? (int)-w0 : 0;                                 // window index of the first sample inside the row
  const int64_t room = p.n_in - w0;                                     // window indices below it lie inside the row; > lo
  const int hi = room < cnt + 2 * L ? (int)room : cnt + 2 * L;          // > lo
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(ref + (p.first + i0), cnt * 4);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(mic + (w0 + lo), (hi - lo) * 4);
  // every offset whole in the vector operand: the range check looks at it
#pragma unroll
  for (int t = 0; t < 16; t++) g.a[t] = buf_ld32(ra, (j + T * t) * 4, 0);
  if (lo == 0) {                                                        // (workgroup-uniform; all but a row's first segment)
#pragma unroll
    for (int t = 0; t < 16; t++) g.b[t] = buf_ld32(rb, (j + T * t) * 4, 0);
  } else {
    // the window starts in front of the row: the resource starts at the row, and a sample in front of it gets an offset
    // that no resource holds
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int e = j + T * t - lo;
      g.b[t] = buf_ld32(rb, e < 0 ? kNowhere : e * 4, 0);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(T, 2) void xcorr_kernel(const Params p, const Pair* __restrict__ pairs) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  float* const cur = lds;               // the tile a pass 1 (and inverse pass A) writes
  float* const oth = lds + 2 * POINTS;  // the tile a pass 2 (and inverse pass B) writes
  float* tw2t = lds + kTw2Off;    // W_256^(t k): forward pass 2
  float* twBt = lds + kTwBOff;    // W_128^(t k): inverse pass B

  const int j = threadIdx.x;
  const v2f K = mkv(kCos8, kSin8), H = mkv(kSqrtHalfF, kSqrtHalfF);
  const __amdgpu_buffer_rsrc_t rs_tw = make_rsrc(p.tw, POINTS * 8);
  const v2f t3a = buf_ld64(rs_tw, (j & (POINTS - 1)) * 8, 0);        // W_2048^j
  const v2f t3b = buf_ld64(rs_tw, ((2 * j) & (POINTS - 1)) * 8, 0);  // W_2048^2j
  const v2f t3c = buf_ld64(rs_tw, ((4 * j) & (POINTS - 1)) * 8, 0);  // W_2048^4j
  xf_fill_twiddle_tables(tw2t, twBt, rs_tw, j);                      // (read behind the first barrier of the loop)
  const XfAddr xa = xf_addresses(j);
  // the pass-3 twiddles are used by every segment and stay resident (the registers are there at 2 waves per SIMD); the
  // pass-C ones are used once per unit and are derived there
  v2f w3r[2][8];
  xf_twiddles3(w3r[0], 0, t3a, t3b, t3c, K, H);
  xf_twiddles3(w3r[1], 1, t3a, t3b, t3c, K, H);

  const int L = p.max_lag, S = POINTS - 2 * L, lags = 2 * L + 1;
  const uint32_t* __restrict__ in = (const uint32_t*)p.in;
  for (uint64_t unit = blockIdx.x; unit < p.n_units; unit += gridDim.x) {
    const uint32_t pair = (uint32_t)(unit / p.n_groups);
    const uint32_t grp = (uint32_t)(unit - (uint64_t)pair * p.n_groups);
    const Pair pr = pairs[pair];
    const uint32_t* __restrict__ ref = in + pr.ref;
    const uint32_t* __restrict__ mic = in + pr.mic;
    const uint32_t seg0 = grp * GROUP;
    const uint32_t seg1 = seg0 + GROUP < p.n_segments ? seg0 + GROUP : p.n_segments;   // > seg0
    v2f acc[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int t = 0; t < 8; t++) acc[h][t] = mkv(0.0f, 0.0f);
    Raw g;
    load_segment(p, ref, mic, seg0, S, L, j, g);
    for (uint32_t seg = seg0; seg < seg1; ++seg) {
      // ---- A_s: forward transform of a_s (registers -> cur -> oth -> registers)
      v2f za[2][8];                                          // A_s[j + 128 h + 256 t]
      {
        v2f v[16];
#pragma unroll
        for (int t = 0; t < 16; t++) v[t] = mkv(as_sample<DT>(g.a[t]), 0.0f);
        pk_dft16(v, K, H);
        xf_store1(cur, xa, xa.s1, v);
      }
      __syncthreads();
      xf_fwd2(cur, oth, tw2t, xa, j, K, H);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; h++) xf_fwd3<true>(oth, za[h], h, w3r[h], t3a, t3b, t3c, j, K, H);
      // ---- B_s: the same of b_s; pass 1 writes the tile pass 2 has read in front of the last barrier, pass 2 the tile pass 3
      // has read in front of the barrier between them
      {
        v2f v[16];
#pragma unroll
        for (int t = 0; t < 16; t++) v[t] = mkv(as_sample<DT>(g.b[t]), 0.0f);
        if (seg + 1 < seg1) load_segment(p, ref, mic, seg + 1, S, L, j, g);   // a whole transform ahead
        pk_dft16(v, K, H);
        xf_store1(cur, xa, xa.s1, v);
      }
      __syncthreads();
      xf_fwd2(cur, oth, tw2t, xa, j, K, H);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; h++) {
        v2f zb[8];
        xf_fwd3<true>(oth, zb, h, w3r[h], t3a, t3b, t3c, j, K, H);
#pragma unroll
        for (int t = 0; t < 8; t++) acc[h][t] = pk_cfmac(zb[t], za[h][t], acc[h][t]);   // + conj(A_s[k]) B_s[k]
      }
    }
    // ---- inverse 8 x 16 x 16 of the group's cross-spectrum (registers -> cur -> oth -> registers): cur was last read by a
    // pass 2, oth by the pass 3 in front of the barrier below
#pragma unroll
    for (int h = 0; h < 2; h++) xf_invA(cur, acc[h], j + T * h, H);
    __syncthreads();
    xf_invB(cur, oth, twBt, xa, j, K, H);
    __syncthreads();
    v2f y[16];
    const v2f none[16] = {};                               // (the resident twiddles xf_invC<false> does not look at)
    xf_invC<false>(oth, y, xa, none, t3a, t3b, t3c, K, H);
    float* __restrict__ dst = p.part + unit * (uint64_t)lags;
#pragma unroll
    for (int t = 0; t < 9; t++) {
      const int k = j + T * t;                               // lag k - L
      if (k < lags) dst[k] = y[t].x * 0x1p-11f;
    }
    // (the next unit's pass 1 writes cur, which pass B has read in front of the last barrier; its pass 2 writes oth behind
    // a barrier that pass C lies in front of)
  }
}

// corr[pair][k] = the pair's unit sums of lag k - max_lag, added in double in ascending group order
__global__ __launch_bounds__(SUM_THREADS) void xcorr_sum_kernel(const Params p) {
  const uint64_t lags = 2 * (uint64_t)p.max_lag + 1;
  const uint64_t total = (uint64_t)p.n_pairs * lags;
  for (uint64_t t = (uint64_t)blockIdx.x * SUM_THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * SUM_THREADS) {
    const uint64_t pair = t / lags, k = t - pair * lags;
    const float* __restrict__ src = p.part + pair * p.n_groups * lags + k;
    double sum = 0.0;
    for (uint32_t s = 0; s < p.n_groups; ++s) sum += (double)src[(uint64_t)s * lags];
    p.corr[pair * p.corr_stride + k] = sum;
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
