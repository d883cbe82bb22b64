// uc_corr_unit.hpp -- one correlation unit: the cross-correlation of a group of segments of one window of a pair of rows
// out to +-512 lags, by overlap-save on the 2048-point transform of uc_xform.hpp, done by one 2-wave workgroup from its
// first load to its 2 L + 1 stored sums.  xcorr_kernel (uc_xcorr_kernel.hip) and track_kernel (uc_track_kernel.hip) are
// this unit under two deals; what a unit computes, and in which order, is written here and nowhere else, so a unit sum
// of the one kernel has the bits of the other's for the same window.  include/uchirp_xcorr.h states the definition.
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
// samples), the resource starts at the row and a sample in front of it is given an offset beyond every window.
// The loads of the segment that comes next -- which one that is, is the caller's deal -- are issued before the arithmetic
// of the current segment's second transform.
#pragma once
#include "uc_dev.hpp"
#include "uc_xform.hpp"
#include "uc_xform_split.hpp"

namespace uc {

// LDS of a workgroup: two tiles of 2048 complex values and, behind them, the two twiddle tables the loop reads
constexpr int kCorrTw2Off = 4 * kN;              // floats
constexpr int kCorrTwBOff = kCorrTw2Off + kXfTw2Floats;
constexpr int kCorrLdsFloats = kCorrTwBOff + kXfTwBFloats;
constexpr int kCorrMaxLags = 9 * kXfThreads;     // outputs j + 128 t, t = 0 .. 8, are stored

static_assert(kN == 2048 && kXfThreads == 128, "the transform of uc_xform.hpp: 16 samples and 16 bins a thread");
static_assert(kCorrLdsFloats * 4 == 35840, "two workgroups a CU and room to spare");

// a raw input word as a sample (INT32: the row holds int32 words)
template <bool INT32>
__device__ __forceinline__ float corr_sample(float raw) {
  return INT32 ? (float)__float_as_int(raw) : raw;
}

constexpr int kCorrNowhere = 0x7ffffff0;   // a byte offset beyond every window (a window has at most 8192 bytes)

// the raw words of one segment: a_s[j + 128 t] and b_s[j + 128 t]
struct CorrRaw {
  float a[16];
  float b[16];
};

// the window a unit's segments are cut from (workgroup-uniform)
struct CorrWindow {
  const uint32_t* ref;   // the pair's rows
  const uint32_t* mic;
  int64_t first;         // row element of the window's first reference sample
  int64_t n;             // its reference samples
  int64_t n_in;          // samples of a row
};

// segment `seg` of the window; S = 2048 - 2 L
__device__ __forceinline__ void corr_load_segment(const CorrWindow& w, uint32_t seg, int S, int L, int j, CorrRaw& g) {
  const int64_t i0 = (int64_t)seg * S;                                  // from the window's first sample
  const int64_t rest = w.n - i0;
  const int cnt = rest < S ? (int)rest : S;                             // >= 1
  const int64_t w0 = w.first + i0 - L;                                  // row element of b_s[0]; >= -L
  const int lo = w0 < 0 ? (int)-w0 : 0;                                 // window index of the first sample inside the row
  const int64_t room = w.n_in - w0;                                     // window indices below it lie inside the row; > lo
  const int hi = room < cnt + 2 * L ? (int)room : cnt + 2 * L;          // > lo
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(w.ref + (w.first + i0), cnt * 4);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(w.mic + (w0 + lo), (hi - lo) * 4);
  // every offset whole in the vector operand: the range check looks at it
#pragma unroll
  for (int t = 0; t < 16; t++) g.a[t] = buf_ld32(ra, (j + kXfThreads * t) * 4, 0);
  if (lo == 0) {                                                        // (workgroup-uniform; all but a row's first samples)
#pragma unroll
    for (int t = 0; t < 16; t++) g.b[t] = buf_ld32(rb, (j + kXfThreads * t) * 4, 0);
  } else {
    // the window starts in front of the row: the resource starts at the row, and a sample in front of it gets an offset
    // that no resource holds
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int e = j + kXfThreads * t - lo;
      g.b[t] = buf_ld32(rb, e < 0 ? kCorrNowhere : e * 4, 0);
    }
  }
}

// what a workgroup keeps over all its units
struct CorrCtx {
  float* cur;      // the tile a pass 1 (and inverse pass A) writes
  float* oth;      // the tile a pass 2 (and inverse pass B) writes
  float* tw2t;     // W_256^(t k): forward pass 2
  float* twBt;     // W_128^(t k): inverse pass B
  int j;           // the thread, 0 .. 127
  v2f K, H;        // the fixed radix-16 constants
  v2f t3a, t3b, t3c;   // W_2048^j, ^2j, ^4j
  XfAddr xa;
  // the pass-3 twiddles are used by every segment and stay resident (the registers are there at 2 waves per SIMD); the
  // pass-C ones are used once per unit and are derived there
  v2f w3r[2][8];
};

// lds: kCorrLdsFloats floats, 16-byte aligned; tw: exp(-2 pi i k / 2048), k < 2048, (re, im)
__device__ __forceinline__ void corr_setup(CorrCtx& c, float* lds, const float* tw, int j) {
  c.cur = lds;
  c.oth = lds + 2 * kN;
  c.tw2t = lds + kCorrTw2Off;
  c.twBt = lds + kCorrTwBOff;
  c.j = j;
  c.K = mkv(kCos8, kSin8);
  c.H = mkv(kSqrtHalfF, kSqrtHalfF);
  const __amdgpu_buffer_rsrc_t rs_tw = make_rsrc(tw, kN * 8);
  c.t3a = buf_ld64(rs_tw, (j & (kN - 1)) * 8, 0);
  c.t3b = buf_ld64(rs_tw, ((2 * j) & (kN - 1)) * 8, 0);
  c.t3c = buf_ld64(rs_tw, ((4 * j) & (kN - 1)) * 8, 0);
  xf_fill_twiddle_tables(c.tw2t, c.twBt, rs_tw, j);                     // (read behind the first barrier of a segment)
  c.xa = xf_addresses(j);
  xf_twiddles3(c.w3r[0], 0, c.t3a, c.t3b, c.t3c, c.K, c.H);
  xf_twiddles3(c.w3r[1], 1, c.t3a, c.t3b, c.t3c, c.K, c.H);
}

// a unit's cross-spectrum: bins j + 128 h + 256 t
__device__ __forceinline__ void corr_clear(v2f (&acc)[2][8]) {
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int t = 0; t < 8; t++) acc[h][t] = mkv(0.0f, 0.0f);
}

// one segment: acc += conj(A_s) B_s of the words in g.  prefetch() is called once, where g's words have been converted
// and the arithmetic of the second transform has not begun: the caller loads the segment that comes next into g there,
// a whole transform ahead (or nothing, behind its last one).
template <bool INT32, class Prefetch>
__device__ __forceinline__ void corr_segment(const CorrCtx& c, CorrRaw& g, v2f (&acc)[2][8], Prefetch prefetch) {
  // ---- A_s: forward transform of a_s (registers -> cur -> oth -> registers)
  v2f za[2][8];                                          // A_s[j + 128 h + 256 t]
  {
    v2f v[16];
#pragma unroll
    for (int t = 0; t < 16; t++) v[t] = mkv(corr_sample<INT32>(g.a[t]), 0.0f);
    pk_dft16(v, c.K, c.H);
    xf_store1(c.cur, c.xa, c.xa.s1, v);
  }
  __syncthreads();
  xf_fwd2(c.cur, c.oth, c.tw2t, c.xa, c.j, c.K, c.H);
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; h++) xf_fwd3<true>(c.oth, za[h], h, c.w3r[h], c.t3a, c.t3b, c.t3c, c.j, c.K, c.H);
  // ---- B_s: the same of b_s; pass 1 writes the tile pass 2 has read in front of the last barrier, pass 2 the tile pass 3
  // has read in front of the barrier between them
  {
    v2f v[16];
#pragma unroll
    for (int t = 0; t < 16; t++) v[t] = mkv(corr_sample<INT32>(g.b[t]), 0.0f);
    prefetch();
    pk_dft16(v, c.K, c.H);
    xf_store1(c.cur, c.xa, c.xa.s1, v);
  }
  __syncthreads();
  xf_fwd2(c.cur, c.oth, c.tw2t, c.xa, c.j, c.K, c.H);
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; h++) {
    v2f zb[8];
    xf_fwd3<true>(c.oth, zb, h, c.w3r[h], c.t3a, c.t3b, c.t3c, c.j, c.K, c.H);
#pragma unroll
    for (int t = 0; t < 8; t++) acc[h][t] = pk_cfmac(zb[t], za[h][t], acc[h][t]);   // + conj(A_s[k]) B_s[k]
  }
}

// the end of a unit: dst[k] = its sum of lag k - L, k < lags = 2 L + 1
__device__ __forceinline__ void corr_finish(const CorrCtx& c, const v2f (&acc)[2][8], float* __restrict__ dst, int lags) {
  // (what a kernel's launch bounds say of j, said here as well: the address arithmetic of the inverse passes is simplified
  // in this function before it is inlined, and without the range it comes out 2 to 6 VGPRs wider)
  __builtin_assume((unsigned)c.j < (unsigned)kXfThreads);
  // ---- inverse 8 x 16 x 16 of the group's cross-spectrum (registers -> cur -> oth -> registers): cur was last read by a
  // pass 2, oth by the pass 3 in front of the barrier below
#pragma unroll
  for (int h = 0; h < 2; h++) xf_invA(c.cur, acc[h], c.j + kXfThreads * h, c.H);
  __syncthreads();
  xf_invB(c.cur, c.oth, c.twBt, c.xa, c.j, c.K, c.H);
  __syncthreads();
  v2f y[16];
  const v2f none[16] = {};                               // (the resident twiddles xf_invC<false> does not look at)
  xf_invC<false>(c.oth, y, c.xa, none, c.t3a, c.t3b, c.t3c, c.K, c.H);
#pragma unroll
  for (int t = 0; t < 9; t++) {
    const int k = c.j + kXfThreads * t;                  // lag k - L
    if (k < lags) dst[k] = y[t].x * 0x1p-11f;
  }
  // (the next unit's pass 1 writes cur, which pass B has read in front of the last barrier; its pass 2 writes oth behind
  // a barrier that pass C lies in front of)
}

// ---- the weighted unit (wcorr_kernel, uc_wcorr_kernel.hip; include/uchirp_wcorr.h): a real, even weight per bin on the
// group's cross-spectrum, between the last corr_segment and the finish, and a finish that stores a part of the outputs

constexpr int kCorrWeightBins = kN / 2 + 1;   // the staged table: w[k], k = 0 .. 1024

// thread j's sixteen weights: wv[t] = (W[j + 256 t], W[j + 128 + 256 t]), W[k] = w[k] for k <= 1024, w[2048 - k] above.
// table: kCorrWeightBins floats; every index read lies inside it, and the load goes through the range check anyway
__device__ __forceinline__ void corr_load_weights(const float* table, int j, v2f (&wv)[8]) {
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(table, kCorrWeightBins * 4);
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const int k0 = j + 2 * kXfThreads * t, k1 = k0 + kXfThreads;
    wv[t] = mkv(buf_ld32(rw, (k0 <= kN / 2 ? k0 : kN - k0) * 4, 0), buf_ld32(rw, (k1 <= kN / 2 ? k1 : kN - k1) * 4, 0));
  }
}

// acc[h][t] *= W[j + 128 h + 256 t]: one multiply for the real part and one for the imaginary part (one packed instruction)
__device__ __forceinline__ void corr_weight(v2f (&acc)[2][8], const v2f (&wv)[8]) {
#pragma unroll
  for (int t = 0; t < 8; t++) {
    acc[0][t] = pk_scale_lo(acc[0][t], wv[t]);
    acc[1][t] = pk_scale_hi(acc[1][t], wv[t]);
  }
}

// the end of a weighted unit: dst[k] = output k0 + k of the inverse transform, k < lags; k0 + lags <= 1025.  What
// corr_finish does, with the window of stored outputs moved by k0 (corr_finish is this at k0 = 0; it is kept as it is so
// that the kernels built on it keep their bytes)
__device__ __forceinline__ void corr_finish_at(const CorrCtx& c, const v2f (&acc)[2][8], float* __restrict__ dst, int k0, int lags) {
  __builtin_assume((unsigned)c.j < (unsigned)kXfThreads);
#pragma unroll
  for (int h = 0; h < 2; h++) xf_invA(c.cur, acc[h], c.j + kXfThreads * h, c.H);
  __syncthreads();
  xf_invB(c.cur, c.oth, c.twBt, c.xa, c.j, c.K, c.H);
  __syncthreads();
  v2f y[16];
  const v2f none[16] = {};
  xf_invC<false>(c.oth, y, c.xa, none, c.t3a, c.t3b, c.t3c, c.K, c.H);
#pragma unroll
  for (int t = 0; t < 9; t++) {
    const int k = c.j + kXfThreads * t - k0;             // output j + 128 t, up to index 1024 at t = 8
    if ((unsigned)k < (unsigned)lags) dst[k] = y[t].x * 0x1p-11f;
  }
}

// one lag's sum over a window's units: src[s * lags], s < n_groups, added in double in ascending group order
__device__ __forceinline__ double corr_unit_sum(const float* src, uint32_t n_groups, uint64_t lags) {
  double sum = 0.0;
  for (uint32_t s = 0; s < n_groups; ++s) sum += (double)src[(uint64_t)s * lags];
  return sum;
}

}  // namespace uc
