// uc_track_kernel.hip -- the delay tracker's kernels (gfx950): the cross-correlations of uc_xcorr_kernel.hip over a series
// of windows of one recording, and the crest search that leaves one small record per (pair, window).
// include/uchirp_track.h states the definitions; uchirp/track.py holds their float64 models.
//
// track_kernel.  The work unit is (pair, window, group of GROUP segments), numbered window-major inside a pair so that
// units which read the same samples are neighbours; units are dealt statically, a contiguous range each, to the 2-wave
// workgroups of a persistent grid, and a workgroup does a unit from its first load to its 2 L + 1 stored sums on its own:
// no atomics, and a sum cannot depend on the grid.  A unit is computed by the passes of uc_xcorr_kernel.hip in that kernel's order and with its barrier
// discipline -- pk_dft16 | xf_store1 | xf_fwd2 | xf_fwd3<true> for a_s and for b_s, pk_cfmac into sixteen resident
// accumulators, xf_invA | xf_invB | xf_invC<false> -- so that a unit sum has the bits that kernel gives for first' =
// first + w hop and n' = window_len.  The comments there on why the two transforms are kept apart, on which tile a pass may
// write behind which barrier and on the buffer resources that cover exactly the samples that exist hold here word for word.
// What is new:
//   - a unit carries its window's first sample;
//   - a window's last group is usually short (window_len = 8192 at L = 128 is 4 + 1 segments), so the units are of unequal
//     length and a workgroup's next unit starts often;
//   - the loads of the next unit's first segment are therefore issued where a segment's successor is loaded inside a
//     unit: before the arithmetic of the unit's last B transform.  They stay in flight over the inverse transform (whose
//     registers are the accumulators' and the za's, both dead by then).
//
// track_crest_kernel.  One wave per (pair, window).  The lanes stride over k: each adds the row's unit sums in double in
// ascending group order (what xcorr_sum_kernel does), stores the double if corr is given and keeps it in LDS; the largest
// sample (the first one on a tie) and the test for values that are not finite ride along.  Then every lane walks its
// candidates and keeps its own best four by (h2 descending, k ascending) in registers; four rounds of a wave-wide
// butterfly pick the best remaining head, and the four winners are written in ascending k.  The order is total (a k
// belongs to one lane), so the result depends neither on the grid nor on which lane saw which k.
#include <hip/hip_runtime.h>

#include "uc_dev.hpp"
#include "uc_track.hpp"
#include "uc_xform.hpp"
#include "uc_xform_split.hpp"

namespace uc_track_dev {
namespace {

using namespace uc;

constexpr int T = THREADS;
constexpr int kTw2Off = 4 * POINTS;              // floats: behind the two tiles of 2048 complex values
constexpr int kTwBOff = kTw2Off + kXfTw2Floats;
constexpr int kLdsFloats = kTwBOff + kXfTwBFloats;

static_assert(POINTS == kN && THREADS == kXfThreads, "the transform of uc_xform.hpp");
static_assert(2 * MAX_LAG + 1 <= 9 * THREADS, "outputs j + 128 t, t = 0 .. 8, hold every lag");
static_assert(sizeof(Slot) == 32 && sizeof(Crest) == 8 + 32 * SLOTS, "struct uc_track_crest");

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

// one unit: its rows, its window and its segments (workgroup-uniform)
struct Unit {
  const uint32_t* ref;
  const uint32_t* mic;
  int64_t first;      // the window's first reference sample
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
  u.ref = (const uint32_t*)p.in + pr.ref;
  u.mic = (const uint32_t*)p.in + pr.mic;
  u.first = p.first + (int64_t)w * p.hop;
  u.seg0 = grp * GROUP;
  u.seg1 = u.seg0 + GROUP < p.n_segments ? u.seg0 + GROUP : p.n_segments;   // > seg0
  return u;
}

// segment `seg` of the unit's window; S = POINTS - 2 L
__device__ __forceinline__ void load_segment(const Params& p, const Unit& u, uint32_t seg, int S, int L, int j, Raw& g) {
  const int64_t i0 = (int64_t)seg * S;                                  // from the window's first sample
  const int64_t rest = p.window_len - i0;
  const int cnt = rest < S ? (int)rest : S;                             // >= 1
  const int64_t w0 = u.first + i0 - L;                                  // row element of b_s[0]; >= -L
  const int lo = w0 < 0 ? (int)-w0 : 0;                                 // window index of the first sample inside the row
  const int64_t room = p.n_in - w0;                                     // window indices below it lie inside the row; > lo
  const int hi = room < cnt + 2 * L ? (int)room : cnt + 2 * L;          // > lo
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(u.ref + (u.first + i0), cnt * 4);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(u.mic + (w0 + lo), (hi - lo) * 4);
  // every offset whole in the vector operand: the range check looks at it
#pragma unroll
  for (int t = 0; t < 16; t++) g.a[t] = buf_ld32(ra, (j + T * t) * 4, 0);
  if (lo == 0) {                                                        // (workgroup-uniform; all but a row's first samples)
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
__global__ __launch_bounds__(T, 2) void track_kernel(const Params p, const Pair* __restrict__ pairs) {
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
  // the pass-3 twiddles are used by every segment and stay resident; the pass-C ones are used once per unit and are
  // derived there
  v2f w3r[2][8];
  xf_twiddles3(w3r[0], 0, t3a, t3b, t3c, K, H);
  xf_twiddles3(w3r[1], 1, t3a, t3b, t3c, K, H);

  const int L = p.max_lag, S = POINTS - 2 * L, lags = 2 * L + 1;
  // this workgroup's units: one contiguous range of the numbering, all ranges within one unit of the same length.  (Dealing
  // unit b, b + grid, ... instead puts every long group on the even workgroups and every short one on the odd ones wherever a
  // window has two groups and the grid is even: 1.6 times the time at the bench shape, profiles/r13_track.txt.)
  uint32_t unit = (uint32_t)((uint64_t)blockIdx.x * p.n_units / gridDim.x);
  const uint32_t end = (uint32_t)(((uint64_t)blockIdx.x + 1) * p.n_units / gridDim.x);
  if (unit >= end) return;                                           // (the host launches no more workgroups than units)
  Unit u = unit_of(p, pairs, unit);
  Raw g;
  load_segment(p, u, u.seg0, S, L, j, g);
  for (;;) {
    const uint32_t next = unit + 1;
    const bool more = next < end;                                    // workgroup-uniform
    v2f acc[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int t = 0; t < 8; t++) acc[h][t] = mkv(0.0f, 0.0f);
    for (uint32_t seg = u.seg0; seg < u.seg1; ++seg) {
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
        // a whole transform ahead: the unit's next segment, or across the unit boundary the next unit's first one
        const bool inside = seg + 1 < u.seg1;
        if (inside || more) {                                // (workgroup-uniform)
          // (the next unit is derived again behind this one: that is cheaper than keeping it)
          const Unit ul = inside ? u : unit_of(p, pairs, next);
          load_segment(p, ul, inside ? seg + 1 : ul.seg0, S, L, j, g);
        }
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
        sum = 0.0;
        for (uint32_t s = 0; s < p.n_groups; ++s) sum += (double)src[(uint64_t)s * lags + k];
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
