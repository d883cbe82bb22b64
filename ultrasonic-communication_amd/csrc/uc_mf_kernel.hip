// uc_mf_kernel.hip -- the pulse compressor's kernel (gfx950): rows filtered with templates by overlap-save on the
// 2048-point transform of uc_xform.hpp, and an arrival record per (job, segment).  include/uchirp_mf.h states the
// definition; uchirp/mf.py holds its float64 model and an independent float32 evaluation.
//
// Shape: that of compress_kernel and of the correlation unit (uc_corr_unit.hpp, whose context, setup and LDS layout are
// used as they are).  The work unit is (job, segment); the units are dealt statically to the 2-wave workgroups of a
// persistent grid in CHUNKS of consecutive units, so that a workgroup walks along the segments of one job: the job's H
// stays in its registers (it is loaded again only where the set changes), and the T samples two neighbouring windows
// share come from L2.  A workgroup does a unit from its first load to its stores and its record on its own: no atomics,
// and nothing stored can depend on the grid.
//
// One unit: thread j loads a[j + 128 t], t = 0 .. 15 (dwordx2 for pairs, dword for the real types; consecutive lanes read
// consecutive elements) through a buffer resource that covers exactly the window's elements that exist, so what lies in
// front of a row or behind it reads +0 without a branch.  Pass 1 in registers | xf_store1 | xf_fwd2 | xf_fwd3_h_invA
// (x H in registers) | xf_invB | xf_invC, a barrier between them: thread j then holds y of the window positions
// j + 128 t.  The loads of the unit that comes next are issued where this unit's words have been converted: they are in
// flight during the transforms.
//
// The record: e goes into the tile that inverse pass B has read (free behind the barrier in front of pass C), a barrier,
// and every thread reads the two neighbours of its sixteen positions and keeps the candidates' powers alone.  Four rounds
// of a WAVE's arg-max on (e, position), no barrier between them: the wave's greatest e (a max over the thread's sixteen,
// then DPP), the lowest position among the lanes that hold it (only they look for it; DPP), the winner's thread takes its
// value out.  The two waves' lists of four meet in sixteen words of LDS behind ONE barrier and are merged by rank: eight
// lanes hold an entry each and count the other wave's entries that come before it.  The sum: the thread's values in ascending t, the wave's by DPP, wave 0 + wave 1.
#include <hip/hip_runtime.h>

#include "uc_corr_unit.hpp"
#include "uc_mf.hpp"

namespace uc_mf_dev {
namespace {

using namespace uc;

static_assert(POINTS == kN && THREADS == kXfThreads, "the transform of uc_xform.hpp");

// LDS: the two tiles and the two twiddle tables of the correlation unit; behind them the words the two waves exchange:
// per selection round and wave (e, position), then per wave (sum, candidates)
constexpr int kMfSelOff = kCorrLdsFloats;            // [CANDIDATES][2 waves][2]
constexpr int kMfSumOff = kMfSelOff + CANDIDATES * 4;   // [2 waves][2]
constexpr int kMfLdsFloats = kMfSumOff + 4;
static_assert(kMfLdsFloats * 4 == 35920, "two workgroups a CU and room to spare");

__device__ __forceinline__ float wave_sum_f32(float v) {
  UC_DPP_REDUCE("v_add_f32_dpp", v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_sum_u32(int v) {
  UC_DPP_REDUCE("v_add_u32_dpp", v);
  return __builtin_amdgcn_readlane(v, 63);
}

// the raw elements of one window: a[j + 128 t]
template <int DT>
struct Raw {
  v2f g[16];   // (the real types use .x alone; the compiler drops the rest)
};

// where a unit lies (workgroup-uniform)
struct Unit {
  uint64_t row;      // the job's row, in elements from in_dev
  uint32_t set;
  uint32_t job;
  uint32_t seg;      // segment of the call
  int64_t base;      // row element of the segment's output 0
};

__device__ __forceinline__ Unit unit_of(const Params& p, const Job* __restrict__ jobs, uint64_t unit) {
  Unit u;
  u.job = (uint32_t)(unit / p.n_segments);
  u.seg = (uint32_t)(unit - (uint64_t)u.job * p.n_segments);
  const Job jb = jobs[u.job];
  u.row = jb.row;
  u.set = jb.set;
  u.base = p.base0 + (int64_t)u.seg * (int64_t)(POINTS - p.taps - 1);
  return u;
}

// the window of unit u: elements base - T .. base - T + 2047 of the row, +0 where the row has none
template <int DT>
__device__ __forceinline__ void load_window(const Params& p, const Unit& u, int j, Raw<DT>& r) {
  constexpr int ELEM = DT == DT_C32 ? 8 : 4;
  const int64_t w0 = u.base - p.taps;                                  // row element of a[0]; > -2048
  const int lo = w0 < 0 ? (int)-w0 : 0;                                 // window index of the first element inside the row
  const int64_t room = p.n_in - w0;                                     // window indices below it lie inside the row
  const int hi = room < POINTS ? (int)room : POINTS;
  // a unit of a call holds an output inside the row, so hi > lo; a resource of no bytes would read nothing all the same
  const int bytes = hi > lo ? (hi - lo) * ELEM : 0;
  const char* first = (const char*)p.in + ((int64_t)u.row + w0 + lo) * ELEM;
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(first, bytes);
  // every offset whole in the vector operand: the range check looks at it
  if (lo == 0) {                                                        // (workgroup-uniform; all but a row's first windows)
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int off = (j + kXfThreads * t) * ELEM;
      if (DT == DT_C32) r.g[t] = buf_ld64(rs, off, 0);
      else r.g[t].x = buf_ld32(rs, off, 0);
    }
  } else {
    // the window starts in front of the row: the resource starts at the row, and an element in front of it gets an
    // offset that no resource holds
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int e = j + kXfThreads * t - lo;
      const int off = e < 0 ? kCorrNowhere : e * ELEM;
      if (DT == DT_C32) r.g[t] = buf_ld64(rs, off, 0);
      else r.g[t].x = buf_ld32(rs, off, 0);
    }
  }
}

__device__ __forceinline__ void load_spectrum(const Params& p, uint32_t set, int j, v2f (&hres)[2][8]) {
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.spectra + (size_t)set * (2 * POINTS), POINTS * 8);
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int t = 0; t < 8; t++) hres[h][t] = buf_ld64(rs, (j + kXfThreads * h + 256 * t) * 8, 0);
}

template <int DT>
__global__ __launch_bounds__(THREADS, 2) void mf_kernel(const Params p, const Job* __restrict__ jobs) {
  __shared__ __attribute__((aligned(16))) float lds[kMfLdsFloats];
  const int j = threadIdx.x;
  __builtin_assume((unsigned)j < (unsigned)kXfThreads);
  CorrCtx c;
  corr_setup(c, lds, p.tw, j);
  float* const sel = lds + kMfSelOff;
  float* const wsum = lds + kMfSumOff;
  const int wave = __builtin_amdgcn_readfirstlane(j >> 6);

  const int T = p.taps, S = POINTS - T - 1;
  const uint64_t unit0 = (uint64_t)blockIdx.x * p.chunk;
  uint64_t unit1 = unit0 + p.chunk;
  if (unit1 > p.n_units) unit1 = p.n_units;
  if (unit0 >= unit1) return;                                           // (workgroup-uniform)

  v2f hres[2][8];
  uint32_t set = 0xffffffffu;
  Unit u = unit_of(p, jobs, unit0);
  Raw<DT> raw;
  load_window<DT>(p, u, j, raw);
  for (uint64_t unit = unit0; unit < unit1; ++unit) {
    if (u.set != set) {
      set = u.set;
      load_spectrum(p, set, j, hres);
    }
    const Unit cur_u = u;
    // ---- forward pass 1 of the window (registers -> cur)
    {
      v2f v[16];
#pragma unroll
      for (int t = 0; t < 16; t++) {
        if (DT == DT_C32) v[t] = raw.g[t];
        else v[t] = mkv(corr_sample<DT == DT_I32>(raw.g[t].x), 0.0f);
      }
      if (unit + 1 < unit1) {                                           // the next unit's loads: in flight during the transforms
        u = unit_of(p, jobs, unit + 1);
        load_window<DT>(p, u, j, raw);
      }
      pk_dft16(v, c.K, c.H);
      xf_store1(c.cur, c.xa, c.xa.s1, v);
    }
    __syncthreads();
    xf_fwd2(c.cur, c.oth, c.tw2t, c.xa, c.j, c.K, c.H);
    __syncthreads();
    xf_fwd3_h_invA<false>(c.oth, c.cur, hres, c.w3r, c.t3a, c.t3b, c.t3c, c.j, c.K, c.H);
    __syncthreads();
    xf_invB(c.cur, c.oth, c.twBt, c.xa, c.j, c.K, c.H);
    __syncthreads();
    v2f y[16];                                                          // window positions j + 128 t
    {
      const v2f none[16] = {};
      xf_invC<false>(c.oth, y, c.xa, none, c.t3a, c.t3b, c.t3c, c.K, c.H);
    }

    // ---- which positions are outputs of the call: T + u_lo <= position < T + u_hi  (u_lo < u_hi: the unit is the call's)
    const int64_t rel = cur_u.base - p.first;                           // the segment's output 0 as an output of the call
    const int u_lo = rel < 0 ? (int)-rel : 0;
    const int64_t left = p.n - rel;
    const int u_hi = left < S ? (int)left : S;
    const int pos_lo = T + u_lo, pos_hi = T + u_hi;

    float e[16];
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int t = 0; t < 16; t++) {
        const float q = y[t].y * y[t].y;                                // rounded first
        e[t] = __builtin_fmaf(y[t].x, y[t].x, q);
      }
    }

    // ---- stores: consecutive lanes on consecutive elements
    if (p.out) {
      const int64_t row0 = (int64_t)cur_u.job * (int64_t)p.out_stride + rel - T;   // element of window position 0
#pragma unroll
      for (int t = 0; t < 16; t++) {
        const int pos = j + kXfThreads * t;
        if (pos >= pos_lo && pos < pos_hi) {
          const int64_t o = row0 + pos;
          switch (p.format) {
            case OUT_COMPLEX: ((v2f*)p.out)[o] = y[t]; break;
            case OUT_REAL: ((float*)p.out)[o] = y[t].x; break;
            case OUT_POWER: ((float*)p.out)[o] = e[t]; break;
            default: ((float*)p.out)[o] = sqrtf(e[t]); break;
          }
        }
      }
    }

    // ---- the record
    if (p.records) {
      // cur was last read by inverse pass B, in front of the barrier that pass C lies behind
      float* const et = c.cur;
#pragma unroll
      for (int t = 0; t < 16; t++) et[j + kXfThreads * t] = e[t];
      __syncthreads();
      // the sum of the outputs in range; then e keeps the candidates' powers alone, 0 elsewhere (a candidate's power is
      // greater than a neighbour's: > 0): the outputs are stored, and the record reads its neighbours from the tile
      unsigned mask = 0;
      float sum = 0.0f;
#pragma unroll
      for (int t = 0; t < 16; t++) {
        const int pos = j + kXfThreads * t;
        if (pos >= pos_lo && pos < pos_hi) {                            // (positions T .. 2046: both neighbours exist)
          sum += e[t];
          if (e[t] >= et[pos - 1] && e[t] > et[pos + 1]) mask |= 1u << t;
        }
      }
#pragma unroll
      for (int t = 0; t < 16; t++) e[t] = ((mask >> t) & 1u) ? e[t] : 0.0f;
      {
        const float ws = wave_sum_f32(sum);
        const int wn = wave_sum_u32(__builtin_popcount(mask));
        // (every lane of a wave stores the wave's words: one address, one value)
        wsum[2 * wave] = ws;
        wsum[2 * wave + 1] = __int_as_float(wn);
      }
#ifdef UC_MF_NO_SELECT   // diagnostic build (tools/mf_bench.py): the rounds' share of the time; its records hold no candidate
      if (j < 4 * CANDIDATES) sel[j] = (j & 1) ? __int_as_float(0x7fffffff) : 0.0f;
#else
      // ---- each wave's four greatest candidates, by falling e, the lower position first on a tie: sel[4 r + 2 wave]
#pragma unroll
      for (int r = 0; r < CANDIDATES; r++) {
        // the wave's greatest power; only the lanes that hold it look for where (the lowest of a lane's positions first:
        // ascending t is ascending position), and the lowest position among them is the wave's
        float be = e[0];
#pragma unroll
        for (int t = 1; t < 16; t++) be = max_f32(be, e[t]);
        const float we = wave_max_f32(be);
        int wp = 0x7fffffff;                                            // no candidate is left
        if (we > 0.0f) {                                                // (wave-uniform)
          int bp = 0x7fffffff;
          if (be == we) {
#pragma unroll
            for (int t = 15; t >= 0; t--)
              if (e[t] == we) bp = j + kXfThreads * t;
          }
          wp = wave_min_u32(bp);
        }
        sel[4 * r + 2 * wave] = we;
        sel[4 * r + 2 * wave + 1] = __int_as_float(wp);
        // the winner's thread takes it out (0x7fffffff >> 7 is no t)
        const int mine = (wp & (kXfThreads - 1)) == j ? wp >> 7 : -1;
#pragma unroll
        for (int t = 0; t < 16; t++) e[t] = t == mine ? 0.0f : e[t];
      }
#endif
      __syncthreads();                                                  // (behind the waves' sums as well)
      // ---- the two lists merged by rank: lane i + 4 w has entry i of wave w and counts the other wave's entries that
      // come before it (a greater e, or the same e at a lower position; positions differ); slot rank is its own
      uint32_t* const rec = p.records + ((uint64_t)cur_u.job * p.n_segments + cur_u.seg) * RECORD_WORDS;
      if (j < 2 * CANDIDATES) {
        const int li = j & (CANDIDATES - 1), w = j >> 2;
        const float my_e = sel[4 * li + 2 * w];
        const int my_p = __float_as_int(sel[4 * li + 2 * w + 1]);
        int rank = li;
#pragma unroll
        for (int k = 0; k < CANDIDATES; k++) {
          const float oe = sel[4 * k + 2 * (1 - w)];
          const int op = __float_as_int(sel[4 * k + 2 * (1 - w) + 1]);
          rank += (oe > my_e || (oe == my_e && op < my_p)) ? 1 : 0;
        }
        if (my_e > 0.0f && rank < CANDIDATES) {
          rec[4 * rank] = (uint32_t)(my_p - T);
          rec[4 * rank + 1] = __float_as_uint(et[my_p - 1]);
          rec[4 * rank + 2] = __float_as_uint(my_e);
          rec[4 * rank + 3] = __float_as_uint(et[my_p + 1]);
        }
      } else if (j < 3 * CANDIDATES) {                                  // the slots no candidate takes: zeros
        const int slot = j - 2 * CANDIDATES;
        int kept = 0;
#pragma unroll
        for (int k = 0; k < 2 * CANDIDATES; k++) kept += sel[2 * k] > 0.0f ? 1 : 0;
        if (slot >= kept) {
          rec[4 * slot] = 0u;
          rec[4 * slot + 1] = 0u;
          rec[4 * slot + 2] = 0u;
          rec[4 * slot + 3] = 0u;
        }
      } else if (j == 3 * CANDIDATES) {
        rec[16] = __float_as_uint(wsum[0] + wsum[2]);
        rec[17] = (uint32_t)(u_hi - u_lo);
        rec[18] = (uint32_t)(__float_as_int(wsum[1]) + __float_as_int(wsum[3]));
        rec[19] = 0u;
      }
      // the next unit's pass 1 writes the tile the record's neighbours are read from, and its sums the words read here
      __syncthreads();
    }
    // (without a record: the next unit's pass 1 writes cur, which pass B has read in front of the last barrier; its pass 2
    // writes oth behind a barrier that pass C lies in front of)
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mf_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mf_kernel<DT_I32>, THREADS, 0); break;
    case DT_C32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mf_kernel<DT_C32>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_run(int dtype, unsigned grid, void* stream, const Params& p, const Job* jobs) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(mf_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p, jobs); break;
    case DT_I32: hipLaunchKernelGGL(mf_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p, jobs); break;
    case DT_C32: hipLaunchKernelGGL(mf_kernel<DT_C32>, dim3(grid), dim3(THREADS), 0, hs, p, jobs); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_mf_dev
