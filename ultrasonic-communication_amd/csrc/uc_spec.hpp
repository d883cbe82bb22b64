// What the host side (uc_spec_api.cpp) and the kernel file (uc_spec_kernel.hip) of libuchirp_spec.so share; and, for the
// kernel file alone, the device helpers that are the analyser's own (the shared device headers stay as they are).
#pragma once
#include <cstddef>
#include <cstdint>

namespace uc_spec_dev {

constexpr int THREADS = 128;             // 2 waves: one 2048-point transform per workgroup (uc_xform.hpp)
constexpr int POINTS = 2048;             // UC_SPEC_POINTS
constexpr int BINS = POINTS / 2 + 1;     // UC_SPEC_BINS: 0 .. 1024

constexpr int DT_I32 = 0, DT_F32 = 1;    // UC_SPEC_DTYPE_*
constexpr int MAG = 0, POWER = 1, DB = 2;   // UC_SPEC_*

// one frame's peak (struct uc_spec_peak)
struct Peak {
  float value;
  uint32_t bin;
};

// A unit is one frame: unit = row * n_frames + frame.  Its bins go to out[unit * out_stride + (k - bin_first)], its peak to
// peaks[unit].
struct Params {
  const void* in;
  const float* tw;           // exp(-2 pi i k / 2048), k < 2048, (re, im)
  const float* window;       // frame_len floats
  float* out;
  Peak* peaks;               // or NULL
  int64_t n_in;
  int64_t first;
  uint64_t in_stride;
  uint64_t out_stride;
  uint64_t n_units;          // n_rows * n_frames
  uint64_t n_frames;
  uint32_t hop;
  int32_t frame_len;
  int32_t bin_first;
  int32_t n_bins;
  int32_t ac_bins;
  int32_t kind;
  float scale;
  float floor;
  float db_mul;
};

// workgroups of the kernel for `dtype` that one CU holds at once (the runtime's occupancy figure; <= 0: unknown)
int resident_blocks_per_cu(int dtype);

// launch (uc_spec_kernel.hip); dtype: UC_SPEC_DTYPE_*; returns the hipError_t of the launch as int
int launch_spectra(int dtype, unsigned grid, void* stream, const Params& p);

}  // namespace uc_spec_dev

#ifdef __HIP__
#include "uc_dev.hpp"
#include "uc_xform.hpp"

namespace uc_spec_dev {

using uc::v2f;

// LDS of a workgroup: two tiles of 2048 complex values, the pass-2 twiddles behind them, and one peak per wave
constexpr int kSpecTw2Off = 4 * uc::kN;                      // floats
constexpr int kSpecPeakOff = kSpecTw2Off + uc::kXfTw2Floats;
constexpr int kSpecLdsFloats = kSpecPeakOff + 4;
static_assert(kSpecLdsFloats * 4 == 34832, "four workgroups a CU");

constexpr int kSpecNowhere = 0x7ffffff0;   // a byte offset beyond every frame (a frame has at most 8192 bytes)
constexpr int kSpecNoBin = 0x7fffffff;     // a lane without a candidate

// W_256^(t k), t < 16, k < 16, at tw2t[16 t + k]: what xf_fwd2 reads (the first table of xf_fill_twiddle_tables)
__device__ __forceinline__ void spec_fill_tw2(float* tw2t, __amdgpu_buffer_rsrc_t rs_tw, int j) {
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int e = j + uc::kXfThreads * r;  // t = e >> 4, k = e & 15
    uc::lds_st(tw2t, e, uc::buf_ld64(rs_tw, ((8 * (e >> 4) * (e & 15)) & (uc::kN - 1)) * 8, 0));
  }
}

// The raw words x[s + j + 128 t], t < 16, of the frame that starts at row element s (which may be negative): the buffer
// resource covers exactly the samples that lie inside the row and below frame_len, and the range check returns 0 for every
// other one.  Where the frame starts in front of its row (lo > 0) the resource starts at the row, and a sample in front of
// it is given an offset that no resource holds (the lo > 0 form of corr_load_segment, uc_corr_unit.hpp).
__device__ __forceinline__ void spec_load_frame(const uint32_t* row, int64_t s, int64_t n_in, int frame_len, int j, float (&g)[16]) {
  const int64_t room = n_in - s;                                        // frame indices below it lie inside the row
  int lo = s < 0 ? (s < -(int64_t)frame_len ? frame_len : (int)-s) : 0;
  int hi = room < (int64_t)frame_len ? (room < 0 ? 0 : (int)room) : frame_len;
  if (hi < lo) hi = lo;                                                 // (a frame wholly outside its row: nothing is read)
  const __amdgpu_buffer_rsrc_t rs = uc::make_rsrc(row + (s + lo), (hi - lo) * 4);
  if (lo == 0) {                                                        // (workgroup-uniform; all but a row's first frames)
#pragma unroll
    for (int t = 0; t < 16; t++) g[t] = uc::buf_ld32(rs, (j + uc::kXfThreads * t) * 4, 0);
  } else {
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int e = j + uc::kXfThreads * t - lo;
      g[t] = uc::buf_ld32(rs, e < 0 ? kSpecNowhere : e * 4, 0);
    }
  }
}

// the stored value of one bin (include/uchirp_spec.h, "Values"): every operation rounded once, none contracted
__device__ __forceinline__ float spec_value(v2f z, int k, const Params& p) {
#pragma clang fp contract(off)
  float v = p.scale * __fsqrt_rn(__fmaf_rn(z.y, z.y, z.x * z.x));
  if (k < p.ac_bins) v = 1.0f;
  if (p.kind == POWER) return v * v;
  if (p.kind == DB) return p.db_mul * log10f(v > p.floor ? v : p.floor);   // (a NaN goes to the floor)
  return v;
}

// the wave's first maximum: the largest candidate and, among the lanes that hold it, the lowest bin
__device__ __forceinline__ void spec_wave_first_max(float& v, int& k) {
  const float m = uc::wave_max_f32(v);
  k = uc::wave_min_u32(v == m ? k : kSpecNoBin);
  v = m;
}

}  // namespace uc_spec_dev
#endif
