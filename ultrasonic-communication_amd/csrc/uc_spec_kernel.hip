// uc_spec_kernel.hip -- the spectrum analyser's kernel (gfx950): the magnitude, power or level spectrum of every frame of
// many rows, and each frame's largest stored value.  include/uchirp_spec.h states the definition; uchirp/spec.py holds its
// float64 model and an independent float32 evaluation.
//
// Shape: that of xcorr_kernel.  The work unit is one frame (row m, frame f; unit = m n_frames + f); units are dealt
// statically, a contiguous range each, to the 2-wave workgroups of a persistent grid (frames that overlap are neighbours in
// the numbering, so a workgroup reads most of its samples twice in a row), and a workgroup does a frame from its first load
// to its last store on its own: no atomics, and a value cannot depend on the grid.
//
// One frame: thread j loads x[first + f hop + j + 128 t], t < 16 (spec_load_frame: the range check of the buffer resource
// supplies every zero), multiplies by its sixteen window values -- loaded once per workgroup and kept in registers -- and
// runs the forward 16 x 16 x 8 transform of uc_xform.hpp on (u, 0): pass 1 in registers, xf_store1 | xf_fwd2 | xf_fwd3, a
// barrier between them.  Each frame has a transform of its own (a frame of zeros gives zeros exactly).  Thread j then holds
// the bins j + 128 h + 256 t; those up to 1023 are h < 2, t < 4, and bin 1024 is thread 0's (h = 0, t = 4).  Neighbouring
// lanes hold neighbouring bins: a wave's store is 64 consecutive floats.  The next frame's loads are issued in front of
// pass 3.  Pass 1 of a frame writes the tile pass 2 of the one before has read, pass 2 the tile pass 3 of the one before
// has read, each behind a barrier the read lies in front of: two barriers per frame.
//
// Peak: every lane keeps the first maximum of the values it stores (ascending bins, a strict comparison), the wave reduces
// (value by v_max_f32 in DPP steps, then the lowest bin among the lanes that hold it), lane 0 of each wave leaves the wave's
// pair in LDS, and thread 0 merges the two BEHIND THE NEXT BARRIER THERE IS ANYWAY -- the first one of the next frame --
// so the search costs no barrier of its own.  A NaN is never a maximum; a frame that stores nothing but NaN has
// { NaN, bin_first }.
#include <hip/hip_runtime.h>

#include "uc_spec.hpp"
#include "uc_xform_split.hpp"

namespace uc_spec_dev {
namespace {

using namespace uc;

static_assert(POINTS == kN && THREADS == kXfThreads, "the transform of uc_xform.hpp: 16 samples a thread");

// u = w x of a raw input word (DT_I32: the row holds int32 words), rounded once: no addition of pass 1 is fused into it
template <int DT>
__device__ __forceinline__ float spec_windowed(float w, float raw) {
#pragma clang fp contract(off)
  return w * (DT == DT_I32 ? (float)__float_as_int(raw) : raw);
}

// frame f of row m (workgroup-uniform), and the loads of its samples
struct Frame {
  uint64_t m, f;
};
__device__ __forceinline__ void spec_load(const Params& p, const Frame& fr, int j, float (&g)[16]) {
  const uint32_t* row = (const uint32_t*)p.in + fr.m * p.in_stride;
  spec_load_frame(row, p.first + (int64_t)(fr.f * p.hop), p.n_in, p.frame_len, j, g);
}

// thread 0, behind a barrier: the two waves' pairs -> the frame's record
__device__ __forceinline__ void spec_emit_peak(const Params& p, const float* slot, uint64_t unit) {
  float v0 = slot[0], v1 = slot[2];
  int k0 = __float_as_int(slot[1]), k1 = __float_as_int(slot[3]);
  if (v1 > v0 || (v1 == v0 && k1 < k0)) {
    v0 = v1;
    k0 = k1;
  }
  Peak r;
  r.value = k0 == kSpecNoBin ? __builtin_nanf("") : v0;
  r.bin = k0 == kSpecNoBin ? (uint32_t)p.bin_first : (uint32_t)k0;
  p.peaks[unit] = r;
}

template <int DT>
__global__ __launch_bounds__(THREADS, 2) void spec_kernel(const Params p) {
  __shared__ __attribute__((aligned(16))) float lds[kSpecLdsFloats];
  const int j = threadIdx.x;
  float* const cur = lds;                  // the tile pass 1 writes
  float* const oth = lds + 2 * kN;         // the tile pass 2 writes
  float* const tw2t = lds + kSpecTw2Off;
  float* const slot = lds + kSpecPeakOff;  // (value, bin) of wave 0, of wave 1
  const v2f K = mkv(kCos8, kSin8), H = mkv(kSqrtHalfF, kSqrtHalfF);
  const __amdgpu_buffer_rsrc_t rs_tw = make_rsrc(p.tw, kN * 8);
  const v2f t3a = buf_ld64(rs_tw, (j & (kN - 1)) * 8, 0);
  const v2f t3b = buf_ld64(rs_tw, ((2 * j) & (kN - 1)) * 8, 0);
  const v2f t3c = buf_ld64(rs_tw, ((4 * j) & (kN - 1)) * 8, 0);
  spec_fill_tw2(tw2t, rs_tw, j);           // (read behind the first barrier of a frame)
  const XfAddr xa = xf_addresses(j);
  v2f w3r[2][8];                           // the pass-3 twiddles stay resident: the registers are there at 2 waves per SIMD
  xf_twiddles3(w3r[0], 0, t3a, t3b, t3c, K, H);
  xf_twiddles3(w3r[1], 1, t3a, t3b, t3c, K, H);
  // the window: w[j + 128 t], +0.0f from frame_len on (the resource's range check)
  float wv[16];
  {
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(p.window, p.frame_len * 4);
#pragma unroll
    for (int t = 0; t < 16; t++) wv[t] = buf_ld32(rs_w, (j + kXfThreads * t) * 4, 0);
  }

  // this workgroup's frames: one contiguous range of the numbering, all ranges within one frame of the same length
  uint64_t unit = (uint64_t)blockIdx.x * p.n_units / gridDim.x;
  const uint64_t end = ((uint64_t)blockIdx.x + 1) * p.n_units / gridDim.x;
  if (unit >= end) return;                 // (the host launches no more workgroups than frames)
  const bool peaks = p.peaks != nullptr;
  float g[16];
  Frame fr;                                // of `unit`; one division a workgroup, then counted on
  fr.m = unit / p.n_frames;
  fr.f = unit - fr.m * p.n_frames;
  spec_load(p, fr, j, g);
  bool pending = false;                    // the frame before has left its waves' peaks in `slot`
  for (;;) {
    const bool more = unit + 1 < end;      // workgroup-uniform
    {
      v2f v[16];
#pragma unroll
      for (int t = 0; t < 16; t++) v[t] = mkv(spec_windowed<DT>(wv[t], g[t]), 0.0f);
      pk_dft16(v, K, H);
      xf_store1(cur, xa, xa.s1, v);
    }
    __syncthreads();
    if (pending && j == 0) spec_emit_peak(p, slot, unit - 1);
    xf_fwd2(cur, oth, tw2t, xa, j, K, H);
    if (more) {                            // a whole pass ahead of its use
      if (++fr.f == p.n_frames) {
        fr.f = 0;
        ++fr.m;
      }
      spec_load(p, fr, j, g);
    }
    __syncthreads();                       // (thread 0 has read `slot` in front of it)
    float* const dst = p.out + unit * p.out_stride;
    float best = -INFINITY;
    int best_k = kSpecNoBin;
    v2f z[2][8];
#pragma unroll
    for (int h = 0; h < 2; h++) xf_fwd3<true>(oth, z[h], h, w3r[h], t3a, t3b, t3c, j, K, H);
    // ascending bins: j, j + 128, j + 256, ..., j + 896, and thread 0's bin 1024
#pragma unroll
    for (int t = 0; t < 5; t++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (t == 4 && h == 1) continue;
        const int k = j + kXfThreads * h + 256 * t;
        const int o = k - p.bin_first;
        if ((t < 4 || j == 0) && (unsigned)o < (unsigned)p.n_bins) {
          const float val = spec_value(z[h][t], k, p);
          dst[o] = val;
          if (val > best) {
            best = val;
            best_k = k;
          }
        }
      }
    if (peaks) {                           // (workgroup-uniform)
      spec_wave_first_max(best, best_k);
      if ((j & 63) == 0) {
        slot[2 * (j >> 6)] = best;
        slot[2 * (j >> 6) + 1] = __int_as_float(best_k);
      }
      pending = true;
    }
    if (!more) break;
    ++unit;
  }
  if (pending) {
    __syncthreads();
    if (j == 0) spec_emit_peak(p, slot, unit);
  }
}

}  // namespace

int resident_blocks_per_cu(int dtype) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (dtype) {
    case DT_F32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spec_kernel<DT_F32>, THREADS, 0); break;
    case DT_I32: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, spec_kernel<DT_I32>, THREADS, 0); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int launch_spectra(int dtype, unsigned grid, void* stream, const Params& p) {
  hipStream_t hs = (hipStream_t)stream;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(spec_kernel<DT_F32>, dim3(grid), dim3(THREADS), 0, hs, p); break;
    case DT_I32: hipLaunchKernelGGL(spec_kernel<DT_I32>, dim3(grid), dim3(THREADS), 0, hs, p); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace uc_spec_dev
