// uc_xform_split.hpp -- the two halves of xf_fwd3_h_invA (uc_xform.hpp) as passes of their own, for kernels that keep the
// SPECTRUM in registers between the forward and the inverse transform (uc_xcorr_kernel.hip adds the cross-spectra of
// several segments before it goes back).  Same butterflies, same twiddles, same LDS layouts: xf_fwd2 feeds xf_fwd3,
// xf_invA feeds xf_invB.
#pragma once
#include "uc_xform.hpp"

namespace uc {

// forward pass 3 (full radix-8) of butterfly b = j + 128 h: z[t] = X[b + 256 t], t = 0..7, in natural order.
// RESIDENT: the twiddles W_2048^(t b) come from w3 (kept in registers by the caller), else they are derived per call.
template <bool RESIDENT>
__device__ __forceinline__ void xf_fwd3(const float* src, v2f (&z)[8], int h, const v2f (&w3)[8], v2f t3a, v2f t3b, v2f t3c,
                                        int j, v2f K, v2f H) {
  const int b = j + kXfThreads * h;
  v2f u[8];
#pragma unroll
  for (int t = 0; t < 8; t++) u[t] = lds_ld(src, b + 256 * t);
  __builtin_amdgcn_sched_barrier(0);
  v2f w[8];
  if (RESIDENT) {
#pragma unroll
    for (int t = 1; t < 8; t++) w[t] = w3[t];
  } else {
    xf_twiddles3(w, h, t3a, t3b, t3c, K, H);
  }
#pragma unroll
  for (int t = 1; t < 8; t++) u[t] = pk_cmul(u[t], w[t]);
  pk_dft8(u, H);
#pragma unroll
  for (int t = 0; t < 8; t++) z[t] = u[pk_slot8(t)];
}

// inverse pass A (radix-8, no twiddles) of butterfly b: c[t] = X[b + 256 t] in natural order -> inverse exchange A
__device__ __forceinline__ void xf_invA(float* dst, const v2f (&c)[8], int b, v2f H) {
  v2f g[8];
#pragma unroll
  for (int t = 0; t < 8; t++) g[t] = c[t];
  pk_dft8(g, H);
  // IDFT8[t] = DFT8[(8 - t) & 7]; element 8 b + t, swizzled phys = o ^ ((o >> 4) & 7)
  UC_XF_PRIO(0);
#pragma unroll
  for (int t = 0; t < 8; t++) lds_st(dst, 8 * b + (t ^ ((b >> 1) & 7)), g[pk_slot8((8 - t) & 7)]);
  UC_XF_PRIO(2);
}

}  // namespace uc
