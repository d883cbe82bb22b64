// uc_mic_api.cpp -- the C-ABI of include/uchirp_mic.h on top of uc_mic_kernel.hip: the two host functions of the definition
// (the quantiser and one row of the modulator, on the arithmetic of uc_mic.hpp that the kernel compiles too), the checks
// that are its own, the launch.  The object's base, create and destroy and the checks of the row matrices are the shared host
// layer's (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_mic.so stands alone.  A call reads no
// host array, so the base's staging slots stay empty.  No CPU compute path exists behind uc_mic_modulate: without a usable
// HIP device uc_mic_create fails.  Every entry point leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_mic.h"
#include "uc_host.hpp"
#include "uc_mic.hpp"

using namespace uc_mic_dev;

static_assert(UC_MIC_DTYPE_I32 == DT_I32 && UC_MIC_DTYPE_F32 == DT_F32, "dtype values");
static_assert(UC_MIC_Q_MAX == Q_MAX && UC_MIC_Y == Y && UC_MIC_OSR == 32, "constants of uchirp_mic.h");

struct uc_mic : HostBase {
  float scale = 1.0f;
};

namespace {

bool scale_ok(float scale) { return std::isfinite(scale) && scale > 0.0f; }

bool on_16_bytes(const void* p, size_t stride) { return ((uintptr_t)p & 15u) == 0 && (stride & 3u) == 0; }

}  // namespace

extern "C" {

int uc_mic_abi_version(void) { return UC_MIC_ABI_VERSION; }

const char* uc_mic_last_error(void) { return g_err.c_str(); }

int uc_mic_quantise(const void* in, int dtype, float scale, size_t n, int32_t* q_out) {
  static const char WHO[] = "uc_mic_quantise";
  if (!in || !q_out) return fail(-EINVAL, "uc_mic_quantise: in or q_out is NULL");
  if (int rc = check_dtype(WHO, dtype)) return rc;
  if (n == 0) return fail(-EINVAL, "uc_mic_quantise: n is 0");
  if (dtype == DT_F32) {
    if (!scale_ok(scale)) return fail(-EINVAL, "uc_mic_quantise: scale must be finite and positive");
    const float* x = (const float*)in;
    for (size_t i = 0; i < n; ++i) q_out[i] = quantise_f32(x[i], scale);
  } else {
    const int32_t* w = (const int32_t*)in;
    for (size_t i = 0; i < n; ++i) q_out[i] = quantise_i32(w[i]);
  }
  return 0;
}

int uc_mic_modulate_row(const int32_t* q, size_t n, int32_t state[4], uint32_t* words_out) {
  if (!q || !state || !words_out) return fail(-EINVAL, "uc_mic_modulate_row: q, state or words_out is NULL");
  if (n == 0) return fail(-EINVAL, "uc_mic_modulate_row: n is 0");
  State s = {(uint32_t)state[0], (uint32_t)state[1], (uint32_t)state[2]};
  for (size_t i = 0; i < n; ++i) words_out[i] = modulate_sample(s, q[i]);
  state[0] = (int32_t)s.prev;
  state[1] = (int32_t)s.s1;
  state[2] = (int32_t)s.s2;
  state[3] = 0;
  return 0;
}

int uc_mic_create(int device, float scale, uc_mic** out) {
  if (!out) return fail(-EINVAL, "uc_mic_create: out is NULL");
  *out = nullptr;
  if (!scale_ok(scale)) return fail(-EINVAL, "uc_mic_create: scale must be finite and positive");
  DeviceGuard guard;
  int rc = open("uc_mic_create", "UC_MIC_GRID", device, out);
  if (rc) return rc;
  (*out)->scale = scale;
  return 0;
}

void uc_mic_destroy(uc_mic* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  delete l;
}

int uc_mic_modulate(uc_mic* l, const void* in_dev, int in_dtype, size_t n_rows, size_t n_samples, size_t in_stride, int32_t* state_dev,
                    uint32_t* out_dev, size_t out_stride, void* hip_stream) {
  static const char WHO[] = "uc_mic_modulate";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_mic_modulate: mic is NULL");
  if (!in_dev || !state_dev || !out_dev) return fail(-EINVAL, "uc_mic_modulate: in_dev, state_dev or out_dev is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (n_samples == 0) return fail(-EINVAL, "uc_mic_modulate: n_samples is 0");
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_samples", n_samples)) return rc;
  if (int rc = check_stride(WHO, "out_stride", out_stride, "n_samples", n_samples)) return rc;
  const size_t istride = stride_or(in_stride, n_samples), ostride = stride_or(out_stride, n_samples);
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_rows, istride, n_rows, ostride, 1ull << 58, "n_rows * out_stride")) return rc;
  if ((((uintptr_t)in_dev | (uintptr_t)state_dev | (uintptr_t)out_dev) & 3u) != 0)
    return fail(-EINVAL, "uc_mic_modulate: in_dev, state_dev or out_dev is not a multiple of 4");
  const size_t in_bytes = span_bytes(n_rows, istride, n_samples, 4), out_bytes = span_bytes(n_rows, ostride, n_samples, 4);
  const size_t state_bytes = n_rows * 16;
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, out_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "out_dev", out_dev, out_bytes)) return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "state_dev", state_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;

  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.out = out_dev;
  p.state = state_dev;
  p.in_stride = istride;
  p.out_stride = ostride;
  p.n_samples = n_samples;
  p.n_rows = (uint32_t)n_rows;
  p.row_blocks = (uint32_t)((n_rows + LANES - 1) / LANES);
  p.scale = l->scale;
  // a single row has no second row for its stride to misplace
  p.in_vec = on_16_bytes(in_dev, n_rows > 1 ? istride : 0) ? 1u : 0u;
  p.out_vec = on_16_bytes(out_dev, n_rows > 1 ? ostride : 0) ? 1u : 0u;
  // one one-wave workgroup per 64 rows; UC_MIC_GRID (under UC_TUNING=1) makes fewer of them walk the row blocks
  unsigned grid = p.row_blocks;
  if (l->grid_override && l->grid_override < grid) grid = l->grid_override;

  // ---- enqueue
  e = (hipError_t)launch_modulate(in_dtype, grid, hip_stream, p);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  return 0;
}

}  // extern "C"
