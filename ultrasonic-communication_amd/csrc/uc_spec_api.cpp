// uc_spec_api.cpp -- the C-ABI of include/uchirp_spec.h on top of uc_spec_kernel.hip: the frame count, the checks of a
// parameter struct, the object with its window and twiddle table, the launch.  The object's base, create and destroy, the
// grid and the checks of the row matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library
// boundary): libuchirp_spec.so stands alone.  A call reads no host array but its parameter struct, which travels as kernel
// arguments, so nothing is staged and the base's staging slots stay empty: a call leaves no event behind, and what must
// wait for the object's calls (uc_spec_set_window, uc_spec_destroy) waits for the device, whatever streams they were given.
// No CPU compute path exists here: without a usable HIP device uc_spec_create fails.  Every entry point leaves the calling
// thread's current HIP device as it found it.
#include "../../include/uchirp_spec.h"
#include "uc_host.hpp"
#include "uc_spec.hpp"

using namespace uc_spec_dev;

static_assert(sizeof(uc_spec_params) == 56 && sizeof(uc_spec_info) == 32 && sizeof(uc_spec_peak) == 8 && sizeof(Peak) == 8, "layouts of uchirp_spec.h");
static_assert(UC_SPEC_DTYPE_I32 == DT_I32 && UC_SPEC_DTYPE_F32 == DT_F32, "dtype values");
static_assert(UC_SPEC_MAG == MAG && UC_SPEC_POWER == POWER && UC_SPEC_DB == DB, "kinds");
static_assert(UC_SPEC_POINTS == POINTS && UC_SPEC_BINS == BINS, "the kernel's constants");

struct uc_spec : HostBase {
  float* tw = nullptr;             // device: exp(-2 pi i k / 2048), k < 2048
  float* window = nullptr;         // device: POINTS floats, the first window_len of them the window
  uint32_t window_len = 0;
};

namespace {

constexpr uint64_t N_IN_MAX = 1ull << 40;
constexpr uint64_t UNITS_MAX = 1ull << 40;

// the frames of the definition, or the code of fail()
int64_t count_frames(const char* who, uint64_t n_in, int64_t first, uint32_t frame_len, uint32_t hop) {
  if (n_in == 0 || n_in > N_IN_MAX) return fail(-EINVAL, "%s: n_in %llu not in 1 .. 2^40", who, (unsigned long long)n_in);
  if (frame_len < 1 || frame_len > (uint32_t)POINTS) return fail(-EINVAL, "%s: frame_len %u not in 1 .. %d", who, frame_len, POINTS);
  if (hop == 0) return fail(-EINVAL, "%s: hop is 0", who);
  if (first <= -(int64_t)frame_len || first >= (int64_t)n_in)
    return fail(-EINVAL, "%s: first %lld not above -frame_len = -%u and below n_in = %llu", who, (long long)first, frame_len, (unsigned long long)n_in);
  return ((int64_t)n_in - first + (int64_t)hop - 1) / (int64_t)hop;     // below 2^41
}

// what uc_spec_plan checks; *info is written on success only
int make_plan(const char* who, const uc_spec_params* q, size_t n_rows, size_t n_in, size_t out_stride, uc_spec_info* info) {
  if (!q) return fail(-EINVAL, "%s: params is NULL", who);
  if (int rc = check_count(who, "n_rows", n_rows)) return rc;
  const int64_t frames = count_frames(who, n_in, q->first, q->frame_len, q->hop);
  if (frames < 0) return (int)frames;
  if (q->n_frames > (uint64_t)frames) return fail(-EINVAL, "%s: n_frames %llu > the %lld frames of the row", who, (unsigned long long)q->n_frames, (long long)frames);
  const uint64_t n_frames = q->n_frames ? q->n_frames : (uint64_t)frames;
  if (q->n_bins == 0 || q->bin_first >= (uint32_t)BINS || q->n_bins > (uint32_t)BINS - q->bin_first)
    return fail(-EINVAL, "%s: bins %u .. %u + %u - 1 not a range inside 0 .. %d", who, q->bin_first, q->bin_first, q->n_bins, BINS - 1);
  if (int rc = check_stride(who, "out_stride", out_stride, "n_bins", q->n_bins)) return rc;
  if (q->kind != MAG && q->kind != POWER && q->kind != DB) return fail(-EINVAL, "%s: unknown kind %d", who, q->kind);
  if (!std::isfinite(q->scale) || !std::isfinite(q->db_mul)) return fail(-EINVAL, "%s: scale or db_mul is not finite", who);
  if (!std::isfinite(q->floor) || !(q->floor > 0.0f)) return fail(-EINVAL, "%s: floor must be finite and above 0", who);
  if (q->reserved != 0) return fail(-EINVAL, "%s: reserved is not 0", who);
  const uint64_t ostride = stride_or(out_stride, q->n_bins);
  if (ostride > STRIDE_MAX) return fail(-EINVAL, "%s: stride too large", who);
  if (n_frames > UNITS_MAX / n_rows) return fail(-EINVAL, "%s: n_rows * n_frames above 2^40", who);
  const uint64_t n_units = (uint64_t)n_rows * n_frames;
  if (n_units > (1ull << 58) / ostride) return fail(-EINVAL, "%s: n_rows * n_frames * out_stride too large", who);
  info->n_frames = n_frames;
  info->out_stride = ostride;
  info->out_elems = (n_units - 1) * ostride + q->n_bins;
  info->bin_first = q->bin_first;
  info->n_bins = q->n_bins;
  return 0;
}

}  // namespace

extern "C" {

int uc_spec_abi_version(void) { return UC_SPEC_ABI_VERSION; }

const char* uc_spec_last_error(void) { return g_err.c_str(); }

int64_t uc_spec_frames(uint64_t n_in, int64_t first, uint32_t frame_len, uint32_t hop) {
  return count_frames("uc_spec_frames", n_in, first, frame_len, hop);
}

int uc_spec_plan(const uc_spec_params* params, size_t n_rows, size_t n_in, size_t out_stride, uc_spec_info* info) {
  if (!info) return fail(-EINVAL, "uc_spec_plan: info is NULL");
  uc_spec_info f;
  if (int rc = make_plan("uc_spec_plan", params, n_rows, n_in, out_stride, &f)) return rc;
  *info = f;
  return 0;
}

int uc_spec_create(int device, uc_spec** out) {
  DeviceGuard guard;
  int rc = open("uc_spec_create", "UC_SPEC_GRID", device, out);
  if (rc) return rc;
  uc_spec* l = *out;
  rc = device_twiddles(&l->tw, POINTS, "uc_spec_create");
  if (!rc) {
    const hipError_t e = hipMalloc((void**)&l->window, POINTS * sizeof(float));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      l->window = nullptr;
      rc = fail(-ENOMEM, "uc_spec_create: the window: %s", hipGetErrorString(e));
    }
  }
  if (!rc) rc = uc_spec_set_window(l, nullptr, POINTS);
  if (rc) {
    const std::string keep = g_err;
    uc_spec_destroy(l);
    g_err = keep;
    *out = nullptr;
  }
  return rc;
}

void uc_spec_destroy(uc_spec* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  (void)hipDeviceSynchronize();      // the calls stage nothing and leave no event to wait for
  if (l->window) (void)hipFree(l->window);
  if (l->tw) (void)hipFree(l->tw);
  delete l;
}

int uc_spec_set_window(uc_spec* l, const float* window, size_t len) {
  if (!l) return fail(-EINVAL, "uc_spec_set_window: spec is NULL");
  if (len < 1 || len > (size_t)POINTS) return fail(-EINVAL, "uc_spec_set_window: len %zu not in 1 .. %d", len, POINTS);
  std::vector<float> w(POINTS, 0.0f);
  for (size_t i = 0; i < len; ++i) {
    w[i] = window ? window[i] : (float)(0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * (double)i / (double)len));
    if (!std::isfinite(w[i])) return fail(-EINVAL, "uc_spec_set_window: window[%zu] is not finite", i);
  }
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, "uc_spec_set_window", "hipSetDevice");
  // no launch may still read the old window, on whatever stream it was enqueued (an event behind the last launch would
  // cover that launch's stream only: nothing orders one call behind the call before)
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "uc_spec_set_window", "hipDeviceSynchronize");
  // (pageable memory: done when the call returns)
  if ((e = hipMemcpy(l->window, w.data(), POINTS * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
    return hip_fail(e, "uc_spec_set_window", "hipMemcpy");
  l->window_len = (uint32_t)len;
  return 0;
}

int uc_spec_run(uc_spec* l, const void* in_dev, int in_dtype, size_t n_rows, size_t n_in, size_t in_stride, const uc_spec_params* params,
                float* out_dev, size_t out_stride, uc_spec_peak* peaks_dev, void* hip_stream) {
  static const char WHO[] = "uc_spec_run";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_spec_run: spec is NULL");
  if (!in_dev || !out_dev) return fail(-EINVAL, "uc_spec_run: in_dev or out_dev is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  uc_spec_info f;
  if (int rc = make_plan(WHO, params, n_rows, n_in, out_stride, &f)) return rc;
  const size_t istride = stride_or(in_stride, n_in);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_strides_max(WHO, istride, f.out_stride)) return rc;
  if (n_rows > (1ull << 58) / istride) return fail(-EINVAL, "uc_spec_run: n_rows * in_stride too large");
  const uint64_t n_units = (uint64_t)n_rows * f.n_frames;
  const size_t in_bytes = span_bytes(n_rows, istride, n_in, 4), out_bytes = (size_t)f.out_elems * 4, peak_bytes = (size_t)n_units * sizeof(Peak);
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, out_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (peaks_dev) {
    if (int rc = check_disjoint(WHO, "peaks_dev", peaks_dev, peak_bytes, "in_dev", in_dev, in_bytes)) return rc;
    if (int rc = check_disjoint(WHO, "peaks_dev", peaks_dev, peak_bytes, "out_dev", out_dev, out_bytes)) return rc;
  }
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  if (peaks_dev)
    if (int rc = check_on_device(WHO, "peaks_dev", peaks_dev, l->device)) return rc;
  // (the first check that reads the object's own fields)
  if (params->frame_len != l->window_len)
    return fail(-EINVAL, "uc_spec_run: frame_len %u is not the length of the object's window, %u", params->frame_len, l->window_len);

  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.tw = l->tw;
  p.window = l->window;
  p.out = out_dev;
  p.peaks = (Peak*)peaks_dev;
  p.n_in = (int64_t)n_in;
  p.first = params->first;
  p.in_stride = istride;
  p.out_stride = f.out_stride;
  p.n_units = n_units;
  p.n_frames = f.n_frames;
  p.hop = params->hop;
  p.frame_len = (int32_t)params->frame_len;
  p.bin_first = (int32_t)params->bin_first;
  p.n_bins = (int32_t)params->n_bins;
  p.ac_bins = params->ac_bins > (uint32_t)BINS ? BINS : (int32_t)params->ac_bins;
  p.kind = params->kind;
  p.scale = params->scale;
  p.floor = params->floor;
  p.db_mul = params->db_mul;
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 4, n_units);

  // ---- enqueue: the only launch
  e = (hipError_t)launch_spectra(in_dtype, (unsigned)grid, (hipStream_t)hip_stream, p);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  return 0;
}

}  // extern "C"
