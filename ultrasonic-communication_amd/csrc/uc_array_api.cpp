// uc_array_api.cpp -- the C-ABI of include/uchirp_array.h on top of uc_array_kernel.hip: errors, the object and its
// staging buffers, the coefficients, argument checks, the launch.  Built like uc_scene_api.cpp, with the same host-side
// helpers (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_array.so stands alone.  No CPU
// compute path exists here: without a usable HIP device uc_array_create fails.  Every entry point leaves the calling
// thread's current HIP device as it found it.
#include "../../include/uchirp_array.h"
#include "uc_array.hpp"
#include "uc_host.hpp"

using namespace uc_array_dev;

static_assert(sizeof(uc_array_tap) == 16 && sizeof(uc_array_beam) == 8 && sizeof(Beam) == sizeof(uc_array_beam), "layouts of uchirp_array.h");
static_assert(sizeof(Tap) == 80 && UC_ARRAY_MAX_TAPS == MAX_TAPS && UC_ARRAY_COEFS == COEFS, "the kernel's tap record");
static_assert(UC_ARRAY_DTYPE_I32 == DT_I32 && UC_ARRAY_DTYPE_F32 == DT_F32, "dtype values");

struct uc_array {
  int device = 0;
  int cus = 0;
  unsigned grid_override = 0;      // UC_ARRAY_GRID under UC_TUNING=1
  int resident[2] = {0, 0};        // by dtype: workgroups one CU holds at once (asked once per format)
  // staging: [n_taps Tap records][n_beams Beam records], pinned on the host and its twin on the device.  Two such pairs,
  // used in turn: call k stages while call k - 1's copy still waits in its stream.
  StagingSlot slot[2];
  unsigned next = 0;
};

namespace {

constexpr double DELAY_MAX = 1073741824.0;   // 2^30

// I0(x), the modified Bessel function of order 0, by its power series: sum ((x / 2)^2k / (k!)^2); x is 0 .. 8 here
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

bool tap_ok(double delay, float weight) { return std::isfinite(delay) && std::isfinite(weight) && std::fabs(delay) <= DELAY_MAX; }

// the coefficients of the definition (include/uchirp_array.h); the arguments are checked by the caller
void coefficients(double delay, float weight, int64_t* shift, float c[COEFS]) {
  double whole = std::floor(delay);
  double f = delay - whole;
  if (f >= 1.0) {   // a tiny negative delay: the subtraction rounded up
    whole += 1.0;
    f = 0.0;
  }
  *shift = (int64_t)whole - 7;
  if (f == 0.0) {
    for (int t = 0; t < COEFS; ++t) c[t] = 0.0f;
    c[7] = weight;
    return;
  }
  const double pi = 3.14159265358979323846;
  const double i0_beta = bessel_i0(8.0);
  for (int t = 0; t < COEFS; ++t) {
    const double u = (double)(t - 7) - f;
    const double r = u / 8.0;
    c[t] = (float)((double)weight * (std::sin(pi * u) / (pi * u)) * bessel_i0(8.0 * std::sqrt(1.0 - r * r)) / i0_beta);
  }
}

}  // namespace

extern "C" {

int uc_array_abi_version(void) { return UC_ARRAY_ABI_VERSION; }

const char* uc_array_last_error(void) { return g_err.c_str(); }

int uc_array_tap_coefficients(double delay_samples, float weight, int64_t* shift, float coef[UC_ARRAY_COEFS]) {
  if (!shift || !coef) return fail(-EINVAL, "uc_array_tap_coefficients: shift or coef is NULL");
  if (!tap_ok(delay_samples, weight))
    return fail(-EINVAL, "uc_array_tap_coefficients: delay_samples and weight must be finite, |delay_samples| <= 2^30");
  coefficients(delay_samples, weight, shift, coef);
  return 0;
}

int uc_array_create(int device, uc_array** out) {
  if (!out) return fail(-EINVAL, "uc_array_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(-ENODEV, "uc_array_create: no HIP device (%s); this library has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "0 devices");
  }
  if (device < 0 || device >= ndev) return fail(-ENODEV, "uc_array_create: device %d out of range [0,%d)", device, ndev);
  DeviceGuard guard;
  if ((e = hipSetDevice(device)) != hipSuccess) return hip_fail(e, "uc_array_create: hipSetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(e, "uc_array_create: hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(-ENODEV, "uc_array_create: device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
  uc_array* l = new uc_array();
  l->device = device;
  l->cus = prop.multiProcessorCount;
  // experiment switches are read only under UC_TUNING=1, so that a stray variable in a production environment changes nothing
  const char* tuning = getenv("UC_TUNING");
  if (tuning && !strcmp(tuning, "1")) {
    const char* g = getenv("UC_ARRAY_GRID");
    if (g && atoi(g) > 0) l->grid_override = (unsigned)atoi(g);
  }
  for (StagingSlot& sl : l->slot)
    if ((e = hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)) != hipSuccess) {
      uc_array_destroy(l);
      return hip_fail(e, "uc_array_create: hipEventCreate");
    }
  *out = l;
  return 0;
}

void uc_array_destroy(uc_array* l) {
  if (!l) return;
  DeviceGuard guard;
  (void)hipSetDevice(l->device);
  for (StagingSlot& sl : l->slot) {
    if (sl.in_flight) (void)hipEventSynchronize(sl.done);
    if (sl.pinned) (void)hipHostFree(sl.pinned);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.copied) (void)hipEventDestroy(sl.copied);
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
  delete l;
}

int uc_array_combine(uc_array* l, const void* in_dev, int in_dtype, size_t n_mics, uint64_t in_first, size_t n_in, size_t in_stride,
                     const uc_array_tap* taps, size_t n_taps, const uc_array_beam* beams, size_t n_beams, float* out_dev,
                     uint64_t out_first, size_t n_out, size_t out_stride, void* hip_stream) {
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_array_combine: array is NULL");
  if (!in_dev || !out_dev) return fail(-EINVAL, "uc_array_combine: in_dev or out_dev is NULL");
  if (!taps || !beams) return fail(-EINVAL, "uc_array_combine: taps or beams is NULL");
  if (in_dtype != UC_ARRAY_DTYPE_I32 && in_dtype != UC_ARRAY_DTYPE_F32) return fail(-EINVAL, "uc_array_combine: unknown dtype %d", in_dtype);
  if (n_mics == 0 || n_mics > 0xFFFFFFFFull) return fail(-EINVAL, "uc_array_combine: n_mics %zu out of range", n_mics);
  if (n_taps == 0 || n_taps > 0xFFFFFFFFull) return fail(-EINVAL, "uc_array_combine: n_taps %zu out of range", n_taps);
  if (n_beams == 0 || n_beams > 0xFFFFFFFFull) return fail(-EINVAL, "uc_array_combine: n_beams %zu out of range", n_beams);
  if (n_in == 0 || n_out == 0) return fail(-EINVAL, "uc_array_combine: n_in or n_out is 0");
  if (in_first > (1ull << 52) || out_first > (1ull << 52) || n_in > (1ull << 40) || n_out > (1ull << 40))
    return fail(-EINVAL, "uc_array_combine: sample range too large");
  const size_t istride = in_stride ? in_stride : n_in, ostride = out_stride ? out_stride : n_out;
  if (istride < n_in) return fail(-EINVAL, "uc_array_combine: in_stride %zu < n_in %zu", in_stride, n_in);
  if (ostride < n_out) return fail(-EINVAL, "uc_array_combine: out_stride %zu < n_out %zu", out_stride, n_out);
  if (istride > (1ull << 40) || ostride > (1ull << 40)) return fail(-EINVAL, "uc_array_combine: stride too large");
  // counts are below 2^32 and strides at most 2^40, so the products below cannot wrap; a buffer of 2^60 bytes is no buffer
  if ((uint64_t)n_mics * istride > (1ull << 58) || (uint64_t)n_beams * ostride > (1ull << 58))
    return fail(-EINVAL, "uc_array_combine: n_mics * in_stride or n_beams * out_stride too large");
  for (size_t k = 0; k < n_taps; ++k) {
    const uc_array_tap& q = taps[k];
    if (q.mic >= n_mics) return fail(-EINVAL, "uc_array_combine: tap %zu: mic %u >= n_mics %zu", k, q.mic, n_mics);
    if (!tap_ok(q.delay_samples, q.weight))
      return fail(-EINVAL, "uc_array_combine: tap %zu: delay_samples and weight must be finite, |delay_samples| <= 2^30", k);
  }
  for (size_t b = 0; b < n_beams; ++b) {
    const uc_array_beam& q = beams[b];
    if (q.n_taps == 0 || q.n_taps > UC_ARRAY_MAX_TAPS)
      return fail(-EINVAL, "uc_array_combine: beam %zu: n_taps %u not in 1 .. %d", b, q.n_taps, UC_ARRAY_MAX_TAPS);
    if ((uint64_t)q.first_tap + q.n_taps > n_taps)
      return fail(-EINVAL, "uc_array_combine: beam %zu: taps [%u, %u + %u) beyond n_taps %zu", b, q.first_tap, q.first_tap, q.n_taps, n_taps);
  }
  const uintptr_t ia = (uintptr_t)in_dev, ib = ia + ((n_mics - 1) * istride + n_in) * 4;
  const uintptr_t oa = (uintptr_t)out_dev, ob = oa + ((n_beams - 1) * ostride + n_out) * 4;
  if (oa < ib && ia < ob) return fail(-EINVAL, "uc_array_combine: out_dev overlaps in_dev");
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, "uc_array_combine: hipSetDevice");
  if (device_of(in_dev) != l->device) return fail(-EINVAL, "uc_array_combine: in_dev is not device memory of device %d", l->device);
  if (device_of(out_dev) != l->device) return fail(-EINVAL, "uc_array_combine: out_dev is not device memory of device %d", l->device);
  const size_t tap_bytes = n_taps * sizeof(Tap), bytes = tap_bytes + n_beams * sizeof(Beam);
  StagingSlot& sl = l->slot[l->next];
  int rc = reserve(&sl, bytes, "uc_array_combine");
  if (rc) return rc;

  // ---- stage (this slot's pinned buffer is free once the copy of two calls back has run)
  if (sl.in_flight) (void)hipEventSynchronize(sl.copied);
  Tap* trec = (Tap*)sl.pinned;
  for (size_t k = 0; k < n_taps; ++k) {
    coefficients(taps[k].delay_samples, taps[k].weight, &trec[k].shift, trec[k].c);
    trec[k].row = (uint64_t)taps[k].mic * istride;
  }
  memcpy((char*)sl.pinned + tap_bytes, beams, n_beams * sizeof(Beam));
  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.out = out_dev;
  p.in_first = (int64_t)in_first;
  p.n_in = (int64_t)n_in;
  p.out_first = (int64_t)out_first;
  p.n_out = (int64_t)n_out;
  p.out_stride = ostride;
  const uint64_t tiles_per_beam = (n_out + TILE_SAMPLES - 1) / TILE_SAMPLES;
  p.tiles_per_beam = (uint32_t)tiles_per_beam;
  p.n_beams = (uint32_t)n_beams;
  const uint64_t n_tiles = (uint64_t)n_beams * tiles_per_beam;
  // a persistent grid of exactly the workgroups the chip holds at once (the tiles are dealt statically); the runtime's
  // occupancy figure is asked, not assumed
  if (!l->resident[in_dtype]) {
    const int r = resident_blocks_per_cu(in_dtype);
    l->resident[in_dtype] = r > 0 ? r : 8;
  }
  uint64_t grid = (uint64_t)l->cus * (uint64_t)l->resident[in_dtype];
  if (l->grid_override) grid = l->grid_override;
  if (grid > n_tiles) grid = n_tiles;

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (sl.in_flight && (e = hipStreamWaitEvent(hs, sl.done, 0)) != hipSuccess) return hip_fail(e, "uc_array_combine: hipStreamWaitEvent");
  if ((e = hipMemcpyAsync(sl.dev, sl.pinned, bytes, hipMemcpyHostToDevice, hs)) != hipSuccess)
    return hip_fail(e, "uc_array_combine: hipMemcpyAsync");
  (void)hipEventRecord(sl.copied, hs);
  const char* d = (const char*)sl.dev;
  e = (hipError_t)launch_combine(in_dtype, (unsigned)grid, hs, p, (const Beam*)(d + tap_bytes), (const Tap*)d);
  (void)hipEventRecord(sl.done, hs);
  sl.in_flight = true;
  l->next ^= 1u;
  if (e != hipSuccess) return hip_fail(e, "uc_array_combine: launch");
  return 0;
}

}  // extern "C"
