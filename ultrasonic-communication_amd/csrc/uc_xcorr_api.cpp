// uc_xcorr_api.cpp -- the C-ABI of include/uchirp_xcorr.h on top of uc_xcorr_kernel.hip: errors, the object, its twiddle
// table, staging buffers and unit sums, the peak rule, argument checks, the launches.  Built like uc_align_api.cpp, with the same
// host-side helpers (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_xcorr.so stands alone.  No
// CPU compute path exists here: without a usable HIP device uc_xcorr_create fails.  Every entry point leaves the calling
// thread's current HIP device as it found it.
#include "../../include/uchirp_xcorr.h"
#include "uc_xcorr.hpp"
#include "uc_host.hpp"

#include <vector>

using namespace uc_xcorr_dev;

static_assert(sizeof(uc_xcorr_pair) == 8 && sizeof(uc_xcorr_peak_t) == 32 && sizeof(Pair) == 16, "layouts of uchirp_xcorr.h");
static_assert(UC_XCORR_MAX_LAG == MAX_LAG && UC_XCORR_POINTS == POINTS && UC_XCORR_GROUP == GROUP, "the kernel's constants");
static_assert(POINTS - 2 * MAX_LAG >= MAX_LAG, "only a row's first segment can start in front of the row");
static_assert(UC_XCORR_DTYPE_I32 == DT_I32 && UC_XCORR_DTYPE_F32 == DT_F32, "dtype values");

// the unit sums of one call (device memory only); one per staging slot, so that call k never writes what call k - 1 reads
struct PartSlot {
  float* dev = nullptr;
  size_t cap = 0;   // bytes
};

struct uc_xcorr {
  int device = 0;
  int cus = 0;
  unsigned grid_override = 0;      // UC_XCORR_GRID under UC_TUNING=1
  int resident[2] = {0, 0};        // by dtype: workgroups one CU holds at once (asked once per format)
  float* tw = nullptr;             // device: exp(-2 pi i k / 2048), k < 2048
  // staging: [n_pairs Pair records], pinned on the host and its twin on the device.  Two such pairs, used in turn: call k
  // stages while call k - 1's copy still waits in its stream.
  StagingSlot slot[2];
  PartSlot part[2];
  unsigned next = 0;
};

namespace {

// the slot's unit sums hold at least `bytes`; called before anything of the call is enqueued
int reserve_part(PartSlot* ps, StagingSlot* sl, size_t bytes) {
  if (bytes <= ps->cap) return 0;
  size_t cap = ps->cap ? ps->cap : (size_t)1 << 16;
  while (cap < bytes) cap *= 2;
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, cap);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(-ENOMEM, "uc_xcorr_correlate: %zu bytes of unit sums: %s", cap, hipGetErrorString(e));
  }
  if (sl->in_flight) (void)hipEventSynchronize(sl->done);  // the old buffer may still be read
  if (ps->dev) (void)hipFree(ps->dev);
  ps->dev = (float*)d;
  ps->cap = cap;
  return 0;
}

}  // namespace

extern "C" {

int uc_xcorr_abi_version(void) { return UC_XCORR_ABI_VERSION; }

const char* uc_xcorr_last_error(void) { return g_err.c_str(); }

int uc_xcorr_peak(const double* r, uint32_t max_lag, uc_xcorr_peak_t* out) {
  if (!r || !out) return fail(-EINVAL, "uc_xcorr_peak: corr or out is NULL");
  if (max_lag < 1 || max_lag > UC_XCORR_MAX_LAG) return fail(-EINVAL, "uc_xcorr_peak: max_lag %u not in 1 .. %d", max_lag, UC_XCORR_MAX_LAG);
  const int L = (int)max_lag, last = 2 * L;
  int largest = 0;
  for (int k = 0; k <= last; ++k) {
    if (!std::isfinite(r[k])) return fail(-EINVAL, "uc_xcorr_peak: corr[%d] is not finite", k);
    if (r[k] > r[largest]) largest = k;
  }
  double best = 0.0, second = 0.0, best_d = 0.0;
  int best_k = -1;
  for (int k = 1; k < last; ++k) {
    if (!(r[k] > 0.0 && r[k] >= r[k - 1] && r[k] > r[k + 1])) continue;
    const double c = (r[k - 1] + r[k + 1]) / (2.0 * r[k]);
    double height = r[k], d = 0.0;
    if (c > -1.0 && c < 1.0) {
      const double w = std::acos(c);
      const double q = (r[k + 1] - r[k - 1]) / (2.0 * std::sin(w));
      height = std::hypot(r[k], q);
      d = std::atan2(q, r[k]) / w;
    }
    if (best_k < 0 || height > best) {
      if (best_k >= 0) second = best;
      best = height;
      best_d = d;
      best_k = k;
    } else if (height > second) {
      second = height;
    }
  }
  memset(out, 0, sizeof(*out));
  if (largest == 0 || largest == last) out->flags |= UC_XCORR_AT_EDGE;
  if (best_k < 0) {
    out->flags |= UC_XCORR_NO_PEAK;
    return 0;
  }
  out->delay_samples = (double)(best_k - L) + best_d;
  out->height = best;
  out->runner_up = second / best;
  out->lag = best_k - L;
  return 0;
}

int uc_xcorr_create(int device, uc_xcorr** out) {
  if (!out) return fail(-EINVAL, "uc_xcorr_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(-ENODEV, "uc_xcorr_create: no HIP device (%s); this library has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "0 devices");
  }
  if (device < 0 || device >= ndev) return fail(-ENODEV, "uc_xcorr_create: device %d out of range [0,%d)", device, ndev);
  DeviceGuard guard;
  if ((e = hipSetDevice(device)) != hipSuccess) return hip_fail(e, "uc_xcorr_create: hipSetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(e, "uc_xcorr_create: hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(-ENODEV, "uc_xcorr_create: device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
  uc_xcorr* l = new uc_xcorr();
  l->device = device;
  l->cus = prop.multiProcessorCount;
  // experiment switches are read only under UC_TUNING=1, so that a stray variable in a production environment changes nothing
  const char* tuning = getenv("UC_TUNING");
  if (tuning && !strcmp(tuning, "1")) {
    const char* g = getenv("UC_XCORR_GRID");
    if (g && atoi(g) > 0) l->grid_override = (unsigned)atoi(g);
  }
  {
    // the transform's twiddles, cosine and sine in double, rounded once (as libuchirp.so builds its own)
    std::vector<float> tw(2 * (size_t)POINTS);
    for (int k = 0; k < POINTS; ++k) {
      const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)POINTS;
      tw[2 * k] = (float)std::cos(a);
      tw[2 * k + 1] = (float)std::sin(a);
    }
    if ((e = hipMalloc((void**)&l->tw, tw.size() * sizeof(float))) != hipSuccess) {
      (void)hipGetLastError();
      delete l;
      return fail(-ENOMEM, "uc_xcorr_create: the twiddle table: %s", hipGetErrorString(e));
    }
    if ((e = hipMemcpy(l->tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) {
      uc_xcorr_destroy(l);
      return hip_fail(e, "uc_xcorr_create: hipMemcpy");
    }
  }
  for (StagingSlot& sl : l->slot)
    if ((e = hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)) != hipSuccess) {
      uc_xcorr_destroy(l);
      return hip_fail(e, "uc_xcorr_create: hipEventCreate");
    }
  *out = l;
  return 0;
}

void uc_xcorr_destroy(uc_xcorr* l) {
  if (!l) return;
  DeviceGuard guard;
  (void)hipSetDevice(l->device);
  for (int i = 0; i < 2; ++i) {
    StagingSlot& sl = l->slot[i];
    if (sl.in_flight) (void)hipEventSynchronize(sl.done);
    if (sl.pinned) (void)hipHostFree(sl.pinned);
    if (sl.dev) (void)hipFree(sl.dev);
    if (l->part[i].dev) (void)hipFree(l->part[i].dev);
    if (sl.copied) (void)hipEventDestroy(sl.copied);
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
  if (l->tw) (void)hipFree(l->tw);
  delete l;
}

int uc_xcorr_correlate(uc_xcorr* l, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                       const uc_xcorr_pair* pairs, size_t n_pairs, size_t first, size_t n, uint32_t max_lag, double* corr_dev,
                       size_t corr_stride, void* hip_stream) {
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_xcorr_correlate: xcorr is NULL");
  if (!in_dev || !corr_dev) return fail(-EINVAL, "uc_xcorr_correlate: in_dev or corr_dev is NULL");
  if (!pairs) return fail(-EINVAL, "uc_xcorr_correlate: pairs is NULL");
  if (in_dtype != UC_XCORR_DTYPE_I32 && in_dtype != UC_XCORR_DTYPE_F32) return fail(-EINVAL, "uc_xcorr_correlate: unknown dtype %d", in_dtype);
  if (n_mics == 0 || n_mics > 0xFFFFFFFFull) return fail(-EINVAL, "uc_xcorr_correlate: n_mics %zu out of range", n_mics);
  if (n_pairs == 0 || n_pairs > 0xFFFFFFFFull) return fail(-EINVAL, "uc_xcorr_correlate: n_pairs %zu out of range", n_pairs);
  if (n_in == 0 || n == 0) return fail(-EINVAL, "uc_xcorr_correlate: n_in or n is 0");
  if (n_in > (1ull << 40)) return fail(-EINVAL, "uc_xcorr_correlate: n_in too large");
  if (first > n_in || n > n_in - first) return fail(-EINVAL, "uc_xcorr_correlate: first %zu + n %zu > n_in %zu", first, n, n_in);
  if (max_lag < 1 || max_lag > UC_XCORR_MAX_LAG) return fail(-EINVAL, "uc_xcorr_correlate: max_lag %u not in 1 .. %d", max_lag, UC_XCORR_MAX_LAG);
  const size_t lags = 2 * (size_t)max_lag + 1;
  const size_t istride = in_stride ? in_stride : n_in, cstride = corr_stride ? corr_stride : lags;
  if (istride < n_in) return fail(-EINVAL, "uc_xcorr_correlate: in_stride %zu < n_in %zu", in_stride, n_in);
  if (cstride < lags) return fail(-EINVAL, "uc_xcorr_correlate: corr_stride %zu < 2 max_lag + 1 = %zu", corr_stride, lags);
  if (istride > (1ull << 40) || cstride > (1ull << 40)) return fail(-EINVAL, "uc_xcorr_correlate: stride too large");
  // counts are below 2^32 and strides at most 2^40, so the products below cannot wrap; a buffer of 2^60 bytes is no buffer
  if ((uint64_t)n_mics * istride > (1ull << 58) || (uint64_t)n_pairs * cstride > (1ull << 57))
    return fail(-EINVAL, "uc_xcorr_correlate: n_mics * in_stride or n_pairs * corr_stride too large");
  for (size_t k = 0; k < n_pairs; ++k)
    if (pairs[k].ref >= n_mics || pairs[k].mic >= n_mics)
      return fail(-EINVAL, "uc_xcorr_correlate: pair %zu: rows %u, %u; n_mics %zu", k, pairs[k].ref, pairs[k].mic, n_mics);
  const uintptr_t ia = (uintptr_t)in_dev, ib = ia + ((n_mics - 1) * istride + n_in) * 4;
  const uintptr_t oa = (uintptr_t)corr_dev, ob = oa + ((n_pairs - 1) * cstride + lags) * 8;
  if (oa < ib && ia < ob) return fail(-EINVAL, "uc_xcorr_correlate: corr_dev overlaps in_dev");
  const uint64_t seg = (uint64_t)POINTS - 2 * max_lag;                    // S: 1024 .. 2046
  const uint64_t n_segments = ((uint64_t)n + seg - 1) / seg, n_groups = (n_segments + GROUP - 1) / GROUP;   // < 2^31, 2^29
  const uint64_t n_units = (uint64_t)n_pairs * n_groups;
  if (n_units > (1ull << 36)) return fail(-EINVAL, "uc_xcorr_correlate: n_pairs * segments too large for one call (%llu units)", (unsigned long long)n_units);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, "uc_xcorr_correlate: hipSetDevice");
  if (device_of(in_dev) != l->device) return fail(-EINVAL, "uc_xcorr_correlate: in_dev is not device memory of device %d", l->device);
  if (device_of(corr_dev) != l->device) return fail(-EINVAL, "uc_xcorr_correlate: corr_dev is not device memory of device %d", l->device);
  const size_t bytes = n_pairs * sizeof(Pair);
  StagingSlot& sl = l->slot[l->next];
  int rc = reserve(&sl, bytes, "uc_xcorr_correlate");
  if (rc) return rc;
  PartSlot& ps = l->part[l->next];
  if ((rc = reserve_part(&ps, &sl, (size_t)n_units * lags * sizeof(float))) != 0) return rc;

  // ---- stage (this slot's pinned buffer is free once the copy of two calls back has run)
  if (sl.in_flight) (void)hipEventSynchronize(sl.copied);
  Pair* rec = (Pair*)sl.pinned;
  for (size_t k = 0; k < n_pairs; ++k) {
    rec[k].ref = (uint64_t)pairs[k].ref * istride;
    rec[k].mic = (uint64_t)pairs[k].mic * istride;
  }
  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.tw = l->tw;
  p.part = ps.dev;
  p.corr = corr_dev;
  p.n_in = (int64_t)n_in;
  p.first = (int64_t)first;
  p.n = (int64_t)n;
  p.corr_stride = cstride;
  p.n_units = n_units;
  p.n_pairs = (uint32_t)n_pairs;
  p.n_segments = (uint32_t)n_segments;
  p.n_groups = (uint32_t)n_groups;
  p.max_lag = (int32_t)max_lag;
  // a persistent grid of exactly the workgroups the chip holds at once (the units are dealt statically to them); the
  // runtime's occupancy figure is asked, not assumed
  if (!l->resident[in_dtype]) {
    const int r = resident_blocks_per_cu(in_dtype);
    l->resident[in_dtype] = r > 0 ? r : 4;
  }
  uint64_t grid = (uint64_t)l->cus * (uint64_t)l->resident[in_dtype];
  if (l->grid_override) grid = l->grid_override;
  if (grid > n_units) grid = n_units;

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (sl.in_flight && (e = hipStreamWaitEvent(hs, sl.done, 0)) != hipSuccess) return hip_fail(e, "uc_xcorr_correlate: hipStreamWaitEvent");
  if ((e = hipMemcpyAsync(sl.dev, sl.pinned, bytes, hipMemcpyHostToDevice, hs)) != hipSuccess)
    return hip_fail(e, "uc_xcorr_correlate: hipMemcpyAsync");
  (void)hipEventRecord(sl.copied, hs);
  e = (hipError_t)launch_correlate(in_dtype, (unsigned)grid, hs, p, (const Pair*)sl.dev);
  if (e == hipSuccess) e = (hipError_t)launch_sum(hs, p);
  (void)hipEventRecord(sl.done, hs);
  sl.in_flight = true;
  l->next ^= 1u;
  if (e != hipSuccess) return hip_fail(e, "uc_xcorr_correlate: launch");
  return 0;
}

}  // extern "C"
