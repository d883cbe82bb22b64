// uc_track_api.cpp -- the C-ABI of include/uchirp_track.h on top of uc_track_kernel.hip: errors, the object, its twiddle
// table, staging buffers and unit sums, the finishing rule, argument checks, the launches.  Built like uc_xcorr_api.cpp, with
// the same host-side helpers (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_track.so stands
// alone.  No CPU compute path exists here: without a usable HIP device uc_track_create fails.  Every entry point leaves the
// calling thread's current HIP device as it found it.
#include "../../include/uchirp_track.h"
#include "uc_track.hpp"
#include "uc_host.hpp"

#include <vector>

using namespace uc_track_dev;

static_assert(sizeof(uc_track_pair) == 8 && sizeof(uc_track_peak_t) == 32 && sizeof(Pair) == 16, "layouts of uchirp_track.h");
static_assert(sizeof(uc_track_slot) == sizeof(Slot) && sizeof(uc_track_crest) == sizeof(Crest) && sizeof(Crest) == 136, "the crest record");
static_assert(offsetof(uc_track_crest, slot) == offsetof(Crest, slot) && offsetof(uc_track_slot, r) == offsetof(Slot, r), "the crest record");
static_assert(UC_TRACK_MAX_LAG == MAX_LAG && UC_TRACK_POINTS == POINTS && UC_TRACK_GROUP == GROUP && UC_TRACK_SLOTS == SLOTS, "the kernel's constants");
static_assert(POINTS - 2 * MAX_LAG >= MAX_LAG, "only a row's first samples can lie in front of the row");
static_assert(UC_TRACK_DTYPE_I32 == DT_I32 && UC_TRACK_DTYPE_F32 == DT_F32, "dtype values");
static_assert(UC_TRACK_NO_PEAK == NO_PEAK && UC_TRACK_AT_EDGE == AT_EDGE && UC_TRACK_NOT_FINITE == NOT_FINITE, "flag values");

// the unit sums of one call (device memory only); one per staging slot, so that call k never writes what call k - 1 reads
struct PartSlot {
  float* dev = nullptr;
  size_t cap = 0;   // bytes
};

struct uc_track {
  int device = 0;
  int cus = 0;
  unsigned grid_override = 0;      // UC_TRACK_GRID under UC_TUNING=1
  bool crests_of_corr = false;     // UC_TRACK_CRESTS_OF_CORR=1 under UC_TUNING=1: corr_dev is READ (tests of the crest kernel)
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
    return fail(-ENOMEM, "uc_track_windows: %zu bytes of unit sums: %s", cap, hipGetErrorString(e));
  }
  if (sl->in_flight) (void)hipEventSynchronize(sl->done);  // the old buffer may still be read
  if (ps->dev) (void)hipFree(ps->dev);
  ps->dev = (float*)d;
  ps->cap = cap;
  return 0;
}

bool overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

}  // namespace

extern "C" {

int uc_track_abi_version(void) { return UC_TRACK_ABI_VERSION; }

const char* uc_track_last_error(void) { return g_err.c_str(); }

int uc_track_finish(const uc_track_crest* crest, uint32_t max_lag, uc_track_peak_t* out) {
  if (!crest || !out) return fail(-EINVAL, "uc_track_finish: crest or out is NULL");
  if (max_lag < 1 || max_lag > UC_TRACK_MAX_LAG) return fail(-EINVAL, "uc_track_finish: max_lag %u not in 1 .. %d", max_lag, UC_TRACK_MAX_LAG);
  if (crest->flags & UC_TRACK_NOT_FINITE) return fail(-EINVAL, "uc_track_finish: the correlation held a value that is not finite");
  const int L = (int)max_lag, last = 2 * L;
  for (int i = 0; i < UC_TRACK_SLOTS; ++i)
    if (crest->slot[i].k != -1 && (crest->slot[i].k < 1 || crest->slot[i].k >= last))
      return fail(-EINVAL, "uc_track_finish: slot %d: k %d not in 1 .. %d", i, crest->slot[i].k, last - 1);
  // the loop body of uc_xcorr_peak over the occupied slots (they are candidates, in ascending k)
  double best = 0.0, second = 0.0, best_d = 0.0;
  int best_k = -1;
  for (int i = 0; i < UC_TRACK_SLOTS; ++i) {
    if (crest->slot[i].k < 0) continue;
    const double* r = crest->slot[i].r;   // r[k-1], r[k], r[k+1]
    const double c = (r[0] + r[2]) / (2.0 * r[1]);
    double height = r[1], d = 0.0;
    if (c > -1.0 && c < 1.0) {
      const double w = std::acos(c);
      const double q = (r[2] - r[0]) / (2.0 * std::sin(w));
      height = std::hypot(r[1], q);
      d = std::atan2(q, r[1]) / w;
    }
    if (best_k < 0 || height > best) {
      if (best_k >= 0) second = best;
      best = height;
      best_d = d;
      best_k = crest->slot[i].k;
    } else if (height > second) {
      second = height;
    }
  }
  memset(out, 0, sizeof(*out));
  out->flags = crest->flags & UC_TRACK_AT_EDGE;
  if (best_k < 0) {
    out->flags |= UC_TRACK_NO_PEAK;
    return 0;
  }
  out->delay_samples = (double)(best_k - L) + best_d;
  out->height = best;
  out->runner_up = second / best;
  out->lag = best_k - L;
  return 0;
}

int uc_track_create(int device, uc_track** out) {
  if (!out) return fail(-EINVAL, "uc_track_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(-ENODEV, "uc_track_create: no HIP device (%s); this library has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "0 devices");
  }
  if (device < 0 || device >= ndev) return fail(-ENODEV, "uc_track_create: device %d out of range [0,%d)", device, ndev);
  DeviceGuard guard;
  if ((e = hipSetDevice(device)) != hipSuccess) return hip_fail(e, "uc_track_create: hipSetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(e, "uc_track_create: hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(-ENODEV, "uc_track_create: device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
  uc_track* l = new uc_track();
  l->device = device;
  l->cus = prop.multiProcessorCount;
  // experiment switches are read only under UC_TUNING=1, so that a stray variable in a production environment changes nothing
  const char* tuning = getenv("UC_TUNING");
  if (tuning && !strcmp(tuning, "1")) {
    const char* g = getenv("UC_TRACK_GRID");
    if (g && atoi(g) > 0) l->grid_override = (unsigned)atoi(g);
    // test-only (include/uchirp_track.h, "Test hook"): corr_dev becomes an INPUT and the correlation kernel is not launched
    const char* c = getenv("UC_TRACK_CRESTS_OF_CORR");
    l->crests_of_corr = c && !strcmp(c, "1");
  }
  {
    // the transform's twiddles, cosine and sine in double, rounded once (as libuchirp_xcorr.so builds its own)
    std::vector<float> tw(2 * (size_t)POINTS);
    for (int k = 0; k < POINTS; ++k) {
      const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)POINTS;
      tw[2 * k] = (float)std::cos(a);
      tw[2 * k + 1] = (float)std::sin(a);
    }
    if ((e = hipMalloc((void**)&l->tw, tw.size() * sizeof(float))) != hipSuccess) {
      (void)hipGetLastError();
      delete l;
      return fail(-ENOMEM, "uc_track_create: the twiddle table: %s", hipGetErrorString(e));
    }
    if ((e = hipMemcpy(l->tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) {
      uc_track_destroy(l);
      return hip_fail(e, "uc_track_create: hipMemcpy");
    }
  }
  for (StagingSlot& sl : l->slot)
    if ((e = hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)) != hipSuccess) {
      uc_track_destroy(l);
      return hip_fail(e, "uc_track_create: hipEventCreate");
    }
  *out = l;
  return 0;
}

void uc_track_destroy(uc_track* l) {
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

int uc_track_windows(uc_track* l, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                     const uc_track_pair* pairs, size_t n_pairs, size_t first, size_t window_len, size_t hop,
                     size_t n_windows, uint32_t max_lag, double* corr_dev, size_t corr_stride, uc_track_crest* crest_dev,
                     void* hip_stream) {
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_track_windows: track is NULL");
  if (!in_dev) return fail(-EINVAL, "uc_track_windows: in_dev is NULL");
  if (!corr_dev && !crest_dev) return fail(-EINVAL, "uc_track_windows: corr_dev and crest_dev are both NULL");
  if (!pairs) return fail(-EINVAL, "uc_track_windows: pairs is NULL");
  if (in_dtype != UC_TRACK_DTYPE_I32 && in_dtype != UC_TRACK_DTYPE_F32) return fail(-EINVAL, "uc_track_windows: unknown dtype %d", in_dtype);
  if (n_mics == 0 || n_mics > 0xFFFFFFFFull) return fail(-EINVAL, "uc_track_windows: n_mics %zu out of range", n_mics);
  if (n_pairs == 0 || n_pairs > 0xFFFFFFFFull) return fail(-EINVAL, "uc_track_windows: n_pairs %zu out of range", n_pairs);
  if (n_windows == 0 || n_windows > 0xFFFFFFFFull) return fail(-EINVAL, "uc_track_windows: n_windows %zu out of range", n_windows);
  if (n_in == 0 || window_len == 0) return fail(-EINVAL, "uc_track_windows: n_in or window_len is 0");
  if (hop == 0) return fail(-EINVAL, "uc_track_windows: hop is 0");
  if (n_in > (1ull << 40)) return fail(-EINVAL, "uc_track_windows: n_in too large");
  if (first > n_in || window_len > n_in - first || (n_windows > 1 && (hop > n_in || (n_windows - 1) > (n_in - first - window_len) / hop)))
    return fail(-EINVAL, "uc_track_windows: first %zu + (n_windows %zu - 1) hop %zu + window_len %zu > n_in %zu", first, n_windows, hop,
                window_len, n_in);
  if (max_lag < 1 || max_lag > UC_TRACK_MAX_LAG) return fail(-EINVAL, "uc_track_windows: max_lag %u not in 1 .. %d", max_lag, UC_TRACK_MAX_LAG);
  const size_t lags = 2 * (size_t)max_lag + 1;
  const size_t istride = in_stride ? in_stride : n_in, cstride = corr_stride ? corr_stride : lags;
  if (istride < n_in) return fail(-EINVAL, "uc_track_windows: in_stride %zu < n_in %zu", in_stride, n_in);
  if (cstride < lags) return fail(-EINVAL, "uc_track_windows: corr_stride %zu < 2 max_lag + 1 = %zu", corr_stride, lags);
  if (istride > (1ull << 40) || cstride > (1ull << 40)) return fail(-EINVAL, "uc_track_windows: stride too large");
  const uint64_t n_rows = (uint64_t)n_pairs * n_windows;
  if (n_rows > 0xFFFFFFFFull) return fail(-EINVAL, "uc_track_windows: n_pairs * n_windows too large for one call (%llu)", (unsigned long long)n_rows);
  // counts are below 2^32 and strides at most 2^40, so the products below cannot wrap; a buffer of 2^60 bytes is no buffer
  if ((uint64_t)n_mics * istride > (1ull << 58) || n_rows > (1ull << 57) / cstride)
    return fail(-EINVAL, "uc_track_windows: n_mics * in_stride or n_pairs * n_windows * corr_stride too large");
  for (size_t k = 0; k < n_pairs; ++k)
    if (pairs[k].ref >= n_mics || pairs[k].mic >= n_mics)
      return fail(-EINVAL, "uc_track_windows: pair %zu: rows %u, %u; n_mics %zu", k, pairs[k].ref, pairs[k].mic, n_mics);
  const uintptr_t ia = (uintptr_t)in_dev, ib = ia + ((n_mics - 1) * istride + n_in) * 4;
  const uintptr_t oa = (uintptr_t)corr_dev, ob = oa + ((n_rows - 1) * cstride + lags) * 8;
  const uintptr_t ca = (uintptr_t)crest_dev, cb = ca + n_rows * sizeof(uc_track_crest);
  if (corr_dev && overlap(oa, ob, ia, ib)) return fail(-EINVAL, "uc_track_windows: corr_dev overlaps in_dev");
  if (crest_dev && overlap(ca, cb, ia, ib)) return fail(-EINVAL, "uc_track_windows: crest_dev overlaps in_dev");
  if (crest_dev && corr_dev && overlap(ca, cb, oa, ob)) return fail(-EINVAL, "uc_track_windows: crest_dev overlaps corr_dev");
  if (l->crests_of_corr && (!corr_dev || !crest_dev)) return fail(-EINVAL, "uc_track_windows: UC_TRACK_CRESTS_OF_CORR needs corr_dev and crest_dev");
  const uint64_t seg = (uint64_t)POINTS - 2 * max_lag;                    // S: 1024 .. 2046
  const uint64_t n_segments = ((uint64_t)window_len + seg - 1) / seg, n_groups = (n_segments + GROUP - 1) / GROUP;   // < 2^31, 2^29
  if (n_groups > 0xFFFFFFFFull / n_rows) return fail(-EINVAL, "uc_track_windows: n_pairs * n_windows * segments too large for one call");
  const uint64_t n_units = n_rows * n_groups;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, "uc_track_windows: hipSetDevice");
  if (device_of(in_dev) != l->device) return fail(-EINVAL, "uc_track_windows: in_dev is not device memory of device %d", l->device);
  if (corr_dev && device_of(corr_dev) != l->device) return fail(-EINVAL, "uc_track_windows: corr_dev is not device memory of device %d", l->device);
  if (crest_dev && device_of(crest_dev) != l->device) return fail(-EINVAL, "uc_track_windows: crest_dev is not device memory of device %d", l->device);
  const size_t bytes = n_pairs * sizeof(Pair);
  StagingSlot& sl = l->slot[l->next];
  int rc = reserve(&sl, bytes, "uc_track_windows");
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
  p.crest = (Crest*)crest_dev;
  p.n_in = (int64_t)n_in;
  p.first = (int64_t)first;
  p.window_len = (int64_t)window_len;
  p.hop = (int64_t)hop;
  p.corr_stride = cstride;
  p.n_units = n_units;
  p.n_pairs = (uint32_t)n_pairs;
  p.n_windows = (uint32_t)n_windows;
  p.n_segments = (uint32_t)n_segments;
  p.n_groups = (uint32_t)n_groups;
  p.max_lag = (int32_t)max_lag;
  p.from_corr = l->crests_of_corr ? 1u : 0u;
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
  if (sl.in_flight && (e = hipStreamWaitEvent(hs, sl.done, 0)) != hipSuccess) return hip_fail(e, "uc_track_windows: hipStreamWaitEvent");
  if ((e = hipMemcpyAsync(sl.dev, sl.pinned, bytes, hipMemcpyHostToDevice, hs)) != hipSuccess)
    return hip_fail(e, "uc_track_windows: hipMemcpyAsync");
  (void)hipEventRecord(sl.copied, hs);
  e = hipSuccess;
  if (!p.from_corr) e = (hipError_t)launch_correlate(in_dtype, (unsigned)grid, hs, p, (const Pair*)sl.dev);
  if (e == hipSuccess) e = (hipError_t)launch_crest(hs, p);
  (void)hipEventRecord(sl.done, hs);
  sl.in_flight = true;
  l->next ^= 1u;
  if (e != hipSuccess) return hip_fail(e, "uc_track_windows: launch");
  return 0;
}

}  // extern "C"
