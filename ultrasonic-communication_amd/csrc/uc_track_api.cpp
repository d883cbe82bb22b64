// uc_track_api.cpp -- the C-ABI of include/uchirp_track.h on top of uc_track_kernel.hip: the object, its twiddle table and
// unit sums, the finishing rule (uc_crest.hpp: that of uc_xcorr_peak), the checks and the staging that are its own, the
// launches.  The object's base, create and destroy, the staging protocol, the grid and the checks of the row matrices are
// the shared host layer's (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_track.so stands alone.
// No CPU compute path exists here: without a usable HIP device uc_track_create fails.  Every entry point leaves the
// calling thread's current HIP device as it found it.
#include "../../include/uchirp_track.h"
#include "uc_track.hpp"
#include "uc_crest.hpp"
#include "uc_host.hpp"

using namespace uc_track_dev;

static_assert(sizeof(uc_track_pair) == 8 && sizeof(uc_track_peak_t) == 32 && sizeof(Pair) == 16, "layouts of uchirp_track.h");
static_assert(sizeof(uc_track_slot) == sizeof(Slot) && sizeof(uc_track_crest) == sizeof(Crest) && sizeof(Crest) == 136, "the crest record");
static_assert(offsetof(uc_track_crest, slot) == offsetof(Crest, slot) && offsetof(uc_track_slot, r) == offsetof(Slot, r), "the crest record");
static_assert(UC_TRACK_MAX_LAG == MAX_LAG && UC_TRACK_POINTS == POINTS && UC_TRACK_GROUP == GROUP && UC_TRACK_SLOTS == SLOTS, "the kernel's constants");
static_assert(POINTS - 2 * MAX_LAG >= MAX_LAG, "only a row's first samples can lie in front of the row");
static_assert(UC_TRACK_DTYPE_I32 == DT_I32 && UC_TRACK_DTYPE_F32 == DT_F32, "dtype values");
static_assert(UC_TRACK_NO_PEAK == NO_PEAK && UC_TRACK_AT_EDGE == AT_EDGE && UC_TRACK_NOT_FINITE == NOT_FINITE, "flag values");

// staging: [n_pairs Pair records]
struct uc_track : HostBase {
  bool crests_of_corr = false;     // UC_TRACK_CRESTS_OF_CORR=1 under UC_TUNING=1: corr_dev is READ (tests of the crest kernel)
  float* tw = nullptr;             // device: exp(-2 pi i k / 2048), k < 2048
  DeviceBuffer part[2];            // the unit sums of one call; one per staging slot, so that call k never writes what call k - 1 reads
};

extern "C" {

int uc_track_abi_version(void) { return UC_TRACK_ABI_VERSION; }

const char* uc_track_last_error(void) { return g_err.c_str(); }

int uc_track_finish(const uc_track_crest* crest, uint32_t max_lag, uc_track_peak_t* out) {
  if (!crest || !out) return fail(-EINVAL, "uc_track_finish: crest or out is NULL");
  if (int rc = check_max_lag("uc_track_finish", max_lag, UC_TRACK_MAX_LAG)) return rc;
  if (crest->flags & UC_TRACK_NOT_FINITE) return fail(-EINVAL, "uc_track_finish: the correlation held a value that is not finite");
  const int L = (int)max_lag, last = 2 * L;
  for (int i = 0; i < UC_TRACK_SLOTS; ++i)
    if (crest->slot[i].k != -1 && (crest->slot[i].k < 1 || crest->slot[i].k >= last))
      return fail(-EINVAL, "uc_track_finish: slot %d: k %d not in 1 .. %d", i, crest->slot[i].k, last - 1);
  // the occupied slots are the candidates, in ascending k: the rule of uc_xcorr_peak (uc_crest.hpp) over them
  CrestChoice choice;
  for (int i = 0; i < UC_TRACK_SLOTS; ++i) {
    const uc_track_slot& c = crest->slot[i];   // r[k-1], r[k], r[k+1]
    if (c.k >= 0) choice.add(c.k, crest_fit(c.r[0], c.r[1], c.r[2]));
  }
  memset(out, 0, sizeof(*out));
  out->flags = crest->flags & UC_TRACK_AT_EDGE;
  if (choice.best_k < 0) {
    out->flags |= UC_TRACK_NO_PEAK;
    return 0;
  }
  choice.store(L, out);
  return 0;
}

int uc_track_create(int device, uc_track** out) {
  DeviceGuard guard;
  int rc = open("uc_track_create", "UC_TRACK_GRID", device, out);
  if (rc) return rc;
  uc_track* l = *out;
  // test-only (include/uchirp_track.h, "Test hook"), read like every experiment switch only under UC_TUNING=1: corr_dev
  // becomes an INPUT and the correlation kernel is not launched
  const char *tuning = getenv("UC_TUNING"), *c = getenv("UC_TRACK_CRESTS_OF_CORR");
  l->crests_of_corr = tuning && !strcmp(tuning, "1") && c && !strcmp(c, "1");
  if ((rc = device_twiddles(&l->tw, POINTS, "uc_track_create")) != 0) {
    uc_track_destroy(l);
    *out = nullptr;
  }
  return rc;
}

void uc_track_destroy(uc_track* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  for (DeviceBuffer& b : l->part)
    if (b.dev) (void)hipFree(b.dev);
  if (l->tw) (void)hipFree(l->tw);
  delete l;
}

int uc_track_windows(uc_track* l, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                     const uc_track_pair* pairs, size_t n_pairs, size_t first, size_t window_len, size_t hop,
                     size_t n_windows, uint32_t max_lag, double* corr_dev, size_t corr_stride, uc_track_crest* crest_dev,
                     void* hip_stream) {
  static const char WHO[] = "uc_track_windows";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_track_windows: track is NULL");
  if (!in_dev) return fail(-EINVAL, "uc_track_windows: in_dev is NULL");
  if (!corr_dev && !crest_dev) return fail(-EINVAL, "uc_track_windows: corr_dev and crest_dev are both NULL");
  if (!pairs) return fail(-EINVAL, "uc_track_windows: pairs is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_mics", n_mics)) return rc;
  if (int rc = check_count(WHO, "n_pairs", n_pairs)) return rc;
  if (int rc = check_count(WHO, "n_windows", n_windows)) return rc;
  if (n_in == 0 || window_len == 0) return fail(-EINVAL, "uc_track_windows: n_in or window_len is 0");
  if (hop == 0) return fail(-EINVAL, "uc_track_windows: hop is 0");
  if (n_in > STRIDE_MAX) return fail(-EINVAL, "uc_track_windows: n_in too large");
  if (first > n_in || window_len > n_in - first || (n_windows > 1 && (hop > n_in || (n_windows - 1) > (n_in - first - window_len) / hop)))
    return fail(-EINVAL, "uc_track_windows: first %zu + (n_windows %zu - 1) hop %zu + window_len %zu > n_in %zu", first, n_windows, hop,
                window_len, n_in);
  if (int rc = check_max_lag(WHO, max_lag, UC_TRACK_MAX_LAG)) return rc;
  const size_t lags = 2 * (size_t)max_lag + 1;
  const size_t istride = stride_or(in_stride, n_in), cstride = stride_or(corr_stride, lags);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_corr_stride(WHO, corr_stride, lags)) return rc;
  if (int rc = check_strides_max(WHO, istride, cstride)) return rc;
  const uint64_t n_rows = (uint64_t)n_pairs * n_windows;
  if (n_rows > COUNT_MAX) return fail(-EINVAL, "uc_track_windows: n_pairs * n_windows too large for one call (%llu)", (unsigned long long)n_rows);
  if (int rc = check_extent(WHO, n_mics, istride, n_rows, cstride, 1ull << 57, "n_pairs * n_windows * corr_stride")) return rc;
  if (int rc = check_pairs(WHO, pairs, n_pairs, n_mics)) return rc;
  const size_t in_bytes = span_bytes(n_mics, istride, n_in, 4), corr_bytes = span_bytes(n_rows, cstride, lags, 8);
  const size_t crest_bytes = n_rows * sizeof(uc_track_crest);
  if (corr_dev)
    if (int rc = check_disjoint(WHO, "corr_dev", corr_dev, corr_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (crest_dev)
    if (int rc = check_disjoint(WHO, "crest_dev", crest_dev, crest_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (crest_dev && corr_dev)
    if (int rc = check_disjoint(WHO, "crest_dev", crest_dev, crest_bytes, "corr_dev", corr_dev, corr_bytes)) return rc;
  if (l->crests_of_corr && (!corr_dev || !crest_dev)) return fail(-EINVAL, "uc_track_windows: UC_TRACK_CRESTS_OF_CORR needs corr_dev and crest_dev");
  const uint64_t seg = (uint64_t)POINTS - 2 * max_lag;                    // S: 1024 .. 2046
  const uint64_t n_segments = ((uint64_t)window_len + seg - 1) / seg, n_groups = (n_segments + GROUP - 1) / GROUP;   // < 2^31, 2^29
  if (n_groups > COUNT_MAX / n_rows) return fail(-EINVAL, "uc_track_windows: n_pairs * n_windows * segments too large for one call");
  const uint64_t n_units = n_rows * n_groups;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (corr_dev)
    if (int rc = check_on_device(WHO, "corr_dev", corr_dev, l->device)) return rc;
  if (crest_dev)
    if (int rc = check_on_device(WHO, "crest_dev", crest_dev, l->device)) return rc;
  const size_t bytes = n_pairs * sizeof(Pair);
  DeviceBuffer& part = l->part[l->next];
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl, &part, (size_t)n_units * lags * sizeof(float), "unit sums")) return rc;

  // ---- stage
  stage_pairs((Pair*)sl->pinned, pairs, n_pairs, istride);
  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.tw = l->tw;
  p.part = (float*)part.dev;
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
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 4, n_units);

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = hipSuccess;
  if (!p.from_corr) e = (hipError_t)launch_correlate(in_dtype, (unsigned)grid, hs, p, (const Pair*)sl->dev);
  if (e == hipSuccess) e = (hipError_t)launch_crest(hs, p);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
