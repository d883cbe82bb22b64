// uc_xcorr_api.cpp -- the C-ABI of include/uchirp_xcorr.h on top of uc_xcorr_kernel.hip: the object, its twiddle table and
// unit sums, the peak rule (uc_crest.hpp: that of uc_align_peak), the checks and the staging that are its own, the
// launches.  The object's base, create and destroy, the staging protocol, the grid and the checks of the row matrices are
// the shared host layer's (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_xcorr.so stands alone.
// No CPU compute path exists here: without a usable HIP device uc_xcorr_create fails.  Every entry point leaves the
// calling thread's current HIP device as it found it.
#include "../../include/uchirp_xcorr.h"
#include "uc_xcorr.hpp"
#include "uc_crest.hpp"
#include "uc_host.hpp"

using namespace uc_xcorr_dev;

static_assert(sizeof(uc_xcorr_pair) == 8 && sizeof(uc_xcorr_peak_t) == 32 && sizeof(Pair) == 16, "layouts of uchirp_xcorr.h");
static_assert(UC_XCORR_MAX_LAG == MAX_LAG && UC_XCORR_POINTS == POINTS && UC_XCORR_GROUP == GROUP, "the kernel's constants");
static_assert(POINTS - 2 * MAX_LAG >= MAX_LAG, "only a row's first segment can start in front of the row");
static_assert(UC_XCORR_DTYPE_I32 == DT_I32 && UC_XCORR_DTYPE_F32 == DT_F32, "dtype values");

// staging: [n_pairs Pair records]
struct uc_xcorr : HostBase {
  float* tw = nullptr;             // device: exp(-2 pi i k / 2048), k < 2048
  DeviceBuffer part[2];            // the unit sums of one call; one per staging slot, so that call k never writes what call k - 1 reads
};

extern "C" {

int uc_xcorr_abi_version(void) { return UC_XCORR_ABI_VERSION; }

const char* uc_xcorr_last_error(void) { return g_err.c_str(); }

int uc_xcorr_peak(const double* r, uint32_t max_lag, uc_xcorr_peak_t* out) {
  if (!r || !out) return fail(-EINVAL, "uc_xcorr_peak: corr or out is NULL");
  if (int rc = check_max_lag("uc_xcorr_peak", max_lag, UC_XCORR_MAX_LAG)) return rc;
  const int L = (int)max_lag, last = 2 * L;
  int largest = 0;
  for (int k = 0; k <= last; ++k) {
    if (!std::isfinite(r[k])) return fail(-EINVAL, "uc_xcorr_peak: corr[%d] is not finite", k);
    if (r[k] > r[largest]) largest = k;
  }
  CrestChoice choice;
  for (int k = 1; k < last; ++k)
    if (r[k] > 0.0 && r[k] >= r[k - 1] && r[k] > r[k + 1]) choice.add(k, crest_fit(r[k - 1], r[k], r[k + 1]));
  memset(out, 0, sizeof(*out));
  if (largest == 0 || largest == last) out->flags |= UC_XCORR_AT_EDGE;
  if (choice.best_k < 0) {
    out->flags |= UC_XCORR_NO_PEAK;
    return 0;
  }
  choice.store(L, out);
  return 0;
}

int uc_xcorr_create(int device, uc_xcorr** out) {
  DeviceGuard guard;
  int rc = open("uc_xcorr_create", "UC_XCORR_GRID", device, out);
  if (rc) return rc;
  if ((rc = device_twiddles(&(*out)->tw, POINTS, "uc_xcorr_create")) != 0) {
    uc_xcorr_destroy(*out);
    *out = nullptr;
  }
  return rc;
}

void uc_xcorr_destroy(uc_xcorr* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  for (DeviceBuffer& b : l->part)
    if (b.dev) (void)hipFree(b.dev);
  if (l->tw) (void)hipFree(l->tw);
  delete l;
}

int uc_xcorr_correlate(uc_xcorr* l, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                       const uc_xcorr_pair* pairs, size_t n_pairs, size_t first, size_t n, uint32_t max_lag, double* corr_dev,
                       size_t corr_stride, void* hip_stream) {
  static const char WHO[] = "uc_xcorr_correlate";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_xcorr_correlate: xcorr is NULL");
  if (!in_dev || !corr_dev) return fail(-EINVAL, "uc_xcorr_correlate: in_dev or corr_dev is NULL");
  if (!pairs) return fail(-EINVAL, "uc_xcorr_correlate: pairs is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_mics", n_mics)) return rc;
  if (int rc = check_count(WHO, "n_pairs", n_pairs)) return rc;
  if (n_in == 0 || n == 0) return fail(-EINVAL, "uc_xcorr_correlate: n_in or n is 0");
  if (n_in > STRIDE_MAX) return fail(-EINVAL, "uc_xcorr_correlate: n_in too large");
  if (first > n_in || n > n_in - first) return fail(-EINVAL, "uc_xcorr_correlate: first %zu + n %zu > n_in %zu", first, n, n_in);
  if (int rc = check_max_lag(WHO, max_lag, UC_XCORR_MAX_LAG)) return rc;
  const size_t lags = 2 * (size_t)max_lag + 1;
  const size_t istride = stride_or(in_stride, n_in), cstride = stride_or(corr_stride, lags);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_corr_stride(WHO, corr_stride, lags)) return rc;
  if (int rc = check_strides_max(WHO, istride, cstride)) return rc;
  if (int rc = check_extent(WHO, n_mics, istride, n_pairs, cstride, 1ull << 57, "n_pairs * corr_stride")) return rc;
  if (int rc = check_pairs(WHO, pairs, n_pairs, n_mics)) return rc;
  if (int rc = check_disjoint(WHO, "corr_dev", corr_dev, span_bytes(n_pairs, cstride, lags, 8), "in_dev", in_dev, span_bytes(n_mics, istride, n_in, 4)))
    return rc;
  const uint64_t seg = (uint64_t)POINTS - 2 * max_lag;                    // S: 1024 .. 2046
  const uint64_t n_segments = ((uint64_t)n + seg - 1) / seg, n_groups = (n_segments + GROUP - 1) / GROUP;   // < 2^31, 2^29
  const uint64_t n_units = (uint64_t)n_pairs * n_groups;
  if (n_units > (1ull << 36)) return fail(-EINVAL, "uc_xcorr_correlate: n_pairs * segments too large for one call (%llu units)", (unsigned long long)n_units);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "corr_dev", corr_dev, l->device)) return rc;
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
  p.n_in = (int64_t)n_in;
  p.first = (int64_t)first;
  p.n = (int64_t)n;
  p.corr_stride = cstride;
  p.n_units = n_units;
  p.n_pairs = (uint32_t)n_pairs;
  p.n_segments = (uint32_t)n_segments;
  p.n_groups = (uint32_t)n_groups;
  p.max_lag = (int32_t)max_lag;
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 4, n_units);

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_correlate(in_dtype, (unsigned)grid, hs, p, (const Pair*)sl->dev);
  if (e == hipSuccess) e = (hipError_t)launch_sum(hs, p);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
