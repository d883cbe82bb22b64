// uc_align_api.cpp -- the C-ABI of include/uchirp_align.h on top of uc_align_kernel.hip: the object and its unit sums, the
// peak rule (uc_crest.hpp), the checks and the staging that are its own, the launches.  The object's base, create and
// destroy, the staging protocol, the grid and the checks of the row matrices are the shared host layer's (uc_host.hpp:
// header-only, nothing crosses a library boundary): libuchirp_align.so stands alone.  No CPU compute path exists here:
// without a usable HIP device uc_align_create fails.  Every entry point leaves the calling thread's current HIP device as
// it found it.
#include "../../include/uchirp_align.h"
#include "uc_align.hpp"
#include "uc_crest.hpp"
#include "uc_host.hpp"

using namespace uc_align_dev;

static_assert(sizeof(uc_align_pair) == 8 && sizeof(uc_align_peak_t) == 32 && sizeof(Pair) == 16, "layouts of uchirp_align.h");
static_assert(UC_ALIGN_MAX_LAG == MAX_LAG && UC_ALIGN_SEGMENT == SEGMENT, "the kernel's constants");
static_assert(UC_ALIGN_ROUNDINGS == SEGMENT / 64 + 6, "a chain of SEGMENT / 64 multiply-adds and a tree of 6 additions");
static_assert(UC_ALIGN_DTYPE_I32 == DT_I32 && UC_ALIGN_DTYPE_F32 == DT_F32, "dtype values");

// staging: [n_pairs Pair records]
struct uc_align : HostBase {
  DeviceBuffer part[2];            // the unit sums of one call; one per staging slot, so that call k never writes what call k - 1 reads
};

extern "C" {

int uc_align_abi_version(void) { return UC_ALIGN_ABI_VERSION; }

const char* uc_align_last_error(void) { return g_err.c_str(); }

int uc_align_peak(const double* r, uint32_t max_lag, uc_align_peak_t* out) {
  if (!r || !out) return fail(-EINVAL, "uc_align_peak: corr or out is NULL");
  if (int rc = check_max_lag("uc_align_peak", max_lag, UC_ALIGN_MAX_LAG)) return rc;
  const int L = (int)max_lag, last = 2 * L;
  int largest = 0;
  for (int k = 0; k <= last; ++k) {
    if (!std::isfinite(r[k])) return fail(-EINVAL, "uc_align_peak: corr[%d] is not finite", k);
    if (r[k] > r[largest]) largest = k;
  }
  CrestChoice choice;
  for (int k = 1; k < last; ++k)
    if (r[k] > 0.0 && r[k] >= r[k - 1] && r[k] > r[k + 1]) choice.add(k, crest_fit(r[k - 1], r[k], r[k + 1]));
  memset(out, 0, sizeof(*out));
  if (largest == 0 || largest == last) out->flags |= UC_ALIGN_AT_EDGE;
  if (choice.best_k < 0) {
    out->flags |= UC_ALIGN_NO_PEAK;
    return 0;
  }
  choice.store(L, out);
  return 0;
}

int uc_align_create(int device, uc_align** out) {
  DeviceGuard guard;
  return open("uc_align_create", "UC_ALIGN_GRID", device, out);
}

void uc_align_destroy(uc_align* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  for (DeviceBuffer& b : l->part)
    if (b.dev) (void)hipFree(b.dev);
  delete l;
}

int uc_align_correlate(uc_align* l, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                       const uc_align_pair* pairs, size_t n_pairs, size_t first, size_t n, uint32_t max_lag, double* corr_dev,
                       size_t corr_stride, void* hip_stream) {
  static const char WHO[] = "uc_align_correlate";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_align_correlate: align is NULL");
  if (!in_dev || !corr_dev) return fail(-EINVAL, "uc_align_correlate: in_dev or corr_dev is NULL");
  if (!pairs) return fail(-EINVAL, "uc_align_correlate: pairs is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_mics", n_mics)) return rc;
  if (int rc = check_count(WHO, "n_pairs", n_pairs)) return rc;
  if (n_in == 0 || n == 0) return fail(-EINVAL, "uc_align_correlate: n_in or n is 0");
  if (n_in > STRIDE_MAX) return fail(-EINVAL, "uc_align_correlate: n_in too large");
  if (first > n_in || n > n_in - first) return fail(-EINVAL, "uc_align_correlate: first %zu + n %zu > n_in %zu", first, n, n_in);
  if (int rc = check_max_lag(WHO, max_lag, UC_ALIGN_MAX_LAG)) return rc;
  const size_t lags = 2 * (size_t)max_lag + 1;
  const size_t istride = stride_or(in_stride, n_in), cstride = stride_or(corr_stride, lags);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_corr_stride(WHO, corr_stride, lags)) return rc;
  if (int rc = check_strides_max(WHO, istride, cstride)) return rc;
  if (int rc = check_extent(WHO, n_mics, istride, n_pairs, cstride, 1ull << 57, "n_pairs * corr_stride")) return rc;
  if (int rc = check_pairs(WHO, pairs, n_pairs, n_mics)) return rc;
  if (int rc = check_disjoint(WHO, "corr_dev", corr_dev, span_bytes(n_pairs, cstride, lags, 8), "in_dev", in_dev, span_bytes(n_mics, istride, n_in, 4)))
    return rc;
  const uint64_t n_segments = ((uint64_t)n + SEGMENT - 1) / SEGMENT, n_blocks = (lags + LAGS - 1) / LAGS;
  const uint64_t n_units = (uint64_t)n_pairs * n_segments * n_blocks;     // < 2^32 * 2^28 * 5
  if (n_units > (1ull << 36)) return fail(-EINVAL, "uc_align_correlate: n_pairs * segments too large for one call (%llu units)", (unsigned long long)n_units);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "corr_dev", corr_dev, l->device)) return rc;
  const size_t bytes = n_pairs * sizeof(Pair);
  DeviceBuffer& part = l->part[l->next];
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl, &part, (size_t)n_units * LAGS * sizeof(float), "unit sums")) return rc;

  // ---- stage
  stage_pairs((Pair*)sl->pinned, pairs, n_pairs, istride);
  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.part = (float*)part.dev;
  p.corr = corr_dev;
  p.n_in = (int64_t)n_in;
  p.first = (int64_t)first;
  p.n = (int64_t)n;
  p.corr_stride = cstride;
  p.n_units = n_units;
  p.n_pairs = (uint32_t)n_pairs;
  p.n_segments = (uint32_t)n_segments;
  p.n_blocks = (uint32_t)n_blocks;
  p.max_lag = (int32_t)max_lag;
  // the units are dealt to the grid's waves
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 3, (n_units + THREADS / 64 - 1) / (THREADS / 64));

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_correlate(in_dtype, (unsigned)grid, hs, p, (const Pair*)sl->dev);
  if (e == hipSuccess) e = (hipError_t)launch_sum(hs, p);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
