// uc_wcorr_api.cpp -- the C-ABI of include/uchirp_wcorr.h on top of uc_wcorr_kernel.hip: the object, its twiddle table and
// unit sums, the band weights, the peak rule (uc_crest.hpp: that of uc_xcorr_peak), the checks and the staging that are its
// own, the launches.  The object's base, create and destroy, the staging protocol, the grid and the checks of the row
// matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library boundary): libuchirp_wcorr.so
// stands alone.  No CPU compute path exists here: without a usable HIP device uc_wcorr_create fails.  Every entry point
// leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_wcorr.h"
#include "uc_wcorr.hpp"
#include "uc_crest.hpp"
#include "uc_host.hpp"

using namespace uc_wcorr_dev;

static_assert(sizeof(uc_wcorr_pair) == 8 && sizeof(uc_wcorr_peak_t) == 32 && sizeof(Pair) == 16, "layouts of uchirp_wcorr.h");
static_assert(UC_WCORR_MAX_LAG == MAX_LAG && UC_WCORR_POINTS == POINTS && UC_WCORR_GROUP == GROUP && UC_WCORR_BINS == BINS, "the kernel's constants");
static_assert(POINTS - 2 * MAX_LAG >= MAX_LAG, "only a row's first samples can lie in front of the row");
static_assert(UC_WCORR_DTYPE_I32 == DT_I32 && UC_WCORR_DTYPE_F32 == DT_F32, "dtype values");

// staging: [n_pairs Pair records][BINS floats: the weights]
struct uc_wcorr : HostBase {
  float* tw = nullptr;             // device: exp(-2 pi i k / 2048), k < 2048
  DeviceBuffer part[2];            // the unit sums of one call; one per staging slot, so that call k never writes what call k - 1 reads
};

extern "C" {

int uc_wcorr_abi_version(void) { return UC_WCORR_ABI_VERSION; }

const char* uc_wcorr_last_error(void) { return g_err.c_str(); }

int uc_wcorr_peak(const double* r, uint32_t max_lag, uc_wcorr_peak_t* out) {
  if (!r || !out) return fail(-EINVAL, "uc_wcorr_peak: corr or out is NULL");
  if (int rc = check_max_lag("uc_wcorr_peak", max_lag, UC_WCORR_MAX_LAG)) return rc;
  const int L = (int)max_lag, last = 2 * L;
  int largest = 0;
  for (int k = 0; k <= last; ++k) {
    if (!std::isfinite(r[k])) return fail(-EINVAL, "uc_wcorr_peak: corr[%d] is not finite", k);
    if (r[k] > r[largest]) largest = k;
  }
  CrestChoice choice;
  for (int k = 1; k < last; ++k)
    if (r[k] > 0.0 && r[k] >= r[k - 1] && r[k] > r[k + 1]) choice.add(k, crest_fit(r[k - 1], r[k], r[k + 1]));
  memset(out, 0, sizeof(*out));
  if (largest == 0 || largest == last) out->flags |= UC_WCORR_AT_EDGE;
  if (choice.best_k < 0) {
    out->flags |= UC_WCORR_NO_PEAK;
    return 0;
  }
  choice.store(L, out);
  return 0;
}

int uc_wcorr_band_weights(double fs, double f_lo, double f_hi, double taper_hz, uint32_t guard, float* w_out, double* tail_out) {
  if (!w_out) return fail(-EINVAL, "uc_wcorr_band_weights: w_out is NULL");
  if (!std::isfinite(fs) || !std::isfinite(f_lo) || !std::isfinite(f_hi) || !std::isfinite(taper_hz))
    return fail(-EINVAL, "uc_wcorr_band_weights: fs, f_lo, f_hi or taper_hz is not finite");
  if (!(fs > 0.0)) return fail(-EINVAL, "uc_wcorr_band_weights: fs %g is not positive", fs);
  if (f_lo < 0.0 || f_lo > f_hi) return fail(-EINVAL, "uc_wcorr_band_weights: band %g .. %g Hz", f_lo, f_hi);
  if (taper_hz < 0.0) return fail(-EINVAL, "uc_wcorr_band_weights: taper_hz %g is negative", taper_hz);
  const double half_pi = 0.5 * 3.14159265358979323846;
  for (int k = 0; k < BINS; ++k) {
    const double f = (double)k * fs / (double)POINTS;
    const double d = f < f_lo ? f_lo - f : f > f_hi ? f - f_hi : 0.0;   // distance to the band
    double w = 0.0;
    if (d == 0.0) {
      w = 1.0;
    } else if (d < taper_hz) {
      const double c = std::cos(half_pi * d / taper_hz);
      w = c * c;
    }
    w_out[k] = (float)w;
  }
  if (!tail_out) return 0;
  // h[t] = (1 / 2048) sum over k of W[k] cos(2 pi k t / 2048), from the rounded weights; h is even: t = 0 .. 1024 suffice
  std::vector<double> cs(POINTS);
  for (int i = 0; i < POINTS; ++i) cs[i] = std::cos(2.0 * 3.14159265358979323846 * (double)i / (double)POINTS);
  double all = 0.0, tail = 0.0;
  for (int t = 0; t <= POINTS / 2; ++t) {
    double h = (double)w_out[0] + (double)w_out[POINTS / 2] * cs[(t * (POINTS / 2)) & (POINTS - 1)];
    for (int k = 1; k < POINTS / 2; ++k) h += 2.0 * (double)w_out[k] * cs[(k * t) & (POINTS - 1)];
    h /= (double)POINTS;
    const double e = (t == 0 || t == POINTS / 2 ? 1.0 : 2.0) * h * h;   // t and 2048 - t
    all += e;
    if ((uint32_t)t > guard) tail += e;
  }
  *tail_out = all > 0.0 ? tail / all : 0.0;
  return 0;
}

int uc_wcorr_create(int device, uc_wcorr** out) {
  DeviceGuard guard;
  int rc = open("uc_wcorr_create", "UC_WCORR_GRID", device, out);
  if (rc) return rc;
  if ((rc = device_twiddles(&(*out)->tw, POINTS, "uc_wcorr_create")) != 0) {
    uc_wcorr_destroy(*out);
    *out = nullptr;
  }
  return rc;
}

void uc_wcorr_destroy(uc_wcorr* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  for (DeviceBuffer& b : l->part)
    if (b.dev) (void)hipFree(b.dev);
  if (l->tw) (void)hipFree(l->tw);
  delete l;
}

int uc_wcorr_windows(uc_wcorr* l, const void* in_dev, int in_dtype, size_t n_mics, size_t n_in, size_t in_stride,
                     const uc_wcorr_pair* pairs, size_t n_pairs, size_t first, size_t window_len, size_t hop,
                     size_t n_windows, uint32_t max_lag, uint32_t guard, const float* weights, double* corr_dev,
                     size_t corr_stride, void* hip_stream) {
  static const char WHO[] = "uc_wcorr_windows";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_wcorr_windows: wcorr is NULL");
  if (!in_dev || !corr_dev) return fail(-EINVAL, "uc_wcorr_windows: in_dev or corr_dev is NULL");
  if (!pairs) return fail(-EINVAL, "uc_wcorr_windows: pairs is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_mics", n_mics)) return rc;
  if (int rc = check_count(WHO, "n_pairs", n_pairs)) return rc;
  if (int rc = check_count(WHO, "n_windows", n_windows)) return rc;
  if (n_in == 0 || window_len == 0) return fail(-EINVAL, "uc_wcorr_windows: n_in or window_len is 0");
  if (hop == 0) return fail(-EINVAL, "uc_wcorr_windows: hop is 0");
  if (n_in > STRIDE_MAX) return fail(-EINVAL, "uc_wcorr_windows: n_in too large");
  if (first > n_in || window_len > n_in - first || (n_windows > 1 && (hop > n_in || (n_windows - 1) > (n_in - first - window_len) / hop)))
    return fail(-EINVAL, "uc_wcorr_windows: first %zu + (n_windows %zu - 1) hop %zu + window_len %zu > n_in %zu", first, n_windows, hop,
                window_len, n_in);
  if (int rc = check_max_lag(WHO, max_lag, UC_WCORR_MAX_LAG)) return rc;
  if (guard > (uint32_t)UC_WCORR_MAX_LAG - max_lag)
    return fail(-EINVAL, "uc_wcorr_windows: max_lag %u + guard %u > %d", max_lag, guard, UC_WCORR_MAX_LAG);
  if (weights)
    for (int k = 0; k < BINS; ++k)
      if (!std::isfinite(weights[k])) return fail(-EINVAL, "uc_wcorr_windows: weights[%d] is not finite", k);
  const size_t lags = 2 * (size_t)max_lag + 1;
  const size_t istride = stride_or(in_stride, n_in), cstride = stride_or(corr_stride, lags);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_corr_stride(WHO, corr_stride, lags)) return rc;
  if (int rc = check_strides_max(WHO, istride, cstride)) return rc;
  const uint64_t n_rows = (uint64_t)n_pairs * n_windows;
  if (n_rows > COUNT_MAX) return fail(-EINVAL, "uc_wcorr_windows: n_pairs * n_windows too large for one call (%llu)", (unsigned long long)n_rows);
  if (int rc = check_extent(WHO, n_mics, istride, n_rows, cstride, 1ull << 57, "n_pairs * n_windows * corr_stride")) return rc;
  if (int rc = check_pairs(WHO, pairs, n_pairs, n_mics)) return rc;
  if (int rc = check_disjoint(WHO, "corr_dev", corr_dev, span_bytes(n_rows, cstride, lags, 8), "in_dev", in_dev, span_bytes(n_mics, istride, n_in, 4)))
    return rc;
  const uint64_t seg = (uint64_t)POINTS - 2 * ((uint64_t)max_lag + guard);     // S at L': 1024 .. 2046
  const uint64_t n_segments = ((uint64_t)window_len + seg - 1) / seg, n_groups = (n_segments + GROUP - 1) / GROUP;   // < 2^31, 2^29
  if (n_groups > COUNT_MAX / n_rows) return fail(-EINVAL, "uc_wcorr_windows: n_pairs * n_windows * segments too large for one call");
  const uint64_t n_units = n_rows * n_groups;
  DeviceGuard dguard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "corr_dev", corr_dev, l->device)) return rc;
  const size_t pair_bytes = n_pairs * sizeof(Pair), bytes = pair_bytes + BINS * sizeof(float);
  DeviceBuffer& part = l->part[l->next];
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl, &part, (size_t)n_units * lags * sizeof(float), "unit sums")) return rc;

  // ---- stage
  stage_pairs((Pair*)sl->pinned, pairs, n_pairs, istride);
  float* w = (float*)((char*)sl->pinned + pair_bytes);
  for (int k = 0; k < BINS; ++k) w[k] = weights ? weights[k] : 1.0f;
  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.tw = l->tw;
  p.weights = (const float*)((const char*)sl->dev + pair_bytes);
  p.part = (float*)part.dev;
  p.corr = corr_dev;
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
  p.guard = (int32_t)guard;
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 4, n_units);

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_correlate(in_dtype, (unsigned)grid, hs, p, (const Pair*)sl->dev);
  if (e == hipSuccess) e = (hipError_t)launch_sum(hs, p);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
