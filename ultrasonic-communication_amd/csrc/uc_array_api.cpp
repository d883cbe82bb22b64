// uc_array_api.cpp -- the C-ABI of include/uchirp_array.h on top of uc_array_kernel.hip: errors, the object and its
// staging tables, the coefficients, argument checks, the launch.  The object's base, create and destroy, the staging
// protocol, the grid and the checks of the row matrices are the shared host layer's (uc_host.hpp: header-only, nothing
// crosses a library boundary): libuchirp_array.so stands alone.  No CPU compute path exists here: without a usable HIP
// device uc_array_create fails.  Every entry point leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_array.h"
#include "uc_array.hpp"
#include "uc_host.hpp"

using namespace uc_array_dev;

static_assert(sizeof(uc_array_tap) == 16 && sizeof(uc_array_beam) == 8 && sizeof(Beam) == sizeof(uc_array_beam), "layouts of uchirp_array.h");
static_assert(sizeof(Tap) == 80 && UC_ARRAY_MAX_TAPS == MAX_TAPS && UC_ARRAY_COEFS == COEFS, "the kernel's tap record");
static_assert(UC_ARRAY_DTYPE_I32 == DT_I32 && UC_ARRAY_DTYPE_F32 == DT_F32, "dtype values");

// staging: [n_taps Tap records][n_beams Beam records]
struct uc_array : HostBase {};

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
  DeviceGuard guard;
  return open("uc_array_create", "UC_ARRAY_GRID", device, out);
}

void uc_array_destroy(uc_array* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  delete l;
}

int uc_array_combine(uc_array* l, const void* in_dev, int in_dtype, size_t n_mics, uint64_t in_first, size_t n_in, size_t in_stride,
                     const uc_array_tap* taps, size_t n_taps, const uc_array_beam* beams, size_t n_beams, float* out_dev,
                     uint64_t out_first, size_t n_out, size_t out_stride, void* hip_stream) {
  static const char WHO[] = "uc_array_combine";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_array_combine: array is NULL");
  if (!in_dev || !out_dev) return fail(-EINVAL, "uc_array_combine: in_dev or out_dev is NULL");
  if (!taps || !beams) return fail(-EINVAL, "uc_array_combine: taps or beams is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_mics", n_mics)) return rc;
  if (int rc = check_count(WHO, "n_taps", n_taps)) return rc;
  if (int rc = check_count(WHO, "n_beams", n_beams)) return rc;
  if (n_in == 0 || n_out == 0) return fail(-EINVAL, "uc_array_combine: n_in or n_out is 0");
  if (in_first > (1ull << 52) || out_first > (1ull << 52) || n_in > (1ull << 40) || n_out > (1ull << 40))
    return fail(-EINVAL, "uc_array_combine: sample range too large");
  const size_t istride = stride_or(in_stride, n_in), ostride = stride_or(out_stride, n_out);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_stride(WHO, "out_stride", out_stride, "n_out", n_out)) return rc;
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_mics, istride, n_beams, ostride, 1ull << 58, "n_beams * out_stride")) return rc;
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
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, span_bytes(n_beams, ostride, n_out, 4), "in_dev", in_dev, span_bytes(n_mics, istride, n_in, 4)))
    return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  const size_t tap_bytes = n_taps * sizeof(Tap), bytes = tap_bytes + n_beams * sizeof(Beam);
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  Tap* trec = (Tap*)sl->pinned;
  for (size_t k = 0; k < n_taps; ++k) {
    coefficients(taps[k].delay_samples, taps[k].weight, &trec[k].shift, trec[k].c);
    trec[k].row = (uint64_t)taps[k].mic * istride;
  }
  memcpy((char*)sl->pinned + tap_bytes, beams, n_beams * sizeof(Beam));
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
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 8, (uint64_t)n_beams * tiles_per_beam);

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  const char* d = (const char*)sl->dev;
  e = (hipError_t)launch_combine(in_dtype, (unsigned)grid, hs, p, (const Beam*)(d + tap_bytes), (const Tap*)d);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
