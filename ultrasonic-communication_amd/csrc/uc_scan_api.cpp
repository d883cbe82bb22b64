// uc_scan_api.cpp -- the C-ABI of include/uchirp_scan.h on top of uc_scan_kernel.hip: the host functions of the definition
// (the quantiser, a tap's table, one beam and one window in plain C on the arithmetic of uc_scan.hpp that the kernel compiles
// too), the steering set, the checks that are its own, the launches.  The object's base, create and destroy, the grid and the
// checks of the row matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library boundary):
// libuchirp_scan.so stands alone.  No CPU compute path exists behind uc_scan_power: without a usable HIP device
// uc_scan_create fails.  Every entry point leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_scan.h"
#include "uc_host.hpp"
#include "uc_scan.hpp"

#include <algorithm>

using namespace uc_scan_dev;

static_assert(UC_SCAN_DTYPE_I32 == DT_I32 && UC_SCAN_DTYPE_F32 == DT_F32, "dtype values");
static_assert(UC_SCAN_MAX_TAPS == MAX_TAPS && UC_SCAN_COEFS == COEFS && UC_SCAN_FRACTIONS == FRACTIONS && UC_SCAN_SEGMENT == SEGMENT, "constants of uchirp_scan.h");
static_assert(sizeof(uc_scan_best) == 16 && sizeof(Best) == 16, "the best record");

struct uc_scan : HostBase {
  // the steering set: one allocation, [n_taps x 256 x 16 floats][n_beams x n_taps int32][n_beams bytes]
  void* set_dev = nullptr;
  uint32_t n_taps = 0;
  uint32_t n_beams = 0;            // 0: no set
  uint32_t n_direct = 0;           // beams that take the kernel's direct path
  uint32_t max_mic = 0;
  uint32_t mic[MAX_TAPS] = {};
  int32_t lo[MAX_TAPS] = {};
  DeviceBuffer scratch;            // the powers of a call without power_dev
};

namespace {

constexpr double DELAY_MAX = 1048576.0;      // 2^20
constexpr int64_t Q_MAX = 1ll << 28;         // 2^20 * 256
constexpr uint64_t SAMPLE_MAX = 1ull << 52, SPAN_MAX = 1ull << 53;

// I0(x), the modified Bessel function of order 0, by its power series, as uc_array_api.cpp sums it
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

// row `frac` of a tap's table: the coefficients of uc_array_tap_coefficients(whole + frac / 256.0, weight) for any whole
// number (frac / 256.0 is exact, and so is the subtraction that array combiner's code gets it back by), operation for
// operation as uc_array_api.cpp evaluates them
void coefficient_row(int frac, float weight, float c[COEFS]) {
  const double f = (double)frac / 256.0;
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

// one beam, one window: the definition
template <int DT>
double power_row(const uint32_t* in, int64_t in_first, int64_t n_in, size_t istride, const uint32_t* mics, const int32_t* q, size_t n_taps,
                 const float* coef, int64_t first, int64_t window_len) {
  double total = 0.0;
  for (int64_t seg = 0; seg < window_len; seg += SEGMENT) {
    float chain[64];
    for (float& v : chain) v = 0.0f;
    const int64_t end = std::min<int64_t>(seg + SEGMENT, window_len);
    for (int64_t i = seg; i < end; ++i) {
      float y = 0.0f;
      for (size_t k = 0; k < n_taps; ++k) {
        const int64_t e0 = first + i + (int64_t)((q[k] >> 8) - 7) - in_first;   // the row element under c[0]
        const uint32_t* row = in + (size_t)mics[k] * istride;
        float x[COEFS];
        for (int t = 0; t < COEFS; ++t) {
          const int64_t idx = e0 + t;
          x[t] = idx >= 0 && idx < n_in ? sample_of<DT>(row[idx]) : 0.0f;
        }
        const float a = tap_sample(coef + COEFS * k, x);
        y = k == 0 ? a : y + a;
      }
      float& ch = chain[((i - seg) % STEP) / 4];
      ch = chain_add(ch, y);
    }
    for (int h = 32; h >= 1; h >>= 1)
      for (int l = 0; l < h; ++l) chain[l] = chain[l] + chain[l + h];
    total = total + (double)chain[0];
  }
  return total;
}

// the ranges that uc_scan_power and uc_scan_power_row share
int check_ranges(const char* who, uint64_t in_first, size_t n_in, uint64_t first, size_t window_len) {
  if (n_in == 0 || window_len == 0) return fail(-EINVAL, "%s: n_in or window_len is 0", who);
  if (in_first > SAMPLE_MAX || first > SAMPLE_MAX || n_in > STRIDE_MAX || window_len > STRIDE_MAX) return fail(-EINVAL, "%s: sample range too large", who);
  return 0;
}

}  // namespace

extern "C" {

int uc_scan_abi_version(void) { return UC_SCAN_ABI_VERSION; }

const char* uc_scan_last_error(void) { return g_err.c_str(); }

int uc_scan_quantise(double delay_samples, int32_t* q) {
  if (!q) return fail(-EINVAL, "uc_scan_quantise: q is NULL");
  if (!std::isfinite(delay_samples) || std::fabs(delay_samples) > DELAY_MAX)
    return fail(-EINVAL, "uc_scan_quantise: delay_samples must be finite, |delay_samples| <= 2^20");
  *q = (int32_t)std::llrint(delay_samples * 256.0);   // (the product is exact; the default rounding mode: ties to even)
  return 0;
}

int uc_scan_table(float weight, float table[UC_SCAN_FRACTIONS * UC_SCAN_COEFS]) {
  if (!table) return fail(-EINVAL, "uc_scan_table: table is NULL");
  if (!std::isfinite(weight)) return fail(-EINVAL, "uc_scan_table: weight is not finite");
  for (int f = 0; f < FRACTIONS; ++f) coefficient_row(f, weight, table + COEFS * f);
  return 0;
}

int uc_scan_power_row(const void* in, int in_dtype, size_t n_rows, uint64_t in_first, size_t n_in, size_t in_stride, const uint32_t* mics,
                      const float* weights, const int32_t* q, size_t n_taps, uint64_t first, size_t window_len, double* power) {
  static const char WHO[] = "uc_scan_power_row";
  if (!in || !mics || !weights || !q || !power) return fail(-EINVAL, "uc_scan_power_row: in, mics, weights, q or power is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (n_taps < 1 || n_taps > (size_t)MAX_TAPS) return fail(-EINVAL, "uc_scan_power_row: n_taps %zu not in 1 .. %d", n_taps, MAX_TAPS);
  if (int rc = check_ranges(WHO, in_first, n_in, first, window_len)) return rc;
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  const size_t istride = stride_or(in_stride, n_in);
  if (istride > STRIDE_MAX) return fail(-EINVAL, "uc_scan_power_row: stride too large");
  float coef[MAX_TAPS * COEFS];
  for (size_t k = 0; k < n_taps; ++k) {
    if (mics[k] >= n_rows) return fail(-EINVAL, "uc_scan_power_row: tap %zu: mic %u >= n_rows %zu", k, mics[k], n_rows);
    if (!std::isfinite(weights[k])) return fail(-EINVAL, "uc_scan_power_row: tap %zu: weight is not finite", k);
    if (q[k] > Q_MAX || q[k] < -Q_MAX) return fail(-EINVAL, "uc_scan_power_row: tap %zu: |q| %d > 2^28", k, q[k]);
    coefficient_row(q[k] & 255, weights[k], coef + COEFS * k);
  }
  *power = in_dtype == DT_F32
               ? power_row<DT_F32>((const uint32_t*)in, (int64_t)in_first, (int64_t)n_in, istride, mics, q, n_taps, coef, (int64_t)first, (int64_t)window_len)
               : power_row<DT_I32>((const uint32_t*)in, (int64_t)in_first, (int64_t)n_in, istride, mics, q, n_taps, coef, (int64_t)first, (int64_t)window_len);
  return 0;
}

int uc_scan_create(int device, uc_scan** out) {
  DeviceGuard guard;
  return open("uc_scan_create", "UC_SCAN_GRID", device, out);
}

void uc_scan_destroy(uc_scan* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  (void)hipDeviceSynchronize();      // the calls stage nothing and leave no event to wait for
  if (l->set_dev) (void)hipFree(l->set_dev);
  if (l->scratch.dev) (void)hipFree(l->scratch.dev);
  delete l;
}

int uc_scan_set_beams(uc_scan* l, const uint32_t* mics, const float* weights, size_t n_taps, const double* delays, size_t n_beams, size_t delay_stride) {
  static const char WHO[] = "uc_scan_set_beams";
  if (!l) return fail(-EINVAL, "uc_scan_set_beams: scan is NULL");
  if (!mics || !weights || !delays) return fail(-EINVAL, "uc_scan_set_beams: mics, weights or delays is NULL");
  if (n_taps < 1 || n_taps > (size_t)MAX_TAPS) return fail(-EINVAL, "uc_scan_set_beams: n_taps %zu not in 1 .. %d", n_taps, MAX_TAPS);
  if (n_beams < 1 || n_beams > (size_t)UC_SCAN_MAX_BEAMS) return fail(-EINVAL, "uc_scan_set_beams: n_beams %zu not in 1 .. %d", n_beams, UC_SCAN_MAX_BEAMS);
  if (int rc = check_stride(WHO, "delay_stride", delay_stride, "n_taps", n_taps)) return rc;
  const size_t dstride = stride_or(delay_stride, n_taps);
  if (dstride > STRIDE_MAX) return fail(-EINVAL, "uc_scan_set_beams: stride too large");
  for (size_t k = 0; k < n_taps; ++k)
    if (!std::isfinite(weights[k])) return fail(-EINVAL, "uc_scan_set_beams: tap %zu: weight is not finite", k);
  // ---- the set on the host: tables, quantised delays, the image's lowest shift per tap, the beams that do not fit it
  const size_t table_bytes = n_taps * FRACTIONS * COEFS * sizeof(float), q_bytes = n_beams * n_taps * sizeof(int32_t);
  std::vector<char> host(table_bytes + q_bytes + n_beams);
  float* const table = (float*)host.data();
  int32_t* const q = (int32_t*)(host.data() + table_bytes);
  uint8_t* const direct = (uint8_t*)(host.data() + table_bytes + q_bytes);
  for (size_t b = 0; b < n_beams; ++b)
    for (size_t k = 0; k < n_taps; ++k) {
      const double d = delays[b * dstride + k];
      if (!std::isfinite(d) || std::fabs(d) > DELAY_MAX)
        return fail(-EINVAL, "uc_scan_set_beams: beam %zu, tap %zu: the delay must be finite, |delay| <= 2^20", b, k);
      q[b * n_taps + k] = (int32_t)std::llrint(d * 256.0);
    }
  int32_t lo[MAX_TAPS];
  uint32_t max_mic = 0;
  std::vector<int32_t> shifts(n_beams);
  for (size_t k = 0; k < n_taps; ++k) {
    max_mic = std::max(max_mic, mics[k]);
    for (int f = 0; f < FRACTIONS; ++f) coefficient_row(f, weights[k], table + (k * FRACTIONS + f) * COEFS);
    // [lo, lo + SPREAD] holds the shifts of as many beams as any other such range (the lowest on a tie)
    for (size_t b = 0; b < n_beams; ++b) shifts[b] = (q[b * n_taps + k] >> 8) - 7;
    std::sort(shifts.begin(), shifts.end());
    size_t most = 0, hi = 0;
    lo[k] = shifts[0];
    for (size_t b = 0; b < n_beams; ++b) {
      while (hi < n_beams && shifts[hi] <= shifts[b] + SPREAD) ++hi;
      if (hi - b > most) {
        most = hi - b;
        lo[k] = shifts[b];
      }
    }
  }
  uint32_t n_direct = 0;
  for (size_t b = 0; b < n_beams; ++b) {
    direct[b] = 0;
    for (size_t k = 0; k < n_taps; ++k) {
      const int32_t s = (q[b * n_taps + k] >> 8) - 7;
      if (s < lo[k] || s > lo[k] + SPREAD) direct[b] = 1;
    }
    n_direct += direct[b];
  }
  // ---- onto the device, into memory of its own; the old set goes only when the new one is there
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  void* fresh = nullptr;
  if ((e = hipMalloc(&fresh, host.size())) != hipSuccess) {
    (void)hipGetLastError();
    return fail(-ENOMEM, "uc_scan_set_beams: %zu bytes of the steering set: %s", host.size(), hipGetErrorString(e));
  }
  if ((e = hipMemcpy(fresh, host.data(), host.size(), hipMemcpyHostToDevice)) != hipSuccess) {
    (void)hipFree(fresh);
    return hip_fail(e, WHO, "hipMemcpy");
  }
  if ((e = hipDeviceSynchronize()) != hipSuccess) {   // no launch may still read the old set
    (void)hipFree(fresh);
    return hip_fail(e, WHO, "hipDeviceSynchronize");
  }
  if (l->set_dev) (void)hipFree(l->set_dev);
  l->set_dev = fresh;
  l->n_taps = (uint32_t)n_taps;
  l->n_beams = (uint32_t)n_beams;
  l->n_direct = n_direct;
  l->max_mic = max_mic;
  for (size_t k = 0; k < n_taps; ++k) {
    l->mic[k] = mics[k];
    l->lo[k] = lo[k];
  }
  return 0;
}

int uc_scan_direct_beams(const uc_scan* l, uint32_t* n_direct) {
  if (!l || !n_direct) return fail(-EINVAL, "uc_scan_direct_beams: scan or n_direct is NULL");
  if (l->n_beams == 0) return fail(-EINVAL, "uc_scan_direct_beams: no steering set: call uc_scan_set_beams first");
  *n_direct = l->n_direct;
  return 0;
}

int uc_scan_power(uc_scan* l, const void* in_dev, int in_dtype, size_t n_rows, uint64_t in_first, size_t n_in, size_t in_stride, size_t n_arrays,
                  size_t array_rows, uint64_t first, size_t window_len, size_t hop, size_t n_windows, double* power_dev, size_t power_stride,
                  uc_scan_best* best_dev, void* hip_stream) {
  static const char WHO[] = "uc_scan_power";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_scan_power: scan is NULL");
  if (!in_dev) return fail(-EINVAL, "uc_scan_power: in_dev is NULL");
  if (!power_dev && !best_dev) return fail(-EINVAL, "uc_scan_power: power_dev and best_dev are both NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (int rc = check_count(WHO, "n_arrays", n_arrays)) return rc;
  if (int rc = check_count(WHO, "array_rows", array_rows)) return rc;
  if (int rc = check_count(WHO, "n_windows", n_windows)) return rc;
  if (int rc = check_ranges(WHO, in_first, n_in, first, window_len)) return rc;
  if (hop == 0 || hop > STRIDE_MAX) return fail(-EINVAL, "uc_scan_power: hop %zu not in 1 .. 2^40", hop);
  if ((uint64_t)n_arrays * array_rows > n_rows)   // (both below 2^32)
    return fail(-EINVAL, "uc_scan_power: n_arrays %zu x array_rows %zu > n_rows %zu", n_arrays, array_rows, n_rows);
  if ((n_windows - 1) > (SPAN_MAX - first - window_len) / hop) return fail(-EINVAL, "uc_scan_power: first + n_windows * hop + window_len > 2^53");
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  const size_t istride = stride_or(in_stride, n_in);
  if (int rc = check_strides_max(WHO, istride, power_stride)) return rc;
  if (n_rows > (1ull << 58) / istride) return fail(-EINVAL, "uc_scan_power: n_rows * in_stride too large");
  if (((uintptr_t)in_dev & 3u) != 0 || ((uintptr_t)power_dev & 7u) != 0 || ((uintptr_t)best_dev & 7u) != 0)
    return fail(-EINVAL, "uc_scan_power: in_dev is not a multiple of 4, or power_dev or best_dev not of 8");
  if (l->n_beams == 0) return fail(-EINVAL, "uc_scan_power: no steering set: call uc_scan_set_beams first");
  const size_t n_beams = l->n_beams;
  if (l->max_mic >= array_rows) return fail(-EINVAL, "uc_scan_power: the set's mic %u >= array_rows %zu", l->max_mic, array_rows);
  if (int rc = check_stride(WHO, "power_stride", power_stride, "n_beams", n_beams)) return rc;
  const size_t pstride = stride_or(power_stride, n_beams);
  const uint64_t rows = (uint64_t)n_arrays * n_windows;
  if (rows > COUNT_MAX / n_beams) return fail(-EINVAL, "uc_scan_power: more than 2^32 - 1 (array, window, beam) triples");
  const size_t in_bytes = span_bytes(n_rows, istride, n_in, 4), power_bytes = span_bytes(rows, pstride, n_beams, 8), best_bytes = rows * sizeof(Best);
  if (power_dev)
    if (int rc = check_disjoint(WHO, "power_dev", power_dev, power_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (best_dev)
    if (int rc = check_disjoint(WHO, "best_dev", best_dev, best_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (power_dev && best_dev)
    if (int rc = check_disjoint(WHO, "best_dev", best_dev, best_bytes, "power_dev", power_dev, power_bytes)) return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (power_dev)
    if (int rc = check_on_device(WHO, "power_dev", power_dev, l->device)) return rc;
  if (best_dev)
    if (int rc = check_on_device(WHO, "best_dev", best_dev, l->device)) return rc;
  // the powers of a call without power_dev: the object's scratch, rows without a gap.  It grows behind everything in flight.
  const size_t spstride = power_dev ? pstride : n_beams;
  if (!power_dev) {
    const size_t bytes = rows * n_beams * sizeof(double);
    if (bytes > l->scratch.cap && (e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, WHO, "hipDeviceSynchronize");
    if (int rc = reserve_device(&l->scratch, &l->slot[0], bytes, WHO, "powers")) return rc;
  }

  // ---- the launches
  Params p;
  memset(&p, 0, sizeof(p));
  const size_t table_bytes = (size_t)l->n_taps * FRACTIONS * COEFS * sizeof(float), q_bytes = n_beams * l->n_taps * sizeof(int32_t);
  p.in = in_dev;
  p.power = power_dev ? power_dev : (double*)l->scratch.dev;
  p.table = (const float*)l->set_dev;
  p.q = (const int32_t*)((const char*)l->set_dev + table_bytes);
  p.direct = (const uint8_t*)l->set_dev + table_bytes + q_bytes;
  p.in_first = (int64_t)in_first;
  p.n_in = (int64_t)n_in;
  p.first = (int64_t)first;
  p.window_len = (int64_t)window_len;
  p.hop = (int64_t)hop;
  p.in_stride = istride;
  p.power_stride = spstride;
  p.array_rows = array_rows;
  p.n_taps = l->n_taps;
  p.n_beams = l->n_beams;
  p.n_windows = (uint32_t)n_windows;
  p.n_arrays = (uint32_t)n_arrays;
  p.beam_groups = (uint32_t)((n_beams + GROUP - 1) / GROUP);
  for (uint32_t k = 0; k < l->n_taps; ++k) {
    p.mic[k] = l->mic[k];
    p.lo[k] = l->lo[k];
  }
  const int variant = in_dtype | (l->n_taps > (uint32_t)SMALL_TAPS ? 2 : 0);
  const uint64_t grid = persistent_grid(l, variant, resident_blocks_per_cu, 3, rows * p.beam_groups);
  hipStream_t hs = (hipStream_t)hip_stream;
  e = (hipError_t)launch_power(in_dtype, (unsigned)grid, hs, p);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  if (best_dev) {
    uint64_t bgrid = (uint64_t)l->cus * 8;
    if (l->grid_override) bgrid = l->grid_override;
    if (bgrid > rows) bgrid = rows;
    e = (hipError_t)launch_best((unsigned)bgrid, hs, p.power, spstride, l->n_beams, (uint32_t)rows, (Best*)best_dev);
    if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  }
  return 0;
}

}  // extern "C"
