// uc_retime_api.cpp -- the C-ABI of include/uchirp_retime.h on top of uc_retime_kernel.hip: the object and its table, the
// fixed-point step, the checks and the staging that are its own, the launch.  The object's base, create and destroy, the
// staging protocol, the grid and the checks of the row matrices are the shared host layer's (uc_host.hpp: header-only,
// nothing crosses a library boundary): libuchirp_retime.so stands alone.  No CPU compute path exists here: without a
// usable HIP device uc_retime_create fails.  Every entry point leaves the calling thread's current HIP device as it found
// it.
#include "../../include/uchirp_retime.h"
#include "uc_host.hpp"
#include "uc_retime.hpp"

using namespace uc_retime_dev;

static_assert(sizeof(uc_retime_line) == 24 && sizeof(Line) == 24, "layouts of uchirp_retime.h and the kernel's line record");
static_assert(UC_RETIME_COEFS == COEFS && UC_RETIME_TABLE_ROWS == TABLE_ROWS, "the table's shape");
static_assert(UC_RETIME_DTYPE_I32 == DT_I32 && UC_RETIME_DTYPE_F32 == DT_F32, "dtype values");

// staging: [n_lines Line records]
struct uc_retime : HostBase {
  float* table = nullptr;          // T[257][16] on the device, written once by uc_retime_create
};

namespace {

constexpr double DELAY_MAX = 1073741824.0;   // 2^30
constexpr double SLOPE_MAX = 0.001953125;    // 2^-9
constexpr double TWO32 = 4294967296.0;
constexpr uint64_t SAMPLE_END_MAX = 1ull << 38;

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

bool line_ok(double delay, double slope) {
  return std::isfinite(delay) && std::isfinite(slope) && std::fabs(delay) <= DELAY_MAX && std::fabs(slope) <= SLOPE_MAX;
}

// the table of the definition (include/uchirp_retime.h): row q the coefficients of uchirp_array.h at the fraction q / 256
// and weight 1, operation for operation as uc_array_tap_coefficients evaluates them
void fill_table(float* t) {
  const double pi = 3.14159265358979323846;
  const double i0_beta = bessel_i0(8.0);
  const double weight = (double)1.0f;
  for (int q = 0; q < TABLE_ROWS; ++q) {
    float* c = t + COEFS * q;
    if (q == 0 || q == TABLE_ROWS - 1) {
      for (int i = 0; i < COEFS; ++i) c[i] = 0.0f;
      c[q == 0 ? 7 : 8] = 1.0f;
      continue;
    }
    const double f = (double)q / 256.0;
    for (int i = 0; i < COEFS; ++i) {
      const double u = (double)(i - 7) - f;
      const double r = u / 8.0;
      c[i] = (float)(weight * (std::sin(pi * u) / (pi * u)) * bessel_i0(8.0 * std::sqrt(1.0 - r * r)) / i0_beta);
    }
  }
}

}  // namespace

extern "C" {

int uc_retime_abi_version(void) { return UC_RETIME_ABI_VERSION; }

const char* uc_retime_last_error(void) { return g_err.c_str(); }

int uc_retime_fixed(double delay_samples, double slope, int64_t* lead_fx, int64_t* drift_fx) {
  if (!lead_fx || !drift_fx) return fail(-EINVAL, "uc_retime_fixed: lead_fx or drift_fx is NULL");
  if (!line_ok(delay_samples, slope))
    return fail(-EINVAL, "uc_retime_fixed: delay_samples and slope must be finite, |delay_samples| <= 2^30, |slope| <= 2^-9");
  // the products are exact (a power of two) and at most 2^62 and 2^23 in magnitude
  *lead_fx = (int64_t)std::llrint(delay_samples * TWO32);
  *drift_fx = (int64_t)std::llrint(slope * TWO32);
  return 0;
}

int uc_retime_table(float table[UC_RETIME_TABLE_ROWS * UC_RETIME_COEFS]) {
  if (!table) return fail(-EINVAL, "uc_retime_table: table is NULL");
  fill_table(table);
  return 0;
}

int uc_retime_create(int device, uc_retime** out) {
  DeviceGuard guard;
  int rc = open("uc_retime_create", "UC_RETIME_GRID", device, out);
  if (rc) return rc;
  // the table: computed once, copied with a synchronous copy (pageable memory: done when the call returns)
  uc_retime* l = *out;
  float host_table[TABLE_ROWS * COEFS];
  fill_table(host_table);
  hipError_t e;
  if ((e = hipMalloc((void**)&l->table, sizeof(host_table))) != hipSuccess ||
      (e = hipMemcpy(l->table, host_table, sizeof(host_table), hipMemcpyHostToDevice)) != hipSuccess) {
    uc_retime_destroy(l);
    *out = nullptr;
    return hip_fail(e, "uc_retime_create", "the table");
  }
  return 0;
}

void uc_retime_destroy(uc_retime* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  if (l->table) (void)hipFree(l->table);
  delete l;
}

int uc_retime_rows(uc_retime* l, const void* in_dev, int in_dtype, size_t n_mics, uint64_t in_first, size_t n_in, size_t in_stride,
                   const uc_retime_line* lines, size_t n_lines, float* out_dev, uint64_t out_first, size_t n_out, size_t out_stride,
                   void* hip_stream) {
  static const char WHO[] = "uc_retime_rows";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_retime_rows: retime is NULL");
  if (!in_dev || !out_dev) return fail(-EINVAL, "uc_retime_rows: in_dev or out_dev is NULL");
  if (!lines) return fail(-EINVAL, "uc_retime_rows: lines is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_mics", n_mics)) return rc;
  if (int rc = check_count(WHO, "n_lines", n_lines)) return rc;
  if (n_in == 0 || n_out == 0) return fail(-EINVAL, "uc_retime_rows: n_in or n_out is 0");
  if (in_first > (1ull << 52) || n_in > (1ull << 40)) return fail(-EINVAL, "uc_retime_rows: sample range too large");
  if (out_first > SAMPLE_END_MAX || n_out > SAMPLE_END_MAX || out_first + n_out > SAMPLE_END_MAX)
    return fail(-EINVAL, "uc_retime_rows: out_first + n_out > 2^38");
  const size_t istride = stride_or(in_stride, n_in), ostride = stride_or(out_stride, n_out);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_stride(WHO, "out_stride", out_stride, "n_out", n_out)) return rc;
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_mics, istride, n_lines, ostride, 1ull << 58, "n_lines * out_stride")) return rc;
  for (size_t k = 0; k < n_lines; ++k) {
    const uc_retime_line& q = lines[k];
    if (q.mic >= n_mics) return fail(-EINVAL, "uc_retime_rows: line %zu: mic %u >= n_mics %zu", k, q.mic, n_mics);
    if (q.reserved != 0) return fail(-EINVAL, "uc_retime_rows: line %zu: reserved is %u, not 0", k, q.reserved);
    if (!line_ok(q.delay_samples, q.slope))
      return fail(-EINVAL, "uc_retime_rows: line %zu: delay_samples and slope must be finite, |delay_samples| <= 2^30, |slope| <= 2^-9", k);
  }
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, span_bytes(n_lines, ostride, n_out, 4), "in_dev", in_dev, span_bytes(n_mics, istride, n_in, 4)))
    return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  const size_t bytes = n_lines * sizeof(Line);
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  Line* rec = (Line*)sl->pinned;
  for (size_t k = 0; k < n_lines; ++k) {
    rec[k].lead_fx = (int64_t)std::llrint(lines[k].delay_samples * TWO32);
    rec[k].drift_fx = (int64_t)std::llrint(lines[k].slope * TWO32);
    rec[k].row = (uint64_t)lines[k].mic * istride;
  }
  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.out = out_dev;
  p.table = l->table;
  p.in_first = (int64_t)in_first;
  p.n_in = (int64_t)n_in;
  p.out_first = (int64_t)out_first;
  p.n_out = (int64_t)n_out;
  p.out_stride = ostride;
  const uint64_t tiles_per_row = (n_out + TILE_SAMPLES - 1) / TILE_SAMPLES;
  p.tiles_per_row = (uint32_t)tiles_per_row;
  p.n_lines = (uint32_t)n_lines;
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 4, (uint64_t)n_lines * tiles_per_row);

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_rows(in_dtype, (unsigned)grid, hs, p, (const Line*)sl->dev);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
