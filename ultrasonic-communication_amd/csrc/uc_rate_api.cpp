// uc_rate_api.cpp -- the C-ABI of include/uchirp_rate.h on top of uc_rate_kernel.hip: the plan of a ratio, the prototype and
// its table, the integer step, the checks that are its own, the launch.  The object's base, create and destroy, the grid and
// the checks of the row matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library
// boundary): libuchirp_rate.so stands alone.  A call reads no host array, so the base's staging slots stay empty.  No CPU
// compute path exists here: without a usable HIP device uc_rate_create fails.  Every entry point leaves the calling thread's
// current HIP device as it found it.
#include "../../include/uchirp_rate.h"
#include "uc_host.hpp"
#include "uc_rate.hpp"

using namespace uc_rate_dev;

static_assert(sizeof(uc_rate_info) == 24, "layout of uchirp_rate.h");
static_assert(UC_RATE_DTYPE_I16 == DT_I16 && UC_RATE_DTYPE_F32 == DT_F32, "dtype values");
static_assert(UC_RATE_TAPS_MAX == TAPS_MAX && UC_RATE_RATIO_MAX == RATIO_MAX, "limits");
static_assert(TAPS_MAX < WINDOW, "a window holds the samples under one output and more");

struct uc_rate : HostBase {
  uc_rate_info info = {};
  uint32_t tile = 0;               // outputs of one tile (uc_rate.hpp)
  float* table = nullptr;          // D[j][f] on the device (uc_rate.hpp), written once by uc_rate_create
};

namespace {

constexpr double BETA_MAX = 100.0;
constexpr uint64_t SAMPLE_END_MAX = 1ull << 38;

// I0(x), the modified Bessel function of order 0, by its power series: sum ((x / 2)^2k / (k!)^2); x is 0 .. 100 here
// (the terms grow until k = x / 2 and stay below 1e43)
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 2000; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

uint32_t gcd32(uint32_t a, uint32_t b) {
  while (b) {
    const uint32_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

bool beta_ok(double beta) { return std::isfinite(beta) && beta >= 0.0 && beta <= BETA_MAX; }

// the plan of the definition; the message names `who`
int make_plan(const char* who, uint32_t up, uint32_t down, uint32_t half, double beta, uc_rate_info* info) {
  if (up == 0 || down == 0) return fail(-EINVAL, "%s: up or down is 0", who);
  const uint32_t g = gcd32(up, down);
  up /= g;
  down /= g;
  if (up == down) return fail(-EINVAL, "%s: the ratio is 1", who);
  if (up > RATIO_MAX || down > RATIO_MAX) return fail(-EINVAL, "%s: %u / %u: up or down > %u after the reduction", who, up, down, RATIO_MAX);
  if (half < UC_RATE_HALF_MIN || half > UC_RATE_HALF_MAX) return fail(-EINVAL, "%s: half %u not in %d .. %d", who, half, UC_RATE_HALF_MIN, UC_RATE_HALF_MAX);
  if (!beta_ok(beta)) return fail(-EINVAL, "%s: beta must be finite and in 0 .. 100", who);
  const uint32_t q = up > down ? up : down;
  const uint32_t taps = 2 * half * q / up + 1;
  if (taps > (uint32_t)TAPS_MAX) return fail(-EINVAL, "%s: %u / %u at half %u needs %u taps > %d", who, up, down, half, taps, TAPS_MAX);
  if (up * taps > UC_RATE_TABLE_MAX) return fail(-EINVAL, "%s: %u / %u at half %u: a table of %u floats > 2^19", who, up, down, half, up * taps);
  info->up = up;
  info->down = down;
  info->half = half;
  info->taps = taps;
  info->centre = half * q;
  info->table_len = up * taps;
  return 0;
}

// is *info what uc_rate_plan makes (of its own up, down and half)?
int check_info(const char* who, const uc_rate_info* info) {
  if (!info) return fail(-EINVAL, "%s: info is NULL", who);
  uc_rate_info again;
  if (info->up == 0 || info->down == 0 || gcd32(info->up, info->down) != 1 || make_plan(who, info->up, info->down, info->half, 0.0, &again) != 0 ||
      memcmp(&again, info, sizeof(again)) != 0)
    return fail(-EINVAL, "%s: info is not what uc_rate_plan made", who);
  return 0;
}

// the prototype h of the definition, N_h = 2 c + 1 doubles
std::vector<double> prototype(const uc_rate_info& f, double beta) {
  const double pi = 3.14159265358979323846;
  const int64_t c = f.centre;
  const double q = (double)(f.up > f.down ? f.up : f.down);
  const double i0_beta = bessel_i0(beta);
  std::vector<double> h((size_t)(2 * c + 1));
  double sum = 0.0;
  for (int64_t i = 0; i <= 2 * c; ++i) {
    const double u = (double)(i - c) / q;
    const double r = (double)(i - c) / (double)c;
    const double s = i == c ? 1.0 : std::sin(pi * u) / (pi * u);
    // 1 - r^2 is exactly 0 at both ends (r = -1, 1)
    h[(size_t)i] = s * bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0_beta;
    sum += h[(size_t)i];
  }
  const double scale = (double)f.up / sum;
  for (double& v : h) v *= scale;
  return h;
}

// C[p][j] of the definition
inline float coefficient(const std::vector<double>& h, const uc_rate_info& f, uint32_t p, uint32_t j) {
  const size_t i = (size_t)p + (size_t)j * f.up;
  return i < h.size() ? (float)h[i] : 0.0f;
}

inline void step(const uc_rate_info& f, uint64_t m, int64_t* k, uint32_t* phase) {
  const uint64_t pos = m * f.down + f.centre;      // below 2^51
  *k = (int64_t)(pos / f.up);
  *phase = (uint32_t)(pos % f.up);
}

}  // namespace

extern "C" {

int uc_rate_abi_version(void) { return UC_RATE_ABI_VERSION; }

const char* uc_rate_last_error(void) { return g_err.c_str(); }

int uc_rate_plan(uint32_t up, uint32_t down, uint32_t half, double beta, uc_rate_info* info) {
  if (!info) return fail(-EINVAL, "uc_rate_plan: info is NULL");
  uc_rate_info f;
  if (int rc = make_plan("uc_rate_plan", up, down, half, beta, &f)) return rc;
  *info = f;
  return 0;
}

int uc_rate_table(const uc_rate_info* info, double beta, float* table, size_t len) {
  if (int rc = check_info("uc_rate_table", info)) return rc;
  if (!table) return fail(-EINVAL, "uc_rate_table: table is NULL");
  if (!beta_ok(beta)) return fail(-EINVAL, "uc_rate_table: beta must be finite and in 0 .. 100");
  if (len != info->table_len) return fail(-EINVAL, "uc_rate_table: len %zu is not table_len %u", len, info->table_len);
  const std::vector<double> h = prototype(*info, beta);
  for (uint32_t p = 0; p < info->up; ++p)
    for (uint32_t j = 0; j < info->taps; ++j) table[(size_t)p * info->taps + j] = coefficient(h, *info, p, j);
  return 0;
}

int uc_rate_step(const uc_rate_info* info, uint64_t m, int64_t* k, uint32_t* phase) {
  if (int rc = check_info("uc_rate_step", info)) return rc;
  if (!k || !phase) return fail(-EINVAL, "uc_rate_step: k or phase is NULL");
  if (m >= SAMPLE_END_MAX) return fail(-EINVAL, "uc_rate_step: m >= 2^38");
  step(*info, m, k, phase);
  return 0;
}

int uc_rate_span(const uc_rate_info* info, uint64_t out_first, size_t n_out, int64_t* in_lo, int64_t* in_hi) {
  if (int rc = check_info("uc_rate_span", info)) return rc;
  if (!in_lo || !in_hi) return fail(-EINVAL, "uc_rate_span: in_lo or in_hi is NULL");
  if (n_out == 0) return fail(-EINVAL, "uc_rate_span: n_out is 0");
  if (out_first > SAMPLE_END_MAX || n_out > SAMPLE_END_MAX || out_first + n_out > SAMPLE_END_MAX)
    return fail(-EINVAL, "uc_rate_span: out_first + n_out > 2^38");
  int64_t k;
  uint32_t p;
  step(*info, out_first, &k, &p);
  *in_lo = k - (int64_t)(info->taps - 1);
  step(*info, out_first + n_out - 1, &k, &p);
  *in_hi = k + 1;
  return 0;
}

int64_t uc_rate_count(const uc_rate_info* info, uint64_t n_in) {
  if (int rc = check_info("uc_rate_count", info)) return rc;
  if (n_in > (1ull << 40)) return fail(-EINVAL, "uc_rate_count: n_in > 2^40");
  return (int64_t)((n_in * info->up + info->down - 1) / info->down);     // below 2^53
}

int uc_rate_create(int device, uint32_t up, uint32_t down, uint32_t half, double beta, uc_rate** out) {
  if (!out) return fail(-EINVAL, "uc_rate_create: out is NULL");
  *out = nullptr;
  uc_rate_info f;
  if (int rc = make_plan("uc_rate_create", up, down, half, beta, &f)) return rc;
  DeviceGuard guard;
  int rc = open("uc_rate_create", "UC_RATE_GRID", device, out);
  if (rc) return rc;
  uc_rate* l = *out;
  l->info = f;
  l->tile = tile_outputs(f.up, f.down, f.taps);
  // the table by output phase, transposed (uc_rate.hpp): computed once, copied with a synchronous copy (pageable memory:
  // done when the call returns)
  const std::vector<double> h = prototype(f, beta);
  std::vector<float> host((size_t)f.table_len);
  for (uint32_t ph = 0; ph < f.up; ++ph) {
    const uint32_t p = (uint32_t)(((uint64_t)ph * f.down + f.centre) % f.up);
    for (uint32_t j = 0; j < f.taps; ++j) host[(size_t)j * f.up + ph] = coefficient(h, f, p, j);
  }
  hipError_t e;
  if ((e = hipMalloc((void**)&l->table, host.size() * sizeof(float))) != hipSuccess ||
      (e = hipMemcpy(l->table, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) {
    uc_rate_destroy(l);
    *out = nullptr;
    return hip_fail(e, "uc_rate_create", "the table");
  }
  return 0;
}

void uc_rate_destroy(uc_rate* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  (void)hipDeviceSynchronize();      // the calls stage nothing and leave no event to wait for
  if (l->table) (void)hipFree(l->table);
  delete l;
}

int uc_rate_convert(uc_rate* l, const void* in_dev, int in_dtype, size_t n_rows, uint64_t in_first, size_t n_in, size_t in_stride,
                    float* out_dev, uint64_t out_first, size_t n_out, size_t out_stride, void* hip_stream) {
  static const char WHO[] = "uc_rate_convert";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_rate_convert: rate is NULL");
  if (!in_dev || !out_dev) return fail(-EINVAL, "uc_rate_convert: in_dev or out_dev is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (n_in == 0 || n_out == 0) return fail(-EINVAL, "uc_rate_convert: n_in or n_out is 0");
  if (in_first > (1ull << 52) || n_in > (1ull << 40)) return fail(-EINVAL, "uc_rate_convert: sample range too large");
  if (out_first > SAMPLE_END_MAX || n_out > SAMPLE_END_MAX || out_first + n_out > SAMPLE_END_MAX)
    return fail(-EINVAL, "uc_rate_convert: out_first + n_out > 2^38");
  const size_t istride = stride_or(in_stride, n_in), ostride = stride_or(out_stride, n_out);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_stride(WHO, "out_stride", out_stride, "n_out", n_out)) return rc;
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_rows, istride, n_rows, ostride, 1ull << 58, "n_rows * out_stride")) return rc;
  const size_t elem = in_dtype == DT_I16 ? 2 : 4;
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, span_bytes(n_rows, ostride, n_out, 4), "in_dev", in_dev, span_bytes(n_rows, istride, n_in, elem)))
    return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  // (the first check that reads the object's own fields: out_dev is memory of this device, so n_out floats fit it)
  const uint64_t tiles_per_row = (n_out + l->tile - 1) / l->tile;
  if (tiles_per_row > 0x7FFFFFFFull) return fail(-EINVAL, "uc_rate_convert: n_out %zu is more than 2^31 - 1 tiles of %u", n_out, l->tile);

  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.out = out_dev;
  p.table = l->table;
  p.in_first = (int64_t)in_first;
  p.n_in = (int64_t)n_in;
  p.out_first = (int64_t)out_first;
  p.n_out = (int64_t)n_out;
  p.in_stride = istride;
  p.out_stride = ostride;
  p.tiles_per_row = (uint32_t)tiles_per_row;
  p.row_blocks = (uint32_t)((n_rows + ROWS - 1) / ROWS);
  p.n_rows = (uint32_t)n_rows;
  p.up = l->info.up;
  p.down = l->info.down;
  p.taps = l->info.taps;
  p.centre = l->info.centre;
  p.tile = l->tile;
  const uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 5, (uint64_t)p.row_blocks * tiles_per_row);

  // ---- enqueue
  e = (hipError_t)launch_convert(in_dtype, (unsigned)grid, hip_stream, p);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  return 0;
}

}  // extern "C"
