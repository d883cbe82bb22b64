// uc_mf_api.cpp -- the C-ABI of include/uchirp_mf.h on top of uc_mf_kernel.hip: the object, its twiddle table and its
// spectra, the host functions of the definition (the plan, the spectrum, the selection rule, the arrival), the checks and
// the staging that are its own, the launch.  The object's base, create and destroy, the staging protocol, the grid and the
// checks of the row matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library boundary):
// libuchirp_mf.so stands alone.  No CPU compute path exists here: without a usable HIP device uc_mf_create fails.
// Every entry point leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_mf.h"
#include "uc_mf.hpp"
#include "uc_host.hpp"

using namespace uc_mf_dev;

static_assert(sizeof(uc_mf_job) == 8 && sizeof(uc_mf_candidate) == 16 && sizeof(uc_mf_record) == 80 && sizeof(Job) == 16, "layouts of uchirp_mf.h");
static_assert(sizeof(uc_mf_record) == RECORD_WORDS * 4 && offsetof(uc_mf_record, sum) == 64, "the record as the kernel writes it");
static_assert(UC_MF_POINTS == POINTS && UC_MF_MAX_TAPS == MAX_TAPS && UC_MF_CANDIDATES == CANDIDATES, "the kernel's constants");
static_assert(UC_MF_DTYPE_I32 == DT_I32 && UC_MF_DTYPE_F32 == DT_F32 && UC_MF_DTYPE_C32 == DT_C32, "dtype values");
static_assert(UC_MF_OUT_COMPLEX == OUT_COMPLEX && UC_MF_OUT_REAL == OUT_REAL && UC_MF_OUT_POWER == OUT_POWER && UC_MF_OUT_MAG == OUT_MAG, "formats");
static_assert(POINTS - MAX_TAPS - 1 >= 1, "a hop");

// staging: [n_jobs Job records]
struct uc_mf : HostBase {
  float* tw = nullptr;             // device: exp(-2 pi i k / 2048), k < 2048
  float* spectra = nullptr;        // device: [n_sets][2048] (re, im)
  uint32_t n_sets = 0;             // 0: no templates yet
  uint32_t n_taps = 0;
};

namespace {

int check_taps(const char* who, uint32_t n_taps) {
  return n_taps < 1 || n_taps > (uint32_t)MAX_TAPS ? fail(-EINVAL, "%s: n_taps %u not in 1 .. %d", who, n_taps, MAX_TAPS) : 0;
}

// exp(-2 pi i m / 2048) in double, m < 2048
const std::vector<double>& unit_circle() {
  static const std::vector<double> w = [] {
    std::vector<double> t(2 * (size_t)POINTS);
    for (int m = 0; m < POINTS; ++m) {
      const double a = -2.0 * 3.14159265358979323846 * (double)m / (double)POINTS;
      t[2 * m] = std::cos(a);
      t[2 * m + 1] = std::sin(a);
    }
    // the axes exactly
    t[2 * (POINTS / 4)] = 0.0;
    t[2 * (POINTS / 2) + 1] = 0.0;
    t[2 * (3 * POINTS / 4)] = 0.0;
    return t;
  }();
  return w;
}

// H of the definition; taps are finite
void spectrum_of(const float* taps, uint32_t n_taps, float* out) {
  const std::vector<double>& w = unit_circle();
  for (uint32_t k = 0; k < (uint32_t)POINTS; ++k) {
    double re = 0.0, im = 0.0;
    uint32_t m = 0;                                         // k t mod P
    for (uint32_t t = 0; t < n_taps; ++t) {
      const double hr = taps[2 * t], hi = taps[2 * t + 1], c = w[2 * m], s = w[2 * m + 1];
      re += hr * c - hi * s;
      im += hr * s + hi * c;
      m = (m + k) & (POINTS - 1);
    }
    out[2 * k] = (float)(re / POINTS);
    out[2 * k + 1] = (float)(im / POINTS);
  }
}

int check_finite_taps(const char* who, const float* taps, size_t n) {
  for (size_t i = 0; i < 2 * n; ++i)
    if (!std::isfinite(taps[i])) return fail(-EINVAL, "%s: tap %zu is not finite", who, i / 2);
  return 0;
}

}  // namespace

extern "C" {

int uc_mf_abi_version(void) { return UC_MF_ABI_VERSION; }

const char* uc_mf_last_error(void) { return g_err.c_str(); }

int uc_mf_plan(uint32_t n_taps, uint64_t pos0, size_t first, size_t n, uint32_t* hop, uint64_t* first_segment, uint64_t* n_segments) {
  static const char WHO[] = "uc_mf_plan";
  if (!hop || !first_segment || !n_segments) return fail(-EINVAL, "uc_mf_plan: hop, first_segment or n_segments is NULL");
  if (int rc = check_taps(WHO, n_taps)) return rc;
  if (n == 0) return fail(-EINVAL, "uc_mf_plan: n is 0");
  const uint64_t top = ~0ull;
  if ((uint64_t)first > top - pos0 || (uint64_t)n - 1 > top - pos0 - first) return fail(-EINVAL, "uc_mf_plan: pos0 + first + n beyond 2^64 - 1");
  const uint64_t S = (uint64_t)POINTS - n_taps - 1, q0 = pos0 + first, q1 = q0 + (n - 1);
  *hop = (uint32_t)S;
  *first_segment = q0 / S;
  *n_segments = q1 / S - q0 / S + 1;
  return 0;
}

int uc_mf_spectrum(const float* taps, uint32_t n_taps, float* spectrum) {
  static const char WHO[] = "uc_mf_spectrum";
  if (!taps || !spectrum) return fail(-EINVAL, "uc_mf_spectrum: taps or spectrum is NULL");
  if (int rc = check_taps(WHO, n_taps)) return rc;
  if (int rc = check_finite_taps(WHO, taps, n_taps)) return rc;
  spectrum_of(taps, n_taps, spectrum);
  return 0;
}

int uc_mf_select(const float* e, uint32_t hop, uint32_t lo, uint32_t hi, uc_mf_record* out) {
  if (!e || !out) return fail(-EINVAL, "uc_mf_select: e or out is NULL");
  if (hop < 1 || hop > (uint32_t)POINTS - 2) return fail(-EINVAL, "uc_mf_select: hop %u not in 1 .. %d", hop, POINTS - 2);
  if (lo >= hi || hi > hop) return fail(-EINVAL, "uc_mf_select: outputs %u .. %u of %u", lo, hi, hop);
  memset(out, 0, sizeof(*out));
  float sum = 0.0f;
  for (uint32_t u = lo; u < hi; ++u) {
    const float l = e[u], v = e[u + 1], r = e[u + 2];
    sum += v;
    if (!(v >= l && v > r)) continue;
    out->n_cand++;
    // its place among the kept ones: behind every one that is greater or equal (those have the lower q)
    int at = CANDIDATES;
    while (at > 0 && (out->cand[at - 1].peak == 0.0f || out->cand[at - 1].peak < v)) --at;
    if (at == CANDIDATES) continue;
    for (int m = CANDIDATES - 1; m > at; --m) out->cand[m] = out->cand[m - 1];
    out->cand[at].offset = u;
    out->cand[at].left = l;
    out->cand[at].peak = v;
    out->cand[at].right = r;
  }
  out->sum = sum;
  out->count = hi - lo;
  return 0;
}

int uc_mf_arrival(const uc_mf_candidate* cand, double* offset, double* height) {
  if (!cand || !offset || !height) return fail(-EINVAL, "uc_mf_arrival: cand, offset or height is NULL");
  const double l = cand->left, v = cand->peak, r = cand->right;
  if (!std::isfinite(l) || !std::isfinite(v) || !std::isfinite(r) || l < 0.0 || v < 0.0 || r < 0.0)
    return fail(-EINVAL, "uc_mf_arrival: a value is negative or not finite");
  const double a = std::sqrt(l), b = std::sqrt(v), c = std::sqrt(r), d = a - 2.0 * b + c;
  double delta = 0.0, top = b;
  if (d < 0.0) {
    delta = (a - c) / (2.0 * d);
    top = b - (a - c) * delta / 4.0;
  }
  *offset = (double)cand->offset + delta;
  *height = top;
  return 0;
}

int uc_mf_create(int device, uc_mf** out) {
  DeviceGuard guard;
  int rc = open("uc_mf_create", "UC_MF_GRID", device, out);
  if (rc) return rc;
  if ((rc = device_twiddles(&(*out)->tw, POINTS, "uc_mf_create")) != 0) {
    uc_mf_destroy(*out);
    *out = nullptr;
  }
  return rc;
}

void uc_mf_destroy(uc_mf* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  if (l->spectra) (void)hipFree(l->spectra);
  if (l->tw) (void)hipFree(l->tw);
  delete l;
}

int uc_mf_set_templates(uc_mf* l, const float* taps, uint32_t n_sets, uint32_t n_taps) {
  static const char WHO[] = "uc_mf_set_templates";
  if (!l) return fail(-EINVAL, "uc_mf_set_templates: mf is NULL");
  if (!taps) return fail(-EINVAL, "uc_mf_set_templates: taps is NULL");
  if (n_sets < 1 || n_sets > UC_MF_MAX_SETS) return fail(-EINVAL, "uc_mf_set_templates: n_sets %u not in 1 .. %d", n_sets, UC_MF_MAX_SETS);
  if (int rc = check_taps(WHO, n_taps)) return rc;
  if (int rc = check_finite_taps(WHO, taps, (size_t)n_sets * n_taps)) return rc;
  std::vector<float> h((size_t)n_sets * 2 * POINTS);
  for (uint32_t s = 0; s < n_sets; ++s) spectrum_of(taps + (size_t)s * 2 * n_taps, n_taps, h.data() + (size_t)s * 2 * POINTS);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  float* d = nullptr;
  if ((e = hipMalloc((void**)&d, h.size() * sizeof(float))) != hipSuccess) {
    (void)hipGetLastError();
    return fail(-ENOMEM, "uc_mf_set_templates: %zu bytes of spectra: %s", h.size() * sizeof(float), hipGetErrorString(e));
  }
  if ((e = hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(e, WHO, "hipMemcpy");
  }
  // the calls in flight read the former spectra
  for (StagingSlot& sl : l->slot)
    if (sl.in_flight) (void)hipEventSynchronize(sl.done);
  if (l->spectra) (void)hipFree(l->spectra);
  l->spectra = d;
  l->n_sets = n_sets;
  l->n_taps = n_taps;
  return 0;
}

int uc_mf_run(uc_mf* l, const void* in_dev, int in_dtype, size_t n_rows, size_t n_in, size_t in_stride, const uc_mf_job* jobs,
              size_t n_jobs, uint64_t pos0, size_t first, size_t n, void* out_dev, int out_format, size_t out_stride,
              uc_mf_record* records_dev, void* hip_stream) {
  static const char WHO[] = "uc_mf_run";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_mf_run: mf is NULL");
  if (!in_dev) return fail(-EINVAL, "uc_mf_run: in_dev is NULL");
  if (!out_dev && !records_dev) return fail(-EINVAL, "uc_mf_run: out_dev and records_dev are both NULL");
  if (!jobs) return fail(-EINVAL, "uc_mf_run: jobs is NULL");
  if (in_dtype != DT_I32 && in_dtype != DT_F32 && in_dtype != DT_C32) return fail(-EINVAL, "uc_mf_run: unknown dtype %d", in_dtype);
  if (out_format < OUT_COMPLEX || out_format > OUT_MAG) return fail(-EINVAL, "uc_mf_run: unknown format %d", out_format);
  if (!l->n_sets) return fail(-EINVAL, "uc_mf_run: no templates set (uc_mf_set_templates)");
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (int rc = check_count(WHO, "n_jobs", n_jobs)) return rc;
  if (n_in == 0 || n == 0) return fail(-EINVAL, "uc_mf_run: n_in or n is 0");
  if (n_in > STRIDE_MAX) return fail(-EINVAL, "uc_mf_run: n_in too large");
  if (first > n_in || n > n_in - first) return fail(-EINVAL, "uc_mf_run: first %zu + n %zu > n_in %zu", first, n, n_in);
  if ((uint64_t)n_in - 1 > ~0ull - pos0) return fail(-EINVAL, "uc_mf_run: pos0 + n_in beyond 2^64 - 1");
  const size_t in_elem = in_dtype == DT_C32 ? 8 : 4, out_elem = out_format == OUT_COMPLEX ? 8 : 4;
  const size_t istride = stride_or(in_stride, n_in), ostride = stride_or(out_stride, n);
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_in", n_in)) return rc;
  if (int rc = check_stride(WHO, "out_stride", out_stride, "n", n)) return rc;
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_rows, istride, n_jobs, ostride, 1ull << 57, "n_jobs * out_stride")) return rc;
  for (size_t k = 0; k < n_jobs; ++k)
    if (jobs[k].row >= n_rows || jobs[k].set >= l->n_sets)
      return fail(-EINVAL, "uc_mf_run: job %zu: row %u, set %u; n_rows %zu, n_sets %u", k, jobs[k].row, jobs[k].set, n_rows, l->n_sets);
  uint32_t hop = 0;
  uint64_t seg0 = 0, n_segments = 0;
  if (int rc = uc_mf_plan(l->n_taps, pos0, first, n, &hop, &seg0, &n_segments)) return rc;
  const uint64_t n_units = (uint64_t)n_jobs * n_segments;                // n_segments < 2^40 / 383 + 2
  if (n_segments > 0x7fffffffull || n_units > (1ull << 36))
    return fail(-EINVAL, "uc_mf_run: n_jobs * segments too large for one call (%llu units)", (unsigned long long)n_units);
  const size_t in_bytes = span_bytes(n_rows, istride, n_in, in_elem);
  const size_t out_bytes = span_bytes(n_jobs, ostride, n, out_elem);
  const size_t rec_bytes = (size_t)n_units * sizeof(uc_mf_record);
  if (out_dev)
    if (int rc = check_disjoint(WHO, "out_dev", out_dev, out_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (records_dev)
    if (int rc = check_disjoint(WHO, "records_dev", records_dev, rec_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (out_dev && records_dev)
    if (int rc = check_disjoint(WHO, "records_dev", records_dev, rec_bytes, "out_dev", out_dev, out_bytes)) return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (out_dev)
    if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  if (records_dev)
    if (int rc = check_on_device(WHO, "records_dev", records_dev, l->device)) return rc;
  const size_t bytes = n_jobs * sizeof(Job);
  StagingSlot* sl;
  if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  Job* rec = (Job*)sl->pinned;
  for (size_t k = 0; k < n_jobs; ++k) {
    rec[k].row = (uint64_t)jobs[k].row * istride;
    rec[k].set = jobs[k].set;
    rec[k].pad = 0;
  }
  Params p;
  memset(&p, 0, sizeof(p));
  p.in = in_dev;
  p.tw = l->tw;
  p.spectra = l->spectra;
  p.out = out_dev;
  p.records = (uint32_t*)records_dev;
  p.n_in = (int64_t)n_in;
  p.base0 = (int64_t)(seg0 * hop - pos0);                                // in (first - S, first]: the difference is exact modulo 2^64
  p.first = (int64_t)first;
  p.n = (int64_t)n;
  p.out_stride = ostride;
  p.n_units = n_units;
  p.n_segments = (uint32_t)n_segments;
  p.taps = (int32_t)l->n_taps;
  p.format = out_format;
  // the units in chunks of consecutive ones, a chunk a workgroup: no more workgroups than the chip holds at once, and
  // none without a unit
  uint64_t grid = persistent_grid(l, in_dtype, resident_blocks_per_cu, 4, n_units);
  p.chunk = (n_units + grid - 1) / grid;
  grid = (n_units + p.chunk - 1) / p.chunk;

  // ---- enqueue
  hipStream_t hs = (hipStream_t)hip_stream;
  if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_run(in_dtype, (unsigned)grid, hs, p, (const Job*)sl->dev);
  return stage_end(l, sl, hs, e, WHO);
}

}  // extern "C"
