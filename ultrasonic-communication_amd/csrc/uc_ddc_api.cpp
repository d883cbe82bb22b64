// uc_ddc_api.cpp -- the C-ABI of include/uchirp_ddc.h on top of uc_ddc_kernel.hip: the carrier's tables, the outputs of a
// call, the host function of the definition (one row, on the arithmetic of uc_ddc.hpp that the kernel compiles too), the tap
// sets, the checks that are its own, the two launches.  The object's base, create and destroy, the staging of the four row
// arrays and the checks of the row matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library
// boundary): libuchirp_ddc.so stands alone.  No CPU compute path exists behind uc_ddc_run: without a usable HIP device
// uc_ddc_create fails.  Every entry point leaves the calling thread's current HIP device as it found it.
#include "../../include/uchirp_ddc.h"
#include "uc_host.hpp"
#include "uc_ddc.hpp"

#include <new>

using namespace uc_ddc_dev;

static_assert(UC_DDC_DTYPE_I32 == DT_I32 && UC_DDC_DTYPE_F32 == DT_F32 && UC_DDC_OUT_IQ == FMT_IQ && UC_DDC_OUT_I == FMT_I, "dtype and format values");
static_assert(UC_DDC_MAX_TAPS == MAX_TAPS && UC_DDC_MAX_DECIM == MAX_DECIM && UC_DDC_MAX_SETS == MAX_SETS && UC_DDC_STATE_WORDS == STATE_WORDS &&
                  UC_DDC_TABLE_WORDS == 2 * TABLE,
              "constants of uchirp_ddc.h");

struct uc_ddc : HostBase {
  float* taps_dev = nullptr;     // MAX_SETS x MAX_TAPS floats; n_sets x n_taps of them in use
  float* tables_dev = nullptr;   // the coarse and the fine table: 2 x 2048 floats
  uint32_t n_sets = 0;
  int n_taps = 0;
  int decim = 0;
};

namespace {

constexpr uint64_t INDEX_MAX = 1ull << 63;   // first + n_samples of a call

// the tables, once per process: cosine and sine in double, rounded once
struct Tables {
  float coarse[2 * TABLE], fine[2 * TABLE];
  Tables() {
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int i = 0; i < TABLE; ++i) {
      const double a = two_pi * (double)i / 1024.0, b = two_pi * (double)i / 1048576.0;
      coarse[2 * i] = (float)std::cos(a);
      coarse[2 * i + 1] = (float)std::sin(a);
      fine[2 * i] = (float)std::cos(b);
      fine[2 * i + 1] = (float)std::sin(b);
    }
  }
};

const Tables& tables() {
  static const Tables t;
  return t;
}

int check_format(const char* who, int format) { return format == FMT_IQ || format == FMT_I ? 0 : fail(-EINVAL, "%s: unknown output format %d", who, format); }

int check_decim(const char* who, int decim) {
  return decim < 1 || decim > MAX_DECIM ? fail(-EINVAL, "%s: decim %d not in 1 .. %d", who, decim, MAX_DECIM) : 0;
}

int check_taps(const char* who, const float* taps, size_t n_sets, int n_taps, int decim) {
  if (!taps) return fail(-EINVAL, "%s: taps is NULL", who);
  if (n_taps < 1 || n_taps > MAX_TAPS) return fail(-EINVAL, "%s: n_taps %d not in 1 .. %d", who, n_taps, MAX_TAPS);
  if (int rc = check_decim(who, decim)) return rc;
  if (n_sets < 1 || n_sets > (size_t)MAX_SETS) return fail(-EINVAL, "%s: n_sets %zu not in 1 .. %d", who, n_sets, MAX_SETS);
  const size_t n = n_sets * (size_t)n_taps;
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(taps[k])) return fail(-EINVAL, "%s: set %zu: tap %zu is not finite", who, k / (size_t)n_taps, k % (size_t)n_taps);
  return 0;
}

// the outputs p with first <= p D <= first + n - 1 (n >= 1, first + n <= 2^64)
void outputs_of(uint64_t first, uint64_t n, uint64_t decim, uint64_t* p_first, uint64_t* count) {
  const uint64_t lo = first / decim + (first % decim ? 1 : 0), hi = (first + (n - 1)) / decim;
  *p_first = lo;
  *count = hi >= lo ? hi - lo + 1 : 0;
}

template <int DT, int FMT>
void filter_row(const float* h, int n_taps, int decim, const uint32_t* in, size_t n, uint64_t first, uint32_t step, uint32_t phase0, float* state,
                float* out) {
  const Tables& tb = tables();
  // the state's 128 samples and the call's, converted; mixed once each
  std::vector<float> x(STATE_WORDS + n), mi(STATE_WORDS + n), mq(FMT == FMT_IQ ? STATE_WORDS + n : 0);
  for (int j = 0; j < STATE_WORDS; ++j) x[j] = state[j];
  for (size_t i = 0; i < n; ++i) x[STATE_WORDS + i] = sample_of<DT>(in[i]);
  for (size_t j = 0; j < STATE_WORDS + n; ++j) {
    const uint32_t ph = phase_of(phase0, step, first - STATE_WORDS + j);          // (wraps in front of 0, as the definition says)
    const float* cs = tb.coarse + 2 * (ph >> 22);
    const float* fs = tb.fine + 2 * ((ph >> 12) & (TABLE - 1));
    float c, s;
    carrier(cs[0], cs[1], fs[0], fs[1], &c, &s);
    mi[j] = mix(x[j], c);
    if (FMT == FMT_IQ) mq[j] = mix(x[j], s);
  }
  uint64_t p_first, count;
  outputs_of(first, n, (uint64_t)decim, &p_first, &count);
  const size_t lead = (size_t)(p_first * (uint64_t)decim - first);
  for (uint64_t o = 0; o < count; ++o) {
    const size_t at = STATE_WORDS + lead + (size_t)o * (size_t)decim;
    float ai = 0.0f, aq = 0.0f;
    for (int k = 0; k < n_taps; ++k) {
      ai = chain(h[k], mi[at - k], ai);
      if (FMT == FMT_IQ) aq = chain(h[k], mq[at - k], aq);
    }
    if (FMT == FMT_IQ) {
      out[2 * o] = ai;
      out[2 * o + 1] = aq;
    } else {
      out[o] = ai;
    }
  }
  for (int j = 0; j < STATE_WORDS; ++j) state[j] = x[n + j];
}

}  // namespace

extern "C" {

int uc_ddc_abi_version(void) { return UC_DDC_ABI_VERSION; }

const char* uc_ddc_last_error(void) { return g_err.c_str(); }

int uc_ddc_carrier_tables(float coarse[2048], float fine[2048]) {
  if (!coarse || !fine) return fail(-EINVAL, "uc_ddc_carrier_tables: coarse or fine is NULL");
  const Tables& tb = tables();
  memcpy(coarse, tb.coarse, sizeof(tb.coarse));
  memcpy(fine, tb.fine, sizeof(tb.fine));
  return 0;
}

int uc_ddc_outputs(uint64_t first, size_t n_samples, int decim, uint64_t* p_first, size_t* count) {
  static const char WHO[] = "uc_ddc_outputs";
  if (!p_first || !count) return fail(-EINVAL, "uc_ddc_outputs: p_first or count is NULL");
  if (int rc = check_decim(WHO, decim)) return rc;
  if (n_samples && first + (uint64_t)(n_samples - 1) < first) return fail(-EINVAL, "uc_ddc_outputs: first + n_samples > 2^64");
  if (n_samples == 0) {
    *p_first = first / (uint64_t)decim + (first % (uint64_t)decim ? 1 : 0);
    *count = 0;
    return 0;
  }
  uint64_t c;
  outputs_of(first, n_samples, (uint64_t)decim, p_first, &c);
  *count = (size_t)c;
  return 0;
}

int uc_ddc_span(int decim) {
  if (int rc = check_decim("uc_ddc_span", decim)) return rc;
  return (int)span_outputs((uint32_t)decim);
}

int uc_ddc_filter_row(const float* taps, int n_taps, int decim, const void* in, int dtype, size_t n, uint64_t first, uint32_t step,
                      uint32_t phase0, float state[128], float* out, int out_format) {
  static const char WHO[] = "uc_ddc_filter_row";
  if (!in || !state || !out) return fail(-EINVAL, "uc_ddc_filter_row: in, state or out is NULL");
  if (int rc = check_dtype(WHO, dtype)) return rc;
  if (int rc = check_format(WHO, out_format)) return rc;
  if (n == 0) return fail(-EINVAL, "uc_ddc_filter_row: n is 0");
  if (int rc = check_taps(WHO, taps, 1, n_taps, decim)) return rc;
  if (first > INDEX_MAX || n > INDEX_MAX - first) return fail(-EINVAL, "uc_ddc_filter_row: first + n > 2^63");
  const uint32_t* w = (const uint32_t*)in;
  try {
    if (dtype == DT_F32) {
      if (out_format == FMT_IQ)
        filter_row<DT_F32, FMT_IQ>(taps, n_taps, decim, w, n, first, step, phase0, state, out);
      else
        filter_row<DT_F32, FMT_I>(taps, n_taps, decim, w, n, first, step, phase0, state, out);
    } else {
      if (out_format == FMT_IQ)
        filter_row<DT_I32, FMT_IQ>(taps, n_taps, decim, w, n, first, step, phase0, state, out);
      else
        filter_row<DT_I32, FMT_I>(taps, n_taps, decim, w, n, first, step, phase0, state, out);
    }
  } catch (const std::bad_alloc&) {
    return fail(-ENOMEM, "uc_ddc_filter_row: %zu samples of working memory", n);
  }
  return 0;
}

int uc_ddc_create(int device, uc_ddc** out) {
  if (!out) return fail(-EINVAL, "uc_ddc_create: out is NULL");
  *out = nullptr;
  DeviceGuard guard;
  uc_ddc* l = nullptr;
  int rc = open("uc_ddc_create", "UC_DDC_GRID", device, &l);
  if (rc) return rc;
  const Tables& tb = tables();
  hipError_t e = hipMalloc((void**)&l->taps_dev, (size_t)MAX_SETS * MAX_TAPS * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&l->tables_dev, sizeof(Tables));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (l->taps_dev) (void)hipFree(l->taps_dev);
    close_base(l);
    delete l;
    return fail(-ENOMEM, "uc_ddc_create: the tap sets and the carrier's tables: %s", hipGetErrorString(e));
  }
  static_assert(sizeof(Tables) == 4 * TABLE * sizeof(float), "coarse, then fine");
  if ((e = hipMemcpy(l->tables_dev, &tb, sizeof(Tables), hipMemcpyHostToDevice)) != hipSuccess) {
    (void)hipFree(l->taps_dev);
    (void)hipFree(l->tables_dev);
    close_base(l);
    delete l;
    return hip_fail(e, "uc_ddc_create", "hipMemcpy");
  }
  *out = l;
  return 0;
}

void uc_ddc_destroy(uc_ddc* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  (void)hipDeviceSynchronize();      // a call that staged nothing left no event to wait for
  if (l->taps_dev) (void)hipFree(l->taps_dev);
  if (l->tables_dev) (void)hipFree(l->tables_dev);
  delete l;
}

int uc_ddc_set_taps(uc_ddc* l, const float* taps, size_t n_sets, int n_taps, int decim) {
  static const char WHO[] = "uc_ddc_set_taps";
  if (!l) return fail(-EINVAL, "uc_ddc_set_taps: ddc is NULL");
  if (int rc = check_taps(WHO, taps, n_sets, n_taps, decim)) return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, WHO, "hipDeviceSynchronize");   // no launch may still read the old sets
  if ((e = hipMemcpy(l->taps_dev, taps, n_sets * (size_t)n_taps * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
    return hip_fail(e, WHO, "hipMemcpy");
  l->n_sets = (uint32_t)n_sets;
  l->n_taps = n_taps;
  l->decim = decim;
  return 0;
}

int uc_ddc_run(uc_ddc* l, const void* in_dev, int in_dtype, size_t n_in_rows, size_t in_stride, size_t n_rows, size_t n_samples,
               uint64_t first, const uint32_t* row_map, const uint32_t* set_index, const uint32_t* step, const uint32_t* phase0,
               float* state_dev, float* out_dev, int out_format, size_t out_stride, void* hip_stream) {
  static const char WHO[] = "uc_ddc_run";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_ddc_run: ddc is NULL");
  if (!in_dev || !state_dev || !out_dev) return fail(-EINVAL, "uc_ddc_run: in_dev, state_dev or out_dev is NULL");
  if (int rc = check_dtype(WHO, in_dtype)) return rc;
  if (int rc = check_format(WHO, out_format)) return rc;
  if (int rc = check_count(WHO, "n_in_rows", n_in_rows)) return rc;
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (n_samples == 0) return fail(-EINVAL, "uc_ddc_run: n_samples is 0");
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_samples", n_samples)) return rc;
  const size_t istride = stride_or(in_stride, n_samples);
  if (istride > STRIDE_MAX) return fail(-EINVAL, "uc_ddc_run: stride too large");
  if (first > INDEX_MAX || n_samples > INDEX_MAX - first) return fail(-EINVAL, "uc_ddc_run: first + n_samples > 2^63");
  if (l->n_sets == 0) return fail(-EINVAL, "uc_ddc_run: no taps: call uc_ddc_set_taps first");
  uint64_t p_first, count;
  outputs_of(first, n_samples, (uint64_t)l->decim, &p_first, &count);
  const size_t words = (size_t)count * (out_format == FMT_IQ ? 2 : 1);          // a row's stored floats
  if (stride_or(out_stride, words) < words) return fail(-EINVAL, "uc_ddc_run: out_stride %zu < the row's %zu floats", out_stride, words);
  const size_t ostride = stride_or(out_stride, words ? words : 1);
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_in_rows, istride, n_rows, ostride, 1ull << 58, "n_rows * out_stride")) return rc;
  if ((((uintptr_t)in_dev | (uintptr_t)state_dev | (uintptr_t)out_dev) & 3u) != 0)
    return fail(-EINVAL, "uc_ddc_run: in_dev, state_dev or out_dev is not a multiple of 4");
  const size_t in_bytes = span_bytes(n_in_rows, istride, n_samples, 4);
  const size_t out_bytes = words ? span_bytes(n_rows, ostride, words, 4) : 4;   // (a call without outputs still names a buffer)
  const size_t state_bytes = n_in_rows * STATE_WORDS * sizeof(float);
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, out_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "out_dev", out_dev, out_bytes)) return rc;
  if (!row_map && n_rows > n_in_rows) return fail(-EINVAL, "uc_ddc_run: n_rows %zu > n_in_rows %zu without a row_map", n_rows, n_in_rows);
  if (row_map)
    for (size_t r = 0; r < n_rows; ++r)
      if (row_map[r] >= n_in_rows) return fail(-EINVAL, "uc_ddc_run: row_map[%zu] = %u; n_in_rows %zu", r, row_map[r], n_in_rows);
  if (set_index)
    for (size_t r = 0; r < n_rows; ++r)
      if (set_index[r] >= l->n_sets) return fail(-EINVAL, "uc_ddc_run: set_index[%zu] = %u; %u sets", r, set_index[r], l->n_sets);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "state_dev", state_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  // the four host arrays travel through the staging pair, in the order of the arguments; a call without them stages nothing
  const uint32_t* const arrays[4] = {row_map, set_index, step, phase0};
  size_t n_arrays = 0;
  for (const uint32_t* a : arrays) n_arrays += a ? 1 : 0;
  const size_t bytes = n_arrays * n_rows * sizeof(uint32_t);
  StagingSlot* sl = nullptr;
  if (bytes)
    if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  Params p;
  memset(&p, 0, sizeof(p));
  if (sl) {
    uint32_t* host = (uint32_t*)sl->pinned;
    const uint32_t* dev = (const uint32_t*)sl->dev;
    const uint32_t** const slots[4] = {&p.row_map, &p.set_index, &p.step, &p.phase0};
    for (int a = 0; a < 4; ++a)
      if (arrays[a]) {
        memcpy(host, arrays[a], n_rows * sizeof(uint32_t));
        *slots[a] = dev;
        host += n_rows;
        dev += n_rows;
      }
  }
  const uint32_t decim = (uint32_t)l->decim;
  p.in = in_dev;
  p.out = out_dev;
  p.state = state_dev;
  p.taps = l->taps_dev;
  p.tables = l->tables_dev;
  p.in_stride = istride;
  p.out_stride = ostride;
  p.n_samples = n_samples;
  p.first = first;
  p.count = count;
  p.span = span_outputs(decim);
  p.spans = (count + p.span - 1) / p.span;
  p.units = (uint64_t)n_rows * p.spans;
  p.n_in_rows = (uint32_t)n_in_rows;
  p.lead = (uint32_t)(p_first * decim - first);
  p.n_taps = (uint32_t)l->n_taps;
  p.decim = decim;
  p.plen = span_plen(decim);
  p.recip = span_recip(decim);
  // a single row has no second row for its stride to misplace
  p.out_vec = ((uintptr_t)out_dev & 7u) == 0 && (n_rows == 1 || (ostride & 1u) == 0) ? 1u : 0u;
  // four workgroups per CU walk the units; UC_DDC_GRID (under UC_TUNING=1) makes fewer of them do it
  uint64_t grid = (uint64_t)l->cus * 4;
  if (l->grid_override && l->grid_override < grid) grid = l->grid_override;
  if (grid > p.units) grid = p.units;
  const uint64_t state_grid = n_in_rows < 65536 ? n_in_rows : 65536;

  // ---- enqueue: the conversion, then behind it the states
  hipStream_t hs = (hipStream_t)hip_stream;
  if (sl)
    if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = hipSuccess;
  if (p.units) e = (hipError_t)launch_convert(in_dtype, out_format, (unsigned)grid, hs, p);
  if (e == hipSuccess) e = (hipError_t)launch_state(in_dtype, (unsigned)state_grid, hs, p);
  if (sl) return stage_end(l, sl, hs, e, WHO);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  return 0;
}

}  // extern "C"
