// uc_duc_api.cpp -- the C-ABI of include/uchirp_duc.h on top of uc_duc_kernel.hip: the carrier's tables, the host functions of
// the definition (one channel of one row, and the sum and output stage, on the arithmetic of uc_duc.hpp that the kernel
// compiles too), the tap sets, the checks that are its own, the two launches.  The object's base, create and destroy, the
// staging of the four channel arrays and the checks of the row matrices are the shared host layer's (uc_host.hpp:
// header-only, nothing crosses a library boundary): libuchirp_duc.so stands alone.  No CPU compute path exists behind
// uc_duc_run: without a usable HIP device uc_duc_create fails.  Every entry point leaves the calling thread's current HIP
// device as it found it.
#include "../../include/uchirp_duc.h"
#include "uc_host.hpp"
#include "uc_duc.hpp"

#include <new>

using namespace uc_duc_dev;

static_assert(UC_DUC_IN_IQ == IN_IQ && UC_DUC_IN_I == IN_I && UC_DUC_OUT_F32 == OUT_F32 && UC_DUC_OUT_I16 == OUT_I16, "format values");
static_assert(UC_DUC_MAX_PHASE_TAPS == MAX_PHASE_TAPS && UC_DUC_MAX_INTERP == MAX_INTERP && UC_DUC_MAX_TAPS == MAX_TAPS && UC_DUC_MAX_SETS == MAX_SETS &&
                  UC_DUC_MAX_CHAN == MAX_CHAN && UC_DUC_STATE_SAMPLES == STATE_SAMPLES && UC_DUC_TABLE_WORDS == 2 * TABLE,
              "constants of uchirp_duc.h");

struct uc_duc : HostBase {
  float* taps_dev = nullptr;     // MAX_SETS x MAX_TAPS floats; n_sets x k_taps * interp of them in use
  float* tables_dev = nullptr;   // the coarse and the fine table: 2 x 2048 floats
  uint32_t n_sets = 0;
  int k_taps = 0;
  int interp = 0;
};

namespace {

constexpr uint64_t INDEX_MAX = 1ull << 63;   // (first + n_samples) * interp of a call

// the tables, once per process: cosine and sine in double, rounded once (as uc_ddc_api.cpp builds its own)
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

int check_in_format(const char* who, int f) { return f == IN_IQ || f == IN_I ? 0 : fail(-EINVAL, "%s: unknown input format %d", who, f); }
int check_out_format(const char* who, int f) { return f == OUT_F32 || f == OUT_I16 ? 0 : fail(-EINVAL, "%s: unknown output format %d", who, f); }

int check_interp(const char* who, int interp) {
  return interp < 1 || interp > MAX_INTERP ? fail(-EINVAL, "%s: interp %d not in 1 .. %d", who, interp, MAX_INTERP) : 0;
}

int check_taps(const char* who, const float* taps, size_t n_sets, int k_taps, int interp) {
  if (!taps) return fail(-EINVAL, "%s: taps is NULL", who);
  if (k_taps < 1 || k_taps > MAX_PHASE_TAPS) return fail(-EINVAL, "%s: k_taps %d not in 1 .. %d", who, k_taps, MAX_PHASE_TAPS);
  if (int rc = check_interp(who, interp)) return rc;
  if (k_taps * interp > MAX_TAPS) return fail(-EINVAL, "%s: k_taps * interp = %d > %d", who, k_taps * interp, MAX_TAPS);
  if (n_sets < 1 || n_sets > (size_t)MAX_SETS) return fail(-EINVAL, "%s: n_sets %zu not in 1 .. %d", who, n_sets, MAX_SETS);
  const size_t n_taps = (size_t)k_taps * (size_t)interp, n = n_sets * n_taps;
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(taps[k])) return fail(-EINVAL, "%s: set %zu: tap %zu is not finite", who, k / n_taps, k % n_taps);
  return 0;
}

// (first + n) * interp <= 2^63, without wrapping
bool position_ok(uint64_t first, uint64_t n, uint64_t interp) { return first <= INDEX_MAX && n <= INDEX_MAX - first && first + n <= INDEX_MAX / interp; }

template <int IN>
void filter_row(const float* h, int K, int L, const uint32_t* in, size_t n, uint64_t first, uint32_t step, uint32_t phase0, float* state, float* out) {
  constexpr size_t W = IN == IN_IQ ? 2 : 1;
  const Tables& tb = tables();
  // the state's 128 samples and the call's, converted
  std::vector<float> z((STATE_SAMPLES + n) * W);
  for (size_t j = 0; j < STATE_SAMPLES * W; ++j) z[j] = state[j];
  for (size_t i = 0; i < n * W; ++i) z[STATE_SAMPLES * W + i] = sample_of(in[i]);
  for (size_t mi = 0; mi < n; ++mi)
    for (int rho = 0; rho < L; ++rho) {
      const size_t at = STATE_SAMPLES + mi;
      float ai = 0.0f, aq = 0.0f;
      for (int k = 0; k < K; ++k) {
        const float t = h[rho + k * L];
        ai = chain(t, z[(at - (size_t)k) * W], ai);
        if (IN == IN_IQ) aq = chain(t, z[(at - (size_t)k) * W + 1], aq);
      }
      const uint64_t idx = (first + mi) * (uint64_t)L + (uint64_t)rho;
      const uint32_t ph = phase_of(phase0, step, idx);
      const float* cs = tb.coarse + 2 * (ph >> 22);
      const float* fs = tb.fine + 2 * ((ph >> 12) & (TABLE - 1));
      float c, s;
      carrier(cs[0], cs[1], fs[0], fs[1], &c, &s);
      out[mi * (size_t)L + (size_t)rho] = IN == IN_IQ ? mix_iq(ai, aq, c, s) : mix_i(ai, c);
    }
  for (size_t j = 0; j < STATE_SAMPLES * W; ++j) state[j] = z[n * W + j];
}

}  // namespace

extern "C" {

int uc_duc_abi_version(void) { return UC_DUC_ABI_VERSION; }

const char* uc_duc_last_error(void) { return g_err.c_str(); }

int uc_duc_carrier_tables(float coarse[2048], float fine[2048]) {
  if (!coarse || !fine) return fail(-EINVAL, "uc_duc_carrier_tables: coarse or fine is NULL");
  const Tables& tb = tables();
  memcpy(coarse, tb.coarse, sizeof(tb.coarse));
  memcpy(fine, tb.fine, sizeof(tb.fine));
  return 0;
}

int uc_duc_span(int interp) {
  if (int rc = check_interp("uc_duc_span", interp)) return rc;
  return (int)span_outputs((uint32_t)interp);
}

int uc_duc_filter_row(const float* taps, int k_taps, int interp, const void* in, int in_format, size_t n, uint64_t first, uint32_t step,
                      uint32_t phase0, float* state, float* out_f32) {
  static const char WHO[] = "uc_duc_filter_row";
  if (!in || !state || !out_f32) return fail(-EINVAL, "uc_duc_filter_row: in, state or out_f32 is NULL");
  if (int rc = check_in_format(WHO, in_format)) return rc;
  if (n == 0) return fail(-EINVAL, "uc_duc_filter_row: n is 0");
  if (int rc = check_taps(WHO, taps, 1, k_taps, interp)) return rc;
  if (!position_ok(first, n, (uint64_t)interp)) return fail(-EINVAL, "uc_duc_filter_row: (first + n) * interp > 2^63");
  const uint32_t* w = (const uint32_t*)in;
  try {
    if (in_format == IN_IQ)
      filter_row<IN_IQ>(taps, k_taps, interp, w, n, first, step, phase0, state, out_f32);
    else
      filter_row<IN_I>(taps, k_taps, interp, w, n, first, step, phase0, state, out_f32);
  } catch (const std::bad_alloc&) {
    return fail(-ENOMEM, "uc_duc_filter_row: %zu samples of working memory", n);
  }
  return 0;
}

int uc_duc_sum_row(const float* const* y, int n_chan, size_t n, void* out, int out_format, uint32_t* clipped) {
  static const char WHO[] = "uc_duc_sum_row";
  if (!y || !out) return fail(-EINVAL, "uc_duc_sum_row: y or out is NULL");
  if (n_chan < 1 || n_chan > MAX_CHAN) return fail(-EINVAL, "uc_duc_sum_row: n_chan %d not in 1 .. %d", n_chan, MAX_CHAN);
  for (int j = 0; j < n_chan; ++j)
    if (!y[j]) return fail(-EINVAL, "uc_duc_sum_row: y[%d] is NULL", j);
  if (n == 0) return fail(-EINVAL, "uc_duc_sum_row: n is 0");
  if (int rc = check_out_format(WHO, out_format)) return rc;
  uint32_t count = 0;
  for (size_t i = 0; i < n; ++i) {
    float sum = y[0][i];
    for (int j = 1; j < n_chan; ++j) sum = add_channel(sum, y[j][i]);
    if (out_format == OUT_F32) {
      ((float*)out)[i] = sum;
    } else {
      bool c;
      ((int16_t*)out)[i] = to_i16(sum, &c);
      count += c ? 1u : 0u;
    }
  }
  if (clipped) *clipped += count;
  return 0;
}

int uc_duc_create(int device, uc_duc** out) {
  if (!out) return fail(-EINVAL, "uc_duc_create: out is NULL");
  *out = nullptr;
  DeviceGuard guard;
  uc_duc* l = nullptr;
  int rc = open("uc_duc_create", "UC_DUC_GRID", device, &l);
  if (rc) return rc;
  const Tables& tb = tables();
  hipError_t e = hipMalloc((void**)&l->taps_dev, (size_t)MAX_SETS * MAX_TAPS * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&l->tables_dev, sizeof(Tables));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (l->taps_dev) (void)hipFree(l->taps_dev);
    close_base(l);
    delete l;
    return fail(-ENOMEM, "uc_duc_create: the tap sets and the carrier's tables: %s", hipGetErrorString(e));
  }
  static_assert(sizeof(Tables) == 4 * TABLE * sizeof(float), "coarse, then fine");
  if ((e = hipMemcpy(l->tables_dev, &tb, sizeof(Tables), hipMemcpyHostToDevice)) != hipSuccess) {
    (void)hipFree(l->taps_dev);
    (void)hipFree(l->tables_dev);
    close_base(l);
    delete l;
    return hip_fail(e, "uc_duc_create", "hipMemcpy");
  }
  *out = l;
  return 0;
}

void uc_duc_destroy(uc_duc* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  (void)hipDeviceSynchronize();      // a call that staged nothing left no event to wait for
  if (l->taps_dev) (void)hipFree(l->taps_dev);
  if (l->tables_dev) (void)hipFree(l->tables_dev);
  delete l;
}

int uc_duc_set_taps(uc_duc* l, const float* taps, size_t n_sets, int k_taps, int interp) {
  static const char WHO[] = "uc_duc_set_taps";
  if (!l) return fail(-EINVAL, "uc_duc_set_taps: duc is NULL");
  if (int rc = check_taps(WHO, taps, n_sets, k_taps, interp)) return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, WHO, "hipDeviceSynchronize");   // no launch may still read the old sets
  if ((e = hipMemcpy(l->taps_dev, taps, n_sets * (size_t)k_taps * (size_t)interp * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
    return hip_fail(e, WHO, "hipMemcpy");
  l->n_sets = (uint32_t)n_sets;
  l->k_taps = k_taps;
  l->interp = interp;
  return 0;
}

int uc_duc_run(uc_duc* l, const void* in_dev, int in_format, size_t n_in_rows, size_t in_stride, size_t n_rows, int n_chan, size_t n_samples,
               uint64_t first, const uint32_t* row_map, const uint32_t* set_index, const uint32_t* step, const uint32_t* phase0, float* state_dev,
               void* out_dev, int out_format, size_t out_stride, uint32_t* clip_dev, void* hip_stream) {
  static const char WHO[] = "uc_duc_run";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_duc_run: duc is NULL");
  if (!in_dev || !state_dev || !out_dev) return fail(-EINVAL, "uc_duc_run: in_dev, state_dev or out_dev is NULL");
  if (int rc = check_in_format(WHO, in_format)) return rc;
  if (int rc = check_out_format(WHO, out_format)) return rc;
  if (int rc = check_count(WHO, "n_in_rows", n_in_rows)) return rc;
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (n_chan < 1 || n_chan > MAX_CHAN) return fail(-EINVAL, "uc_duc_run: n_chan %d not in 1 .. %d", n_chan, MAX_CHAN);
  if (n_samples == 0) return fail(-EINVAL, "uc_duc_run: n_samples is 0");
  if (n_samples > STRIDE_MAX) return fail(-EINVAL, "uc_duc_run: stride too large");
  const size_t in_words = in_format == IN_IQ ? 2 : 1, row_floats = n_samples * in_words;
  if (int rc = check_stride(WHO, "in_stride", in_stride, "the row's floats", row_floats)) return rc;
  const size_t istride = stride_or(in_stride, row_floats);
  if (istride > STRIDE_MAX) return fail(-EINVAL, "uc_duc_run: stride too large");
  if (first > INDEX_MAX || n_samples > INDEX_MAX - first) return fail(-EINVAL, "uc_duc_run: (first + n_samples) * interp > 2^63");
  if (l->n_sets == 0) return fail(-EINVAL, "uc_duc_run: no taps: call uc_duc_set_taps first");
  const uint32_t interp = (uint32_t)l->interp, k_taps = (uint32_t)l->k_taps;
  if (!position_ok(first, n_samples, interp)) return fail(-EINVAL, "uc_duc_run: (first + n_samples) * interp > 2^63");
  const size_t count = n_samples * (size_t)interp;                              // a row's outputs
  if (stride_or(out_stride, count) < count) return fail(-EINVAL, "uc_duc_run: out_stride %zu < the row's %zu outputs", out_stride, count);
  const size_t ostride = stride_or(out_stride, count);
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_in_rows, istride, n_rows, ostride, 1ull << 58, "n_rows * out_stride")) return rc;
  const size_t out_elem = out_format == OUT_F32 ? 4 : 2;
  if ((((uintptr_t)in_dev | (uintptr_t)state_dev | (uintptr_t)clip_dev) & 3u) != 0)
    return fail(-EINVAL, "uc_duc_run: in_dev, state_dev or clip_dev is not a multiple of 4");
  if (((uintptr_t)out_dev & (out_elem - 1)) != 0) return fail(-EINVAL, "uc_duc_run: out_dev is not a multiple of %zu", out_elem);
  const size_t in_bytes = span_bytes(n_in_rows, istride, row_floats, 4);
  const size_t out_bytes = span_bytes(n_rows, ostride, count, out_elem);
  const size_t state_bytes = n_in_rows * STATE_SAMPLES * in_words * sizeof(float);
  const size_t clip_bytes = n_rows * sizeof(uint32_t);
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, out_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "in_dev", in_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "out_dev", out_dev, out_bytes)) return rc;
  if (clip_dev) {
    if (int rc = check_disjoint(WHO, "clip_dev", clip_dev, clip_bytes, "in_dev", in_dev, in_bytes)) return rc;
    if (int rc = check_disjoint(WHO, "clip_dev", clip_dev, clip_bytes, "out_dev", out_dev, out_bytes)) return rc;
    if (int rc = check_disjoint(WHO, "clip_dev", clip_dev, clip_bytes, "state_dev", state_dev, state_bytes)) return rc;
  }
  const size_t slots = n_rows * (size_t)n_chan;
  if (!row_map && slots > n_in_rows)
    return fail(-EINVAL, "uc_duc_run: n_rows * n_chan = %zu > n_in_rows %zu without a row_map", slots, n_in_rows);
  if (row_map)
    for (size_t i = 0; i < slots; ++i)
      if (row_map[i] >= n_in_rows) return fail(-EINVAL, "uc_duc_run: row_map[%zu] = %u; n_in_rows %zu", i, row_map[i], n_in_rows);
  if (set_index)
    for (size_t i = 0; i < slots; ++i)
      if (set_index[i] >= l->n_sets) return fail(-EINVAL, "uc_duc_run: set_index[%zu] = %u; %u sets", i, set_index[i], l->n_sets);
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "in_dev", in_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "state_dev", state_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;
  if (clip_dev)
    if (int rc = check_on_device(WHO, "clip_dev", clip_dev, l->device)) return rc;
  // the four host arrays travel through the staging pair as one record per channel; a call without them stages nothing
  const bool records = row_map || set_index || step || phase0;
  const size_t bytes = records ? slots * sizeof(Channel) : 0;
  StagingSlot* sl = nullptr;
  if (bytes)
    if (int rc = stage_begin(l, bytes, WHO, &sl)) return rc;

  // ---- stage
  Params p;
  memset(&p, 0, sizeof(p));
  if (sl) {
    Channel* host = (Channel*)sl->pinned;
    for (size_t i = 0; i < slots; ++i) {
      host[i].row = row_map ? row_map[i] : (uint32_t)i;
      host[i].set = set_index ? set_index[i] : 0u;
      host[i].step = step ? step[i] : 0u;
      host[i].phase0 = phase0 ? phase0[i] : 0u;
    }
    p.chan = (const Channel*)sl->dev;
  }
  p.in = (const uint32_t*)in_dev;
  p.out = out_dev;
  p.state = state_dev;
  p.clip = out_format == OUT_I16 ? clip_dev : nullptr;                          // (floats are never clipped)
  p.taps = l->taps_dev;
  p.tables = l->tables_dev;
  p.in_stride = istride;
  p.out_stride = ostride;
  p.n_samples = n_samples;
  p.first_out = first * interp;
  p.count = count;
  p.span = span_outputs(interp);
  p.span_in = span_inputs(interp);
  p.spans = (count + p.span - 1) / p.span;
  p.units = (uint64_t)n_rows * p.spans;
  p.n_in_rows = (uint32_t)n_in_rows;
  p.n_chan = (uint32_t)n_chan;
  p.k_taps = k_taps;
  p.interp = interp;
  p.recip = span_recip(interp);
  // a single row has no second row for its stride to misplace
  p.in_vec = in_format == IN_IQ && ((uintptr_t)in_dev & 7u) == 0 && (n_in_rows == 1 || (istride & 1u) == 0) ? 1u : 0u;
  // four workgroups per CU walk the units; UC_DUC_GRID (under UC_TUNING=1) makes fewer of them do it
  uint64_t grid = (uint64_t)l->cus * 4;
  if (l->grid_override && l->grid_override < grid) grid = l->grid_override;
  if (grid > p.units) grid = p.units;
  const uint64_t state_grid = n_in_rows < 65536 ? n_in_rows : 65536;

  // ---- enqueue: the conversion, then behind it the states
  hipStream_t hs = (hipStream_t)hip_stream;
  if (sl)
    if (int rc = stage_copy(sl, bytes, hs, WHO)) return rc;
  e = (hipError_t)launch_convert(in_format, out_format, (unsigned)grid, hs, p);
  if (e == hipSuccess) e = (hipError_t)launch_state(in_format, (unsigned)state_grid, hs, p);
  if (sl) return stage_end(l, sl, hs, e, WHO);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  return 0;
}

}  // extern "C"
