// uc_dfsdm_api.cpp -- the C-ABI of include/uchirp_dfsdm.h on top of uc_dfsdm_kernel.hip: the check of a configuration, its
// gain and plan, one row of the definition in plain C (on the arithmetic of uc_dfsdm.hpp that the kernel compiles too), the
// word path's tables, the checks that are its own, the launch.  The object's base, create and destroy and the checks of the
// row matrices are the shared host layer's (uc_host.hpp: header-only, nothing crosses a library boundary):
// libuchirp_dfsdm.so stands alone.  A call reads no host array, so the base's staging slots stay empty.  No CPU compute path
// exists behind uc_dfsdm_run: without a usable HIP device uc_dfsdm_create fails.  Every entry point leaves the calling
// thread's current HIP device as it found it.
#include "../../include/uchirp_dfsdm.h"
#include "uc_host.hpp"
#include "uc_dfsdm.hpp"

using namespace uc_dfsdm_dev;

static_assert(UC_DFSDM_ORDER_FASTSINC == ORDER_FAST && UC_DFSDM_ORDER_MAX == ORDER_MAX && UC_DFSDM_RATIO_MAX == RATIO_MAX &&
                  UC_DFSDM_INTEGRATOR_MAX == INTEG_MAX && UC_DFSDM_SHIFT_MAX == SHIFT_MAX && UC_DFSDM_OFFSET_MIN == OUT_MIN &&
                  UC_DFSDM_OFFSET_MAX == OUT_MAX && UC_DFSDM_GAIN_MAX == GAIN_MAX && UC_DFSDM_STATE_WORDS == STATE_WORDS,
              "constants of uchirp_dfsdm.h");

struct uc_dfsdm : HostBase {
  uc_dfsdm_config cfg = {0, 0, 0, 0, 0};
  bool word_path = false;          // R is a multiple of 32
  int32_t* table = nullptr;        // device: the word path's tables (uc_dfsdm.hpp: Params::table)
};

namespace {

constexpr uint64_t WORDS_MAX = 1ull << 58;   // 32 * words fits a uint64 with room to spare

int check_config(const char* who, const uc_dfsdm_config* c) {
  if (!c) return fail(-EINVAL, "%s: cfg is NULL", who);
  if (c->order < 0 || c->order > ORDER_MAX) return fail(-EINVAL, "%s: order %d not in 0 (FastSinc) .. 5", who, c->order);
  if (c->ratio < 1 || c->ratio > RATIO_MAX) return fail(-EINVAL, "%s: ratio %u not in 1 .. 1024", who, c->ratio);
  if (c->integrator < 1 || c->integrator > INTEG_MAX) return fail(-EINVAL, "%s: integrator %u not in 1 .. 256", who, c->integrator);
  if (c->shift < 0 || c->shift > SHIFT_MAX) return fail(-EINVAL, "%s: shift %d not in 0 .. 31", who, c->shift);
  if (c->offset < OUT_MIN || c->offset > OUT_MAX) return fail(-EINVAL, "%s: offset %d not in -2^23 .. 2^23 - 1", who, c->offset);
  const uint64_t g = gain_of(c->order, c->ratio, c->integrator);
  if (g > GAIN_MAX)
    return fail(-EINVAL, "%s: full-scale gain %llu (order %d, ratio %u, integrator %u) exceeds 2^31 - 1", who, (unsigned long long)g, c->order,
                c->ratio, c->integrator);
  return 0;
}

int check_words(const char* who, uint64_t words_before, uint64_t n_words) {
  return words_before > WORDS_MAX || n_words > WORDS_MAX - words_before
             ? fail(-EINVAL, "%s: words_before + n_words exceeds 2^58", who)
             : 0;
}

uint64_t outputs_of(const uc_dfsdm_config& c, uint64_t words_before, uint64_t n_words) {
  const uint64_t period = (uint64_t)c.ratio * c.integrator;
  return 32 * (words_before + n_words) / period - 32 * words_before / period;
}

bool on_16_bytes(const void* p, size_t stride) { return ((uintptr_t)p & 15u) == 0 && (stride & 3u) == 0; }

// the host's emitter of uc_dfsdm.hpp's word_by_bits
struct RowSink {
  int32_t* out;
  size_t n;
  void operator()(int32_t w) { out[n++] = w; }
};

template <int ORDER>
size_t filter_row(const uc_dfsdm_config& c, const uint32_t* words, size_t n_words, uint64_t words_before, int32_t* state, int32_t* out) {
  State<ORDER> s;
  load_state(s, state);
  Phase ph = phase_of(words_before, c.ratio, c.integrator);
  RowSink sink = {out, 0};
  for (size_t j = 0; j < n_words; ++j) word_by_bits<ORDER>(s, words[j], ph, c.ratio, c.integrator, c.shift, c.offset, sink);
  store_state(s, state);
  return sink.n;
}

// Params::table for an order: entry e = 256 b + v; stages 0 .. 3 as 4 ints per entry, then stage 4 as one
template <int ORDER>
void fill_table(std::vector<int32_t>& t) {
  constexpr int N = State<ORDER>::N;
  for (int e = 0; e < TABLE_ENTRIES; ++e) {
    uint32_t v[N];
    table_entry(e >> 8, (uint32_t)e & 255u, v);
    for (int k = 0; k < N; ++k) (k < 4 ? t[4 * (size_t)e + k] : t[4 * (size_t)TABLE_ENTRIES + e]) = (int32_t)v[k];
  }
}

}  // namespace

extern "C" {

int uc_dfsdm_abi_version(void) { return UC_DFSDM_ABI_VERSION; }

const char* uc_dfsdm_last_error(void) { return g_err.c_str(); }

int uc_dfsdm_check(const uc_dfsdm_config* cfg) { return check_config("uc_dfsdm_check", cfg); }

uint64_t uc_dfsdm_gain(const uc_dfsdm_config* cfg) {
  if (!cfg || cfg->order < 0 || cfg->order > ORDER_MAX || cfg->ratio < 1 || cfg->ratio > RATIO_MAX || cfg->integrator < 1 ||
      cfg->integrator > INTEG_MAX)
    return 0;
  return gain_of(cfg->order, cfg->ratio, cfg->integrator);
}

int uc_dfsdm_plan(const uc_dfsdm_config* cfg, uint64_t words_before, uint64_t n_words, uint64_t* n_out) {
  static const char WHO[] = "uc_dfsdm_plan";
  if (int rc = check_config(WHO, cfg)) return rc;
  if (!n_out) return fail(-EINVAL, "uc_dfsdm_plan: n_out is NULL");
  if (int rc = check_words(WHO, words_before, n_words)) return rc;
  *n_out = outputs_of(*cfg, words_before, n_words);
  return 0;
}

int uc_dfsdm_filter_row(const uc_dfsdm_config* cfg, const uint32_t* words, size_t n_words, uint64_t words_before, int32_t state[16],
                        int32_t* out, size_t out_cap, size_t* n_out) {
  static const char WHO[] = "uc_dfsdm_filter_row";
  if (int rc = check_config(WHO, cfg)) return rc;
  if (!words || !state || !n_out) return fail(-EINVAL, "uc_dfsdm_filter_row: words, state or n_out is NULL");
  if (n_words == 0) return fail(-EINVAL, "uc_dfsdm_filter_row: n_words is 0");
  if (int rc = check_words(WHO, words_before, n_words)) return rc;
  const uint64_t want = outputs_of(*cfg, words_before, n_words);
  if (want > out_cap) return fail(-EINVAL, "uc_dfsdm_filter_row: out_cap %zu < the %llu outputs of the call", out_cap, (unsigned long long)want);
  if (want && !out) return fail(-EINVAL, "uc_dfsdm_filter_row: out is NULL");
  size_t n = 0;
  switch (cfg->order) {
    case 0: n = filter_row<0>(*cfg, words, n_words, words_before, state, out); break;
    case 1: n = filter_row<1>(*cfg, words, n_words, words_before, state, out); break;
    case 2: n = filter_row<2>(*cfg, words, n_words, words_before, state, out); break;
    case 3: n = filter_row<3>(*cfg, words, n_words, words_before, state, out); break;
    case 4: n = filter_row<4>(*cfg, words, n_words, words_before, state, out); break;
    default: n = filter_row<5>(*cfg, words, n_words, words_before, state, out); break;
  }
  *n_out = n;
  return 0;
}

int uc_dfsdm_create(int device, const uc_dfsdm_config* cfg, uc_dfsdm** out) {
  static const char WHO[] = "uc_dfsdm_create";
  if (!out) return fail(-EINVAL, "uc_dfsdm_create: out is NULL");
  *out = nullptr;
  if (int rc = check_config(WHO, cfg)) return rc;
  DeviceGuard guard;
  uc_dfsdm* l = nullptr;
  int rc = open(WHO, "UC_DFSDM_GRID", device, &l);
  if (rc) return rc;
  l->cfg = *cfg;
  l->word_path = cfg->ratio % 32 == 0;
  if (l->word_path) {
    std::vector<int32_t> host(5 * (size_t)TABLE_ENTRIES, 0);
    switch (cfg->order) {
      case 0: fill_table<0>(host); break;
      case 1: fill_table<1>(host); break;
      case 2: fill_table<2>(host); break;
      case 3: fill_table<3>(host); break;
      case 4: fill_table<4>(host); break;
      default: fill_table<5>(host); break;
    }
    hipError_t e;
    if ((e = hipMalloc((void**)&l->table, host.size() * sizeof(int32_t))) != hipSuccess ||
        (e = hipMemcpy(l->table, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess) {
      uc_dfsdm_destroy(l);
      return hip_fail(e, WHO, "the tables");
    }
  }
  *out = l;
  return 0;
}

void uc_dfsdm_destroy(uc_dfsdm* l) {
  if (!l) return;
  DeviceGuard guard;
  close_base(l);
  (void)hipDeviceSynchronize();      // the calls stage nothing and leave no event to wait for
  if (l->table) (void)hipFree(l->table);
  delete l;
}

int uc_dfsdm_run(uc_dfsdm* l, const uint32_t* pdm_dev, size_t n_rows, size_t n_words, size_t in_stride, uint64_t words_before,
                 int32_t* state_dev, int32_t* out_dev, size_t out_stride, void* hip_stream) {
  static const char WHO[] = "uc_dfsdm_run";
  // ---- checks: nothing is enqueued before the last of them
  if (!l) return fail(-EINVAL, "uc_dfsdm_run: obj is NULL");
  if (!pdm_dev || !state_dev || !out_dev) return fail(-EINVAL, "uc_dfsdm_run: pdm_dev, state_dev or out_dev is NULL");
  if (int rc = check_count(WHO, "n_rows", n_rows)) return rc;
  if (n_words == 0) return fail(-EINVAL, "uc_dfsdm_run: n_words is 0");
  if (int rc = check_words(WHO, words_before, n_words)) return rc;
  const uint64_t n_out = outputs_of(l->cfg, words_before, n_words);
  const size_t out_len = n_out ? (size_t)n_out : 1;                  // (a call without outputs: its rows count as one word wide)
  if (int rc = check_stride(WHO, "in_stride", in_stride, "n_words", n_words)) return rc;
  if (int rc = check_stride(WHO, "out_stride", out_stride, "n_out", (size_t)n_out)) return rc;
  const size_t istride = stride_or(in_stride, n_words), ostride = stride_or(out_stride, out_len);
  if (int rc = check_strides_max(WHO, istride, ostride)) return rc;
  if (int rc = check_extent(WHO, n_rows, istride, n_rows, ostride, 1ull << 58, "n_rows * out_stride")) return rc;
  if ((((uintptr_t)pdm_dev | (uintptr_t)state_dev | (uintptr_t)out_dev) & 3u) != 0)
    return fail(-EINVAL, "uc_dfsdm_run: pdm_dev, state_dev or out_dev is not a multiple of 4");
  const size_t in_bytes = span_bytes(n_rows, istride, n_words, 4), out_bytes = span_bytes(n_rows, ostride, out_len, 4);
  const size_t state_bytes = n_rows * STATE_WORDS * 4;
  if (int rc = check_disjoint(WHO, "out_dev", out_dev, out_bytes, "pdm_dev", pdm_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "pdm_dev", pdm_dev, in_bytes)) return rc;
  if (int rc = check_disjoint(WHO, "state_dev", state_dev, state_bytes, "out_dev", out_dev, out_bytes)) return rc;
  DeviceGuard guard;
  hipError_t e = hipSetDevice(l->device);
  if (e != hipSuccess) return hip_fail(e, WHO, "hipSetDevice");
  if (int rc = check_on_device(WHO, "pdm_dev", pdm_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "state_dev", state_dev, l->device)) return rc;
  if (int rc = check_on_device(WHO, "out_dev", out_dev, l->device)) return rc;

  Params p;
  memset(&p, 0, sizeof(p));
  p.in = pdm_dev;
  p.out = out_dev;
  p.state = state_dev;
  p.table = l->table;
  p.in_stride = istride;
  p.out_stride = ostride;
  p.n_words = n_words;
  p.n_out = n_out;
  p.n_rows = (uint32_t)n_rows;
  p.row_blocks = (uint32_t)((n_rows + LANES - 1) / LANES);
  p.ratio = l->cfg.ratio;
  p.integ = l->cfg.integrator;
  const Phase ph = phase_of(words_before, l->cfg.ratio, l->cfg.integrator);
  p.phase_r = ph.r;
  p.phase_i = ph.i;
  p.shift = l->cfg.shift;
  p.offset = l->cfg.offset;
  // a single row has no second row for its stride to misplace
  p.in_vec = on_16_bytes(pdm_dev, n_rows > 1 ? istride : 0) ? 1u : 0u;
  p.out_vec = on_16_bytes(out_dev, n_rows > 1 ? ostride : 0) ? 1u : 0u;
  // one one-wave workgroup per 64 rows; UC_DFSDM_GRID (under UC_TUNING=1) makes fewer of them walk the row blocks
  unsigned grid = p.row_blocks;
  if (l->grid_override && l->grid_override < grid) grid = l->grid_override;

  // ---- enqueue
  e = (hipError_t)launch_filter(l->cfg.order, l->word_path, grid, hip_stream, p);
  if (e != hipSuccess) return hip_fail(e, WHO, "launch");
  return 0;
}

}  // extern "C"
